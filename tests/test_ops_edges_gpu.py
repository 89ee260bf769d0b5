"""GPU edge and dispatch-path tests for the HIP data-plane kernels.

test_ops_gpu.py compares every kernel with its CPU reference at friendly
shapes on the default dispatch path.  This module covers what that
leaves open: grid-stride second trips, the multi-chain CRC
instantiations, every LZ4 decoder geometry on both the single-wave and
the producer/consumer kernel (with guard bytes around every output
slot), the decoder's per-block error codes, the staged decoder path,
the untested compressor instantiations and encoding edges, both
compressors against a Python model of their match policy, and SHA-256
tail-page padding.  Every comparison is exact (bytes or integers)
against gf2, lz4py, lz4_match_model or hashlib; inputs come from
ops_edge_corpus.py and are seeded."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lz4_match_model as match_model  # noqa: E402
import ops_edge_corpus as corpus  # noqa: E402

from shipyard_amd.data import lz4py  # noqa: E402
from shipyard_amd.ops import gf2  # noqa: E402

pytestmark = pytest.mark.gpu


def _bytes(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _cuda(arr):
    if isinstance(arr, (bytes, bytearray)):
        arr = np.frombuffer(bytes(arr), dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(arr).copy()).cuda()


def _ints(t):
    return [int(x) for x in t.tolist()]


# ------------------------------------------------------------------ CRC32C
class TestCrcEdges:
    def test_v2_beyond_grid_cap(self):
        """514 chunks on a 512-workgroup grid: workgroups 0 and 1 take a
        second trip through the chunk loop and reuse lane_crc."""
        from shipyard_amd import ops

        chunk, n = 4096, 513 * 4096 + 7
        host = _bytes(101, n)
        d = _cuda(host)
        got = _ints(ops.crc32c_chunks(d, chunk_size=chunk))
        want = [int(w) for w in
                gf2.crc32c_chunks_numpy(host.tobytes(), chunk)]
        assert len(got) == 514
        assert got == want
        assert ops.crc32c_file_digest(d, chunk_size=chunk) == \
            gf2.crc32c(host.tobytes())

    def test_v3_beyond_grid_cap(self):
        """1025 full chunks on the 1024-workgroup v3 grid (workgroup 0
        reuses tiles[] / wave_crc) plus a 1-byte v2 tail chunk."""
        from shipyard_amd import ops

        chunk, n = 32768, 1025 * 32768 + 1
        host = _bytes(102, n)
        got = _ints(ops.crc32c_chunks(_cuda(host), chunk_size=chunk))
        want = [int(w) for w in
                gf2.crc32c_chunks_numpy(host.tobytes(), chunk)]
        assert len(got) == 1026
        assert got == want

    @pytest.mark.parametrize("chunk", [32768, 65536, 98304])
    def test_v3_chunk_sizes_raw(self, chunk):
        """One, two and three 32 KiB rounds per chunk (98304 is not a
        power of two), raw register values per chunk."""
        from shipyard_amd import ops

        host = _bytes(103 + chunk, 3 * chunk)
        got = _ints(ops.crc32c_chunks_coal_raw(_cuda(host),
                                               chunk_size=chunk))
        want = [gf2.crc32c_raw(host[c * chunk:(c + 1) * chunk].tobytes())
                for c in range(3)]
        assert got == want

    @pytest.mark.parametrize("chunk", [4096, 32768])
    def test_ragged_tails_through_wrapper(self, chunk):
        from shipyard_amd import ops

        host = _bytes(104, 3 * chunk)
        for n in (1, 15, 16, 17, chunk - 1, chunk + 1, 2 * chunk + 15,
                  3 * chunk - 1):
            data = host[:n]
            got = _ints(ops.crc32c_chunks(_cuda(data), chunk_size=chunk))
            want = [int(w) for w in
                    gf2.crc32c_chunks_numpy(data.tobytes(), chunk)]
            assert got == want, n

    def test_multi_chain_in_one_process(self, monkeypatch):
        """crc32c_chunks_kernel<2,9>, <4,10>, <8,11> and their
        in-register pairwise combine.  The chain count changes inside one
        process at one chunk size, so a matrix cache keyed without the
        chain count would hand the 9..11-level kernels the 8-level
        operator tensor cached by the first iteration."""
        from shipyard_amd import ops

        chunk = 32768
        n = 3 * chunk + 777
        host = _bytes(105, n)
        d = _cuda(host)
        want = [int(w) for w in
                gf2.crc32c_chunks_numpy(host.tobytes(), chunk)]
        monkeypatch.setenv("SHIPYARD_CRC_V3", "0")
        for chains in (1, 2, 4, 8):
            monkeypatch.setenv("SHIPYARD_CRC_CHAINS", str(chains))
            got = _ints(ops.crc32c_chunks(d, chunk_size=chunk))
            assert got == want, chains

    @pytest.mark.parametrize("chunk", [4096, 32768])
    def test_view_with_storage_offset(self, chunk):
        from shipyard_amd import ops

        buf = _cuda(_bytes(106, 4096 + 3 * chunk + 100))
        view = buf[4096:]
        assert view.storage_offset() == 4096 and view.data_ptr() % 16 == 0
        a = ops.crc32c_chunks(view, chunk_size=chunk)
        b = ops.crc32c_chunks(view.clone(), chunk_size=chunk)
        assert _ints(a) == _ints(b)
        host = view.cpu().numpy().tobytes()
        assert _ints(a) == [int(w) for w in
                            gf2.crc32c_chunks_numpy(host, chunk)]


# ----------------------------------------------------------------- SHA-256
def _sha_pages(host: np.ndarray, page: int) -> np.ndarray:
    raw = host.tobytes()
    ref = b"".join(hashlib.sha256(raw[o:o + page]).digest()
                   for o in range(0, len(raw), page))
    return np.frombuffer(ref, dtype=np.uint8).reshape(-1, 32)


class TestShaEdges:
    def test_beyond_grid_cap(self):
        """524,292 pages on 2048 x 256 threads: threads 0..3 digest a
        second page, the last of them the 57-byte tail page."""
        from shipyard_amd import ops

        n = 64 * 524288 + 64 * 3 + 57
        host = _bytes(201, n)
        got = ops.sha256_pages(_cuda(host), page_size=64).cpu().numpy()
        want = _sha_pages(host, 64)
        assert got.shape == want.shape == (524292, 32)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, "first differing page %d" % bad[0]

    @pytest.mark.parametrize("page", [64, 192, 4096])
    def test_tail_page_padding_behind_full_pages(self, page):
        from shipyard_amd import ops

        host = _bytes(202 + page, 4 * page)
        for t in (1, 55, 56, 57, 63, 64, 65, 119, 120):
            if t >= page:
                continue
            data = host[:3 * page + t]
            got = ops.sha256_pages(_cuda(data), page_size=page)
            got = got.cpu().numpy()
            assert np.array_equal(got, _sha_pages(data, page)), t

    def test_bad_page_size_is_rejected(self):
        from shipyard_amd import ops

        with pytest.raises(RuntimeError, match="-22"):
            ops.sha256_pages(_cuda(_bytes(203, 400)), page_size=100)


# -------------------------------------------------------------- LZ4 decode
_RAW_CAPS = [4096, 8192, 16384, 32768, 65536]


def _pc_effective_cap(raw_cap: int) -> int:
    # sy_lz4_decode_blocks_pc has 8/16/64 KiB instantiations only
    return 8192 if raw_cap <= 8192 else 16384 if raw_cap <= 16384 else 65536


class TestLz4DecodeEdges:
    @pytest.mark.parametrize("pc", [False, True])
    @pytest.mark.parametrize("raw_cap", _RAW_CAPS)
    def test_guarded_fuzz(self, raw_cap, pc):
        """Every decoder geometry, slots at stride raw_cap + 64 in a
        0xA5-filled tensor: payloads exact, every other byte untouched.
        For pc the set holds a >200-sequence block (ring wrap, unbatched
        tail publish)."""
        corpus.check_guarded_fuzz(raw_cap, pc, seed=raw_cap + int(pc))

    @pytest.mark.parametrize("pc", [False, True])
    def test_error_codes_in_mixed_launch(self, pc):
        """good, bad, good, bad, ... in one launch at raw_cap = 4096.

        Expected codes are the table in ops_edge_corpus for both
        kernels.  The producer of lz4_decode_pc_kernel runs the same
        checks in the same order as lz4_decode_kernel: literal-length
        TRUNC (producer loop `if (pos >= slen)` inside the litlen
        extension), OVERFLOW (`dtotal + litlen > rawlen || pos + litlen
        > slen`), offset TRUNC (`pos + 2 > slen`), match-length TRUNC,
        OFFSET (`offset == 0 || offset > dtotal`), match OVERFLOW
        (`dtotal + mlen > rawlen`) and MISMATCH once `pos == slen`.
        Every check precedes the src read or dst write it guards, and
        the consumer only executes records the producer has bounded.
        One difference: pc has no 4 KiB instantiation, raw_cap = 4096
        runs lz4_decode_pc_kernel<8192>, whose TOOBIG test is `rawlen >
        8192`; the toobig case therefore claims 8193 bytes there, and
        slots are spaced for the 8 KiB geometry."""
        raw_cap = 4096
        cap = _pc_effective_cap(raw_cap) if pc else raw_cap
        bad = corpus.malformed_lz4_cases(cap)
        rng_blocks = corpus.decode_fuzz_blocks(raw_cap, 31, many_seq=pc)
        acc = corpus.accepted_lz4_case()
        good = [(lz4py.compress_block(b), b) for b in rng_blocks]
        good.insert(1, (acc[1], acc[3]))
        streams, out_lens, expect, codes, names = [], [], [], [], []
        for i, (name, stream, out_len, code) in enumerate(bad):
            g_stream, g_raw = good[i % len(good)]
            streams += [g_stream, stream]
            out_lens += [len(g_raw), out_len]
            expect += [g_raw, b""]
            codes += [corpus.OK, code]
            names += ["good", name]
        streams.append(good[-1][0])
        out_lens.append(len(good[-1][1]))
        expect.append(good[-1][1])
        codes.append(corpus.OK)
        names.append("good")
        status, got, stride = corpus.guarded_decode(
            streams, out_lens, raw_cap, pc, stride=corpus.slot_stride(cap))
        assert status == codes, [
            (n, s, c) for n, s, c in zip(names, status, codes) if s != c]
        corpus.check_slots(got, stride, expect)

    @pytest.mark.parametrize("pc", [False, True])
    def test_incompressible_64k_block(self, pc):
        """in_len > out_len: the stream of a random 64 KiB block is
        longer than the block (65 794 bytes, inside the staged kernels'
        RAWCAP + 1024 - 48 limit)."""
        raw = _bytes(301, 65536).tobytes()
        stream = lz4py.compress_block(raw)
        assert len(stream) > len(raw)
        status, got, stride = corpus.guarded_decode(
            [stream], [len(raw)], 65536, pc)
        assert status == [corpus.OK]
        corpus.check_slots(got, stride, [raw])

    def test_staged_path_in_child_process(self):
        """SY_LZ4_NOSTAGE is read once per process, so the staged v3
        kernels (LDS-staged source, 16 B-aligned enclosing copy of an
        unaligned stream) run in one fresh child interpreter: every rung
        of the staged ladder, then the -22 rejection above the top rung,
        which must hold under this setting too."""
        here = os.path.dirname(os.path.abspath(__file__))
        root = os.path.dirname(here)
        code = (
            "import sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "import ops_edge_corpus as c\n"
            "c.check_guarded_fuzz(4096, False, 40)\n"
            "c.check_guarded_fuzz(8192, False, 41)\n"
            "c.check_guarded_fuzz(16384, False, 43)\n"
            "c.check_guarded_fuzz(32768, False, 44)\n"
            "c.check_guarded_fuzz(65536, False, 42)\n"
            "try:\n"
            "    c.guarded_decode([c.accepted_lz4_case()[1]], [5], 65537,\n"
            "                     False, stride=c.slot_stride(65536))\n"
            "except RuntimeError as e:\n"
            "    assert '-22' in str(e), e\n"
            "else:\n"
            "    raise AssertionError('raw_cap 65537 was accepted')\n"
            "print('OK')\n" % (here, root))
        # five geometries + interpreter and torch start-up
        res = subprocess.run(
            [sys.executable, "-c", code],
            env={**os.environ, "SY_LZ4_NOSTAGE": "0"}, timeout=300,
            capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert res.stdout.strip().splitlines()[-1] == "OK"

    @pytest.mark.parametrize("pc", [False, True])
    @pytest.mark.parametrize("raw_cap", [4097, 8193, 16385, 32769])
    def test_off_rung_routing(self, raw_cap, pc):
        """A raw_cap one past a rung runs the next compiled rung: a block
        of exactly that rung's size decodes, and in the same launch a
        block one byte longer is TOOBIG with its slot untouched.  An
        instantiation one rung too small would report the first block
        TOOBIG, one too large would accept the second."""
        rung = _pc_effective_cap(raw_cap) if pc else \
            next(c for c in _RAW_CAPS if c >= raw_cap)
        import random

        raw = corpus.mixed_content(random.Random(raw_cap + int(pc)), rung)
        stream = lz4py.compress_block(raw)
        status, got, stride = corpus.guarded_decode(
            [stream, stream], [rung, rung + 1], raw_cap, pc,
            stride=corpus.slot_stride(rung))
        assert status == [corpus.OK, corpus.ERR_TOOBIG]
        corpus.check_slots(got, stride, [raw, b""])

    @pytest.mark.parametrize("pc", [False, True])
    def test_raw_cap_above_top_rung_is_rejected(self, pc):
        """raw_cap = 65537 has no rung: the host wrapper returns -22
        before any launch."""
        name, stream, out_len, raw = corpus.accepted_lz4_case()
        with pytest.raises(RuntimeError, match="-22"):
            corpus.guarded_decode([stream], [out_len], 65537, pc,
                                  stride=corpus.slot_stride(65536))

    @pytest.mark.parametrize("pc", [False, True])
    def test_assembled_streams(self, pc):
        """Hand-assembled streams no greedy matcher emits, one launch at
        raw_cap = 4096: every offset/length relation of the match copy
        (single, strided loop, doubling with two and with many rounds),
        both literal paths, every length-extension shape, a 309-long
        chain of zero-literal sequences, a stream ending on a match, the
        empty stream and the lone token."""
        corpus.check_assembled(4096, pc)

    @pytest.mark.parametrize("pc", [False, True])
    @pytest.mark.parametrize("raw_cap", _RAW_CAPS)
    def test_far_reach(self, raw_cap, pc):
        """offset == dpos: the match reads dst[0] and ends on the last
        byte of the block and of the stream; offset == dpos + 1 in the
        next slot is ERR_OFFSET and leaves the slot untouched.  On the
        single-wave kernel the match ends on dst[RAWCAP - 1].  pc has no
        4 KiB or 32 KiB rung (lz4_decode.hip), so there raw_cap = 4096
        and 32768 end in the middle of dst[8192] and dst[65536]."""
        cap = _pc_effective_cap(raw_cap) if pc else raw_cap
        stream, raw, bad = corpus.far_reach(raw_cap)
        status, got, stride = corpus.guarded_decode(
            [stream, bad], [raw_cap, raw_cap], raw_cap, pc,
            stride=corpus.slot_stride(cap))
        assert status == [corpus.OK, corpus.ERR_OFFSET]
        corpus.check_slots(got, stride, [raw, b""])

    @pytest.mark.parametrize("pc", [False, True])
    def test_deep_errors_in_mixed_launch(self, pc):
        """Errors at sequence 1, 15, 16, 63, 64, 65 and the last one of
        a zero-literal chain and of an ordinary chain, interleaved with
        good blocks.  The codes are those of
        test_error_codes_in_mixed_launch's check order on both kernels;
        in lz4_decode_pc_kernel the producer raises them with a full or
        wrapped ring while the consumer still holds unread records, and
        no block may report DEADLOCK (6)."""
        corpus.check_deep_errors(pc)

    def test_pc_workgroup_decodes_second_block(self):
        """4096 + 40 blocks on the 4096-workgroup pc grid at raw_cap =
        8192: workgroup w decodes blocks w and w + 4096 and reuses dst,
        sbuf, ring and ctl.  Pairs, in both orders: deep-error block and
        good block (ctl[2] reset), TOOBIG block and good block (the
        `__syncthreads(); continue;` path), zero-literal chain and
        5-byte block (ring counters, short block in a used dst).

        First launch: blocks of at most 448 raw bytes in 512-byte slots;
        300 zero-literal sequences need 1200 raw bytes, so the chain
        here has 100 sequences (one ring wrap).  Second launch: the same
        pattern with the full ``zero_lit_chain`` in 4160-byte slots."""
        corpus.check_slot_reuse(4096, True, full_chain=False)
        corpus.check_slot_reuse(4096, True, full_chain=True)

    @pytest.mark.parametrize("nostage", [None, "0"])
    def test_single_wave_workgroup_decodes_second_block_in_child(
            self, nostage):
        """SY_LZ4_GRID is read once per process: a fresh child with
        SY_LZ4_GRID=3 decodes 3 + 40 blocks, so every workgroup of
        lz4_decode_kernel makes 14 or 15 trips through its block loop
        over the pairs of test_pc_workgroup_decodes_second_block (full
        ``zero_lit_chain``).  The second child adds SY_LZ4_NOSTAGE=0:
        the staged instantiation reuses sbuf as well.  Both children
        also decode the assembled blocks and the deep-error launch, in
        three trips per workgroup or more.

        The cap cannot be observed from outside (a capped and an
        uncapped launch write the same bytes), so the test also pins
        that the host wrapper still reads the variable under this name;
        the child checks that it arrived."""
        here = os.path.dirname(os.path.abspath(__file__))
        root = os.path.dirname(here)
        with open(os.path.join(root, "shipyard_amd", "ops", "csrc",
                               "lz4_decode.hip")) as f:
            assert 'sy_env_atoi("SY_LZ4_GRID", 0)' in f.read()
        code = (
            "import sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "import ops_edge_corpus as c\n"
            "from shipyard_amd import ops\n"
            "assert ops._env_atoi('SY_LZ4_GRID', 0) == 3\n"
            "c.check_slot_reuse(3, False, full_chain=True)\n"
            "c.check_slot_reuse(3, False, full_chain=False)\n"
            "c.check_assembled(4096, False)\n"
            "c.check_deep_errors(False)\n"
            "print('OK')\n" % (here, root))
        env = {k: v for k, v in os.environ.items() if k != "SY_LZ4_NOSTAGE"}
        env["SY_LZ4_GRID"] = "3"
        if nostage is not None:
            env["SY_LZ4_NOSTAGE"] = nostage
        # four small launches + interpreter and torch start-up
        res = subprocess.run(
            [sys.executable, "-c", code], env=env, timeout=300,
            capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert res.stdout.strip().splitlines()[-1] == "OK"


# --------------------------------------------------------- GPU compressors
def _gpu_compress(data: bytes, block_raw: int, screen: bool):
    """-> (list of compressed bytes or None per block, device slots,
    stride, lens)"""
    from shipyard_amd import ops

    d_out, stride, lens = ops.lz4_compress_blocks_gpu(
        _cuda(data), block_raw, screen=screen)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    lens_np = lens.numpy().view(np.uint32)
    blobs = []
    for b, ln in enumerate(int(x) for x in lens_np):
        blobs.append(bytes(host[b * stride:b * stride + ln].tobytes())
                     if ln else None)
    return blobs, d_out, stride, lens_np


def _raw_blocks(data: bytes, block_raw: int):
    return [data[o:o + block_raw] for o in range(0, len(data), block_raw)]


def _stored_size(blobs, raws):
    return sum(len(c) if c is not None else len(r)
               for c, r in zip(blobs, raws))


def _seeded(seed: int, n: int) -> bytes:
    import random

    return corpus.mixed_content(random.Random(seed), n)


class TestGpuCompressorEdges:
    @pytest.mark.parametrize("block_raw", [16384, 32768])
    def test_byte_identical_to_cpu(self, block_raw):
        """lz4_compress_kernel<16 KiB> and <32 KiB>."""
        from shipyard_amd import ops

        data = _seeded(block_raw, block_raw * 5 + 1234)
        cpu = ops.lz4_compress_blocks(data, block_raw)
        blobs, _, _, _ = _gpu_compress(data, block_raw, screen=False)
        assert len(blobs) == len(cpu) == 6
        for b, (got, ref) in enumerate(zip(blobs, cpu)):
            assert got == ref, b

    @pytest.mark.parametrize("block_raw", [16384, 32768, 65536])
    def test_screen_roundtrip_and_ratio(self, block_raw):
        """lz4_compress_screen_kernel<16 KiB>, <32 KiB> and <64 KiB>."""
        from shipyard_amd import ops

        data = _seeded(block_raw + 1, block_raw * 4 + 1234)
        raws = _raw_blocks(data, block_raw)
        blobs, _, _, _ = _gpu_compress(data, block_raw, screen=True)
        assert len(blobs) == len(raws)
        for b, (blob, raw) in enumerate(zip(blobs, raws)):
            if blob is None:
                continue
            assert len(blob) < len(raw), b
            assert lz4py.decompress_block(blob, len(raw)) == raw, b
        comp_v2 = _stored_size(blobs, raws)
        comp_v1 = _stored_size(ops.lz4_compress_blocks(data, block_raw),
                               raws)
        # bound taken from TestScreenCompressor.test_roundtrip_and_ratio
        assert comp_v2 <= comp_v1 * 1.25 + 1024, (comp_v1, comp_v2)

    @pytest.mark.parametrize("screen", [False, True])
    def test_block_raw_above_top_rung_is_rejected(self, screen):
        """block_raw = 64 KiB + 4 KiB has no rung in either matcher
        family: the host wrapper returns -22 before any launch."""
        from shipyard_amd import ops

        data = _cuda(_seeded(7, 65536 + 4096))
        with pytest.raises(RuntimeError, match="-22"):
            ops.lz4_compress_blocks_gpu(data, 65536 + 4096, screen=screen)

    @pytest.mark.parametrize("block_raw", [12288, 61440])
    def test_off_rung_block_sizes(self, block_raw):
        """block_raw between rungs: 12 KiB runs the 16 KiB and 60 KiB
        the 64 KiB instantiations of both matchers and of both decoders
        with every block shorter than RAWCAP.  The serial matcher is
        byte-identical to the CPU compressor, the screen matcher
        round-trips through lz4py, and the device slots of both decode
        on the GPU with raw_cap = block_raw into guarded slots."""
        from shipyard_amd import ops

        data = _seeded(block_raw + 2, 3 * block_raw + 1234)
        raws = _raw_blocks(data, block_raw)
        cpu = ops.lz4_compress_blocks(data, block_raw)
        assert len(raws) == len(cpu) == 4
        for screen in (False, True):
            blobs, d_out, stride, lens = _gpu_compress(
                data, block_raw, screen)
            if not screen:
                assert blobs == cpu
            kept = [b for b, blob in enumerate(blobs) if blob is not None]
            assert kept, "no compressible block"
            for b in kept:
                assert len(blobs[b]) < len(raws[b]), (screen, b)
                assert lz4py.decompress_block(
                    blobs[b], len(raws[b])) == raws[b], (screen, b)
            dev = d_out.device
            slot = corpus.slot_stride(block_raw)
            t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
            t32 = lambda v: torch.tensor(v, dtype=torch.int64).to(
                torch.uint32).to(dev)
            for pc in (False, True):
                out = torch.full((len(kept) * slot,), corpus.GUARD,
                                 dtype=torch.uint8, device=dev)
                status = ops.lz4_decode_blocks(
                    d_out, t64([b * stride for b in kept]),
                    t32([int(lens[b]) for b in kept]), out,
                    t64([i * slot for i in range(len(kept))]),
                    t32([len(raws[b]) for b in kept]), raw_cap=block_raw,
                    pc=pc)
                torch.cuda.synchronize()
                assert ops.lz4_all_ok(status), (screen, pc, status.cpu())
                corpus.check_slots(out.cpu().numpy(), slot,
                                   [raws[b] for b in kept])

    def test_shard_roundtrip_at_block_raw_12288(self):
        """shardfmt.pack_gpu then unpack_gpu at a block size between the
        8 and 16 KiB rungs returns the input (CRC-verified)."""
        from shipyard_amd.data import shardfmt

        data = _seeded(12288, 3 * 12288 + 1234)
        blob = shardfmt.pack_gpu(data, block_raw=12288)
        assert shardfmt.read_index(blob).block_raw == 12288
        got = shardfmt.unpack_gpu(blob)
        assert bytes(got.cpu().numpy().tobytes()) == data
        assert shardfmt.unpack_cpu(blob) == data

    @pytest.mark.parametrize("screen", [False, True])
    def test_encoding_edges(self, screen):
        """Length-extension bytes of exactly 0, literal runs around the
        15 and 270 thresholds, final blocks around the 13-byte minimum
        and an input that is an exact block multiple, at block_raw =
        4096: valid for lz4py and for the GPU decoder, and for the
        greedy matcher byte-identical to the CPU compressor."""
        from shipyard_amd import ops

        block_raw = 4096
        for name, data in corpus.compress_edge_blocks(block_raw):
            raws = _raw_blocks(data, block_raw)
            blobs, d_out, stride, lens = _gpu_compress(
                data, block_raw, screen)
            assert len(blobs) == len(raws), name
            if not screen:
                assert blobs == ops.lz4_compress_blocks(data, block_raw), \
                    name
            if name in ("final_5", "final_12"):
                assert int(lens[-1]) == 0, name
            kept = []
            for b, (blob, raw) in enumerate(zip(blobs, raws)):
                assert int(lens[b]) < len(raw), (name, b)
                if blob is None:
                    continue
                assert lz4py.decompress_block(blob, len(raw)) == raw, \
                    (name, b)
                kept.append(b)
            # decode the device-side slots in place on the GPU
            dev = d_out.device
            slot = corpus.slot_stride(block_raw)
            out = torch.full((len(kept) * slot,), corpus.GUARD,
                             dtype=torch.uint8, device=dev)
            t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
            t32 = lambda v: torch.tensor(v, dtype=torch.int64).to(
                torch.uint32).to(dev)
            status = ops.lz4_decode_blocks(
                d_out, t64([b * stride for b in kept]),
                t32([int(lens[b]) for b in kept]), out,
                t64([i * slot for i in range(len(kept))]),
                t32([len(raws[b]) for b in kept]), raw_cap=block_raw,
                pc=False)
            torch.cuda.synchronize()
            assert ops.lz4_all_ok(status), (name, status.cpu())
            corpus.check_slots(out.cpu().numpy(), slot,
                               [raws[b] for b in kept])


# ------------------------------------------- GPU matchers against the model
@functools.lru_cache(maxsize=None)
def _model_stream(screen: bool, block: bytes):
    fn = match_model.screen_model if screen else match_model.greedy_model
    return fn(block)


def _direct_compress(screen: bool, buf: bytes, in_off, in_len, stride: int,
                     raw_cap: int):
    """One launch through the C entry point with buffers of the test's
    own: slots GUARD-filled, lengths pre-filled with 0xFFFFFFFF.
    -> (slots as a numpy array, uint32 lengths)"""
    from shipyard_amd import ops

    n_blocks = len(in_len)
    d_data = _cuda(buf)
    assert d_data.data_ptr() % 16 == 0
    d_off = _cuda(np.asarray(in_off, dtype=np.uint64).view(np.int64))
    d_len = _cuda(np.asarray(in_len, dtype=np.uint32).view(np.int32))
    d_out = torch.full((n_blocks * stride,), corpus.GUARD,
                       dtype=torch.uint8, device="cuda")
    d_lens = torch.full((n_blocks,), -1, dtype=torch.int32, device="cuda")
    rc = ops._call("sy_lz4_compress_blocks_gpu2" if screen
                   else "sy_lz4_compress_blocks_gpu",
                   d_data, d_off, d_len, d_out, stride, d_lens, n_blocks,
                   raw_cap)
    assert rc == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_lens.cpu().numpy().view(np.uint32)


class TestGpuMatchersEqualModel:
    """Both compressor kernels byte for byte against lz4_match_model on
    the matcher corpus (pinned on the CPU by test_lz4_match_model.py)."""

    def _wrapper_launch(self, rung: int, screen: bool):
        names, slots = corpus.matcher_launch(rung)
        blobs, _, _, lens = _gpu_compress(b"".join(slots), rung, screen)
        want = [_model_stream(screen, s) for s in slots]
        assert [int(x) for x in lens] == [len(w) if w else 0 for w in want], \
            [n for n, x, w in zip(names, lens, want)
             if int(x) != (len(w) if w else 0)]
        assert blobs == want, [n for n, g, w in zip(names, blobs, want)
                               if g != w]
        return slots, want

    @pytest.mark.parametrize("rung", corpus.MATCHER_RUNGS)
    def test_serial_equals_model(self, rung):
        """One wrapper launch per rung, a corpus block per slot
        (zero-padded; the last block is rung - 1 bytes): lengths and
        bytes of lz4_compress_kernel equal greedy_model, length 0
        exactly where the model drops the block, and the CPU compressor
        agrees."""
        from shipyard_amd import ops

        slots, want = self._wrapper_launch(rung, screen=False)
        assert ops.lz4_compress_blocks(b"".join(slots), rung) == want

    @pytest.mark.parametrize("rung", corpus.MATCHER_RUNGS)
    def test_screen_equals_model(self, rung):
        """The same launch on lz4_compress_screen_kernel against
        screen_model: atomicMax makes its stream deterministic, so the
        comparison is exact."""
        self._wrapper_launch(rung, screen=True)

    @pytest.mark.parametrize("screen", [False, True])
    @pytest.mark.parametrize("rung", [4096, 65536])
    def test_slots_and_lens_are_guarded(self, rung, screen):
        """Direct launch with every corpus block at its own length (so
        fit_*, drop_at_*, tail_* and full_minus_1 keep their feature)
        and a 13-byte last block, in slots of rung + 64 bytes: every
        length is written and equals the model's, kept slots hold the
        model's stream, and no byte from in_len[b] to the stride (for a
        kept block: from its length) has changed.  cap = n, so a
        dropped block may have written below in_len[b] only."""
        cases = corpus.matcher_blocks(rung) + [("last_13", b"\x07" * 13)]
        stride = rung + corpus.SLOT_SLACK
        buf = b"".join(corpus.pad_slot(b, rung) for _, b in cases)
        in_len = [len(b) for _, b in cases]
        got, lens = _direct_compress(
            screen, buf, [i * rung for i in range(len(cases))], in_len,
            stride, rung)
        assert not (lens == 0xFFFFFFFF).any(), "a length was not written"
        want = [_model_stream(screen, b) for _, b in cases]
        assert [int(x) for x in lens] == [len(w) if w else 0 for w in want], \
            [c[0] for c, x, w in zip(cases, lens, want)
             if int(x) != (len(w) if w else 0)]
        assert any(w is None for w in want) and any(want)
        for i, ((name, block), w) in enumerate(zip(cases, want)):
            slot = got[i * stride:(i + 1) * stride]
            clean = len(block)
            if w is not None:
                assert bytes(slot[:len(w)].tobytes()) == w, name
                clean = len(w)
            assert (slot[clean:] == corpus.GUARD).all(), (
                name, clean + int(np.nonzero(
                    slot[clean:] != corpus.GUARD)[0][0]))

    @pytest.mark.parametrize("screen", [False, True])
    def test_workgroup_compresses_second_block(self, screen):
        """(1 << 20) + 64 blocks on the 1 << 20-workgroup grid at the
        4 KiB rung: workgroup w < 64 compresses blocks w and w + (1 <<
        20) and reuses sbuf and the hash table.  Block i reads source
        i % 61 of 61 small sources, so the two differ; a few of the
        first 64 blocks claim 4097 bytes, the `n > RAWCAP` `continue`
        in front of an ordinary second trip: length 0, slot untouched.
        Lengths and the whole 64 MiB slot array are compared in one
        vectorised step with the model on the 61 sources (bytes below
        in_len of a dropped block excepted)."""
        here = os.path.dirname(os.path.abspath(__file__))
        with open(os.path.join(os.path.dirname(here), "shipyard_amd", "ops",
                               "csrc", "lz4_compress_gpu.hip")) as f:
            assert ("grid = n_blocks < (1u << 20) ? n_blocks : (1u << 20)"
                    in f.read())
        buf, offs, src_lens, n_blocks = corpus.second_trip_launch()
        assert n_blocks > 1 << 20
        n_src, stride = len(offs), 64
        which = np.arange(n_blocks) % n_src
        toobig = np.asarray(corpus.SECOND_TRIP_TOOBIG)
        in_off = np.asarray(offs, dtype=np.uint64)[which]
        in_len = np.asarray(src_lens, dtype=np.uint32)[which]
        in_len[toobig] = 4097
        got, lens = _direct_compress(screen, buf, in_off, in_len, stride,
                                     4096)

        streams = [_model_stream(screen, buf[o:o + n])
                   for o, n in zip(offs, src_lens)]
        if not screen:
            assert any(streams) and not all(streams)
        tile = np.full((n_src, stride), corpus.GUARD, dtype=np.uint8)
        care = np.ones((n_src, stride), dtype=bool)
        for i, (w, n) in enumerate(zip(streams, src_lens)):
            if w is None:
                care[i, :n] = False
            else:
                tile[i, :len(w)] = np.frombuffer(w, dtype=np.uint8)
        want_lens = np.asarray([len(w) if w else 0 for w in streams],
                               dtype=np.uint32)[which]
        want_lens[toobig] = 0
        bad = np.nonzero(lens != want_lens)[0]
        assert bad.size == 0, (int(bad[0]), int(lens[bad[0]]))
        want, care = tile[which], care[which]
        want[toobig], care[toobig] = corpus.GUARD, True
        wrong = np.nonzero(
            ((got.reshape(n_blocks, stride) != want) & care).any(axis=1))[0]
        assert wrong.size == 0, "first differing slot %d (source %d)" % (
            wrong[0], wrong[0] % n_src)
