"""GPU tests of the SYSHARD pipeline above the kernels: shardfmt.pack_gpu
/ decode_device / unpack_gpu and integrity.compute_gpu, end to end.

test_ops_edges_gpu.py pins each kernel; this module pins the layer the
replicator, the OCI ingest, the object store and the DDP recipe call.
Every comparison is exact (bytes or integers) against shardfmt.unpack_cpu,
lz4py, gf2, hashlib or the raw input; inputs are the seeded shard corpus
of ops_edge_corpus.py (whose stored/compressed layout is pinned on the
CPU by test_shard_index_validation.py).  Only payload bytes are ever
corrupted here: bad block tables and misaligned pointers are rejected on
the host and are tested there, through stub ops."""
import functools
import hashlib
import os
import random
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ops_edge_corpus as corpus  # noqa: E402

from shipyard_amd.data import integrity, lz4py, shardfmt  # noqa: E402
from shipyard_amd.ops import gf2  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = corpus.SHARD_BLOCK_SIZES
FINALS = list(corpus.SHARD_FINALS)
GUARD = corpus.GUARD


@functools.lru_cache(maxsize=None)
def _data(block_raw: int, final: str) -> bytes:
    return corpus.shard_corpus(block_raw, final)


@functools.lru_cache(maxsize=None)
def _packed(block_raw: int, final: str) -> bytes:
    """CPU-written reference shard (computed once per case, shared)."""
    return shardfmt.pack(_data(block_raw, final), block_raw=block_raw)


def _cuda(raw: bytes):
    if not raw:
        return torch.empty(0, dtype=torch.uint8, device="cuda:0")
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda:0")


def _host(t) -> bytes:
    return bytes(t.cpu().numpy().tobytes())


# ------------------------------------------------------------ 1. read matrix
def _check_read(block_raw, final):
    data, packed = _data(block_raw, final), _packed(block_raw, final)
    assert shardfmt.unpack_cpu(packed) == data
    for verify in (True, False):
        got = shardfmt.unpack_gpu(packed, verify=verify)
        torch.cuda.current_stream().synchronize()
        assert got.numel() == len(data), verify
        assert _host(got) == data, verify


@pytest.mark.parametrize("block_raw", SIZES)
@pytest.mark.parametrize("final", FINALS)
def test_read_matrix(block_raw, final):
    _check_read(block_raw, final)


@pytest.mark.parametrize("block_raw", SIZES)
@pytest.mark.parametrize("final", FINALS)
def test_decode_from_a_view_returns_exactly_raw_size(block_raw, final):
    """The payload is a view into a larger guard-filled buffer (non-zero
    storage offset, bytes behind it).  The result is raw_size bytes, no
    more, and the decoder writes nothing into the payload buffer."""
    data, packed = _data(block_raw, final), _packed(block_raw, final)
    idx = shardfmt.read_index(packed)
    payload = packed[idx.payload_off:]
    lead, trail = 4096, 4096
    host = np.full(lead + len(payload) + trail, GUARD, dtype=np.uint8)
    host[lead:lead + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    big = torch.from_numpy(host.copy()).to("cuda:0")
    view = big[lead:lead + len(payload)]
    assert view.storage_offset() == lead and view.data_ptr() % 16 == 0
    dev = torch.device("cuda:0")
    for verify in (True, False):
        out = shardfmt.decode_device(view, idx, dev, verify=verify)
        torch.cuda.synchronize()
        assert out.numel() == idx.raw_size == len(data)
        assert _host(out) == data
    assert np.array_equal(big.cpu().numpy(), host)


# ----------------------------------------------------------- 2. write matrix
def _check_write(block_raw, final, as_tensor, monkeypatch):
    data, cpu_shard = _data(block_raw, final), _packed(block_raw, final)
    src = _cuda(data) if as_tensor else data

    monkeypatch.setenv("SHIPYARD_LZ4C_SCREEN", "0")
    greedy = shardfmt.pack_gpu(src, block_raw=block_raw)
    assert greedy == cpu_shard

    monkeypatch.setenv("SHIPYARD_LZ4C_SCREEN", "1")
    screen = shardfmt.pack_gpu(src, block_raw=block_raw)
    assert shardfmt.unpack_cpu(screen) == data
    idx = shardfmt.read_index(screen)
    payload = screen[idx.payload_off:]
    shardfmt.validate_index(idx, len(payload))
    assert idx.block_raw == block_raw and idx.raw_size == len(data)
    blocks = corpus.shard_blocks(data, block_raw)
    assert idx.n_blocks == len(blocks)
    covered = np.zeros(len(payload), dtype=bool)
    for b, raw in zip(idx.blocks, blocks):
        assert b.comp_off % 16 == 0
        assert b.raw_len == len(raw)
        assert b.crc32c == gf2.crc32c(raw)
        assert not covered[b.comp_off:b.comp_off + b.comp_len].any()
        covered[b.comp_off:b.comp_off + b.comp_len] = True
    pad = np.frombuffer(payload, dtype=np.uint8)[~covered]
    assert pad.size < 16 * len(blocks) and not pad.any()
    assert len(screen) <= len(cpu_shard) * 1.25 + 1024

    for shard in (greedy, screen):
        got = shardfmt.unpack_gpu(shard)
        torch.cuda.current_stream().synchronize()
        assert _host(got) == data
    if as_tensor:
        assert _host(src) == data  # the writer leaves its input alone


@pytest.mark.parametrize("as_tensor", [False, True], ids=["bytes", "tensor"])
@pytest.mark.parametrize("block_raw", SIZES)
@pytest.mark.parametrize("final", FINALS)
def test_write_matrix(block_raw, final, as_tensor, monkeypatch):
    _check_write(block_raw, final, as_tensor, monkeypatch)


@pytest.mark.parametrize("screen", ["0", "1"])
def test_pack_gpu_empty(screen, monkeypatch):
    monkeypatch.setenv("SHIPYARD_LZ4C_SCREEN", screen)
    for src in (b"", _cuda(b"")):
        blob = shardfmt.pack_gpu(src)
        assert len(blob) == shardfmt.HEADER.size
        idx = shardfmt.read_index(blob)
        assert idx.n_blocks == 0 and idx.raw_size == 0
        shardfmt.validate_index(idx, 0)
        assert shardfmt.unpack_cpu(blob) == b""
        got = shardfmt.unpack_gpu(blob)
        assert got.is_cuda and got.numel() == 0


# -------------------------------------------------------- 3. stored layouts
@pytest.mark.parametrize("block_raw", SIZES)
@pytest.mark.parametrize("final", ["equal_5", "random_bm1", "none"])
def test_stored_contiguous_is_a_view_of_the_payload(block_raw, final):
    data = _data(block_raw, final)
    packed = shardfmt.pack(data, block_raw=block_raw, compress=False)
    idx = shardfmt.read_index(packed)
    assert shardfmt._stored_contiguous(idx)
    d_comp = _cuda(packed[idx.payload_off:])
    dev = torch.device("cuda:0")
    for verify in (True, False):
        out = shardfmt.decode_device(d_comp, idx, dev, verify=verify)
        torch.cuda.synchronize()
        assert out.data_ptr() == d_comp.data_ptr()
        assert out.untyped_storage().data_ptr() == \
            d_comp.untyped_storage().data_ptr()
        assert out.numel() == len(data) and _host(out) == data
        got = shardfmt.unpack_gpu(packed, verify=verify)
        torch.cuda.synchronize()
        assert _host(got) == data


@pytest.mark.parametrize("block_raw", SIZES)
@pytest.mark.parametrize("final", ["equal_5", "random_bm1", "none"])
def test_stored_reversed_takes_gather_copy(block_raw, final):
    data = _data(block_raw, final)
    packed = corpus.reversed_stored_shard(data, block_raw)
    idx = shardfmt.read_index(packed)
    assert not shardfmt._stored_contiguous(idx)
    assert all(b.stored for b in idx.blocks)
    assert shardfmt.unpack_cpu(packed) == data
    d_comp = _cuda(packed[idx.payload_off:])
    dev = torch.device("cuda:0")
    for verify in (True, False):
        out = shardfmt.decode_device(d_comp, idx, dev, verify=verify)
        torch.cuda.synchronize()
        assert out.untyped_storage().data_ptr() != \
            d_comp.untyped_storage().data_ptr()
        assert out.numel() == len(data) and _host(out) == data


# ------------------------------------------- 4. corruption (payload only)
def _flip(packed: bytes, pos: int) -> bytes:
    bad = bytearray(packed)
    bad[pos] ^= 0x5A
    return bytes(bad)


@pytest.mark.parametrize("block_raw", [4096, 65536])
@pytest.mark.parametrize("final", ["equal_5", "zeros_25"])
def test_flipped_payload_byte_is_detected(block_raw, final):
    data, packed = _data(block_raw, final), _packed(block_raw, final)
    idx = shardfmt.read_index(packed)
    want_stored = [False, True, False, True]
    assert [b.stored for b in idx.blocks[:4]] == want_stored
    assert idx.blocks[-1].stored is corpus.SHARD_FINALS[final]
    assert idx.blocks[-1].raw_len < 32
    for bi in (0, 1, idx.n_blocks - 1):  # compressed, stored, final short
        b = idx.blocks[bi]
        for at in (0, b.comp_len // 2, b.comp_len - 1):
            bad = _flip(packed, idx.payload_off + b.comp_off + at)
            with pytest.raises(ValueError):
                shardfmt.unpack_cpu(bad)
            with pytest.raises(ValueError):
                shardfmt.unpack_gpu(bad, verify=True)
            torch.cuda.synchronize()
    # a pad byte belongs to no block: flipping it changes nothing
    padded = [b for b in idx.blocks if b.comp_len % 16]
    assert padded
    for b in (padded[0], padded[-1]):
        bad = _flip(packed, idx.payload_off + b.comp_off + b.comp_len)
        got = shardfmt.unpack_gpu(bad, verify=True)
        torch.cuda.synchronize()
        assert _host(got) == data


# ------------------------------------------------------------ 5. side stream
@pytest.mark.parametrize("final", FINALS)
def test_read_and_write_on_a_side_stream(final, monkeypatch):
    """The ops launch on torch's current stream; the whole matrix at
    8 KiB blocks again with a non-default stream current."""
    side = torch.cuda.Stream()
    assert side != torch.cuda.default_stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        _check_read(8192, final)
        _check_write(8192, final, False, monkeypatch)
        _check_write(8192, final, True, monkeypatch)
        side.synchronize()


# ------------------------------------------------- 6. alignment contract
class TestAlignmentContract:
    """buf[1:] is contiguous uint8 but not 16-byte aligned: ValueError on
    the host, nothing reaches the device.  buf[16:] is an aligned view
    with a storage offset and must match the reference."""

    N = 3 * 32768

    @pytest.fixture(scope="class")
    def host(self):
        return corpus.mixed_content(random.Random(61), self.N + 32)

    @pytest.fixture(scope="class")
    def buf(self, host):
        return _cuda(host)

    def _views(self, buf, host, n):
        bad = buf[1:1 + n]
        ok = buf[16:16 + n]
        assert bad.is_contiguous() and bad.data_ptr() % 16 == 1
        assert ok.data_ptr() % 16 == 0 and ok.storage_offset() == 16
        return bad, ok, host[16:16 + n]

    @pytest.mark.parametrize("chunk", [4096, 32768])
    def test_crc32c_chunks(self, buf, host, chunk):
        from shipyard_amd import ops

        bad, ok, ref = self._views(buf, host, self.N - 100)
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.crc32c_chunks(bad, chunk_size=chunk)
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.crc32c_file_digest(bad, chunk_size=chunk)
        got = [int(x) for x in ops.crc32c_chunks(ok, chunk_size=chunk)
               .tolist()]
        assert got == [int(w) for w in gf2.crc32c_chunks_numpy(ref, chunk)]
        assert ops.crc32c_file_digest(ok, chunk_size=chunk) == \
            gf2.crc32c(ref)

    def test_crc32c_chunks_coal_raw(self, buf, host):
        from shipyard_amd import ops

        chunk = 32768
        bad, ok, ref = self._views(buf, host, 2 * chunk)
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.crc32c_chunks_coal_raw(bad, chunk_size=chunk)
        got = [int(x) for x in
               ops.crc32c_chunks_coal_raw(ok, chunk_size=chunk).tolist()]
        assert got == [gf2.crc32c_raw(ref[:chunk]),
                       gf2.crc32c_raw(ref[chunk:])]

    def test_sha256_pages(self, buf, host):
        from shipyard_amd import ops

        bad, ok, ref = self._views(buf, host, 5 * 4096 + 57)
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.sha256_pages(bad, page_size=4096)
        got = _host(ops.sha256_pages(ok, page_size=4096))
        assert got == b"".join(hashlib.sha256(ref[o:o + 4096]).digest()
                               for o in range(0, len(ref), 4096))

    @pytest.mark.parametrize("screen", [False, True],
                             ids=["greedy", "screen"])
    def test_lz4_compress_blocks_gpu(self, buf, host, screen):
        from shipyard_amd import ops

        block = 4096
        bad, ok, ref = self._views(buf, host, 5 * block + 321)
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.lz4_compress_blocks_gpu(bad, block, screen=screen)
        d_out, stride, lens = ops.lz4_compress_blocks_gpu(ok, block,
                                                          screen=screen)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        lens = lens.numpy().view(np.uint32)
        cpu = ops.lz4_compress_blocks(ref, block)
        assert len(lens) == len(cpu) == 6
        for b, raw in enumerate(corpus.shard_blocks(ref, block)):
            ln = int(lens[b])
            got = bytes(out[b * stride:b * stride + ln].tobytes())
            if not screen:
                assert (got if ln else None) == cpu[b], b
            if ln:
                assert ln < len(raw)
                assert lz4py.decompress_block(got, len(raw)) == raw, b

    @pytest.mark.parametrize("pc", [False, True], ids=["wave", "pc"])
    def test_lz4_decode_blocks_out_and_comp(self, pc):
        from shipyard_amd import ops

        rng = random.Random(62)
        raws = [corpus.text_like(rng, 4096), b"\x11" * 4096,
                corpus.mixed_content(rng, 1001)]
        streams = [lz4py.compress_block(r) for r in raws]
        # streams back to back, so in_off is unaligned; on the default
        # (byte-parsing) path the comp base is an unaligned view too
        comp = _cuda(b"\0" + b"".join(streams) + b"\0" * 16)[1:]
        assert comp.data_ptr() % 16 == 1
        unaligned = comp
        if pc:  # uint4 staging from comp + (in_off & ~15): aligned base
            comp = comp.clone()
            assert comp.data_ptr() % 16 == 0
        in_off = np.cumsum([0] + [len(s) for s in streams[:-1]])
        dev = comp.device
        t64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)
        t32 = lambda v: torch.tensor(list(v), dtype=torch.int64).to(
            torch.uint32).to(dev)
        args = (t64(in_off), t32(len(s) for s in streams))
        oargs = (t64(i * 4096 for i in range(3)),
                 t32(len(r) for r in raws))
        big = torch.full((16 + 3 * 4096 + 16,), GUARD, dtype=torch.uint8,
                         device=dev)
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.lz4_decode_blocks(comp, *args, big[1:], *oargs,
                                  raw_cap=4096, pc=pc)
        if pc:
            with pytest.raises(ValueError, match="comp base pointer"):
                ops.lz4_decode_blocks(unaligned, *args, big[16:], *oargs,
                                      raw_cap=4096, pc=True)
        torch.cuda.synchronize()
        assert bool((big == GUARD).all().item())  # nothing was launched
        out = big[16:]
        status = ops.lz4_decode_blocks(comp, *args, out, *oargs,
                                       raw_cap=4096, pc=pc)
        torch.cuda.synchronize()
        assert ops.lz4_all_ok(status)
        got = big.cpu().numpy()
        want = np.full(got.shape, GUARD, dtype=np.uint8)
        for i, r in enumerate(raws):
            lo = 16 + i * 4096
            want[lo:lo + len(r)] = np.frombuffer(r, dtype=np.uint8)
        assert np.array_equal(got, want)

    def test_pipeline_entry_points_inherit_it(self, buf, host):
        bad, ok, ref = self._views(buf, host, 2 * 8192 + 500)
        with pytest.raises(ValueError, match="16-byte aligned"):
            shardfmt.pack_gpu(bad, block_raw=8192)
        with pytest.raises(ValueError, match="16-byte aligned"):
            integrity.compute_gpu(bad, chunk_size=4096)
        assert shardfmt.unpack_cpu(
            shardfmt.pack_gpu(ok, block_raw=8192)) == ref
        assert integrity.verify(integrity.compute_cpu(ref, 4096),
                                integrity.compute_gpu(ok, 4096))


# --------------------------------------------------------------- 7. manifests
MANIFEST_CHUNKS = [4096, 65536, 262144]
MANIFEST_LENGTHS = {
    "0": lambda c: 0, "1": lambda c: 1, "chunk-1": lambda c: c - 1,
    "chunk": lambda c: c, "chunk+1": lambda c: c + 1,
    "3*chunk+777": lambda c: 3 * c + 777,
}


@functools.lru_cache(maxsize=None)
def _manifest_bytes() -> bytes:
    return random.Random(71).randbytes(3 * 262144 + 777)


@pytest.mark.parametrize("chunk", MANIFEST_CHUNKS)
@pytest.mark.parametrize("length", list(MANIFEST_LENGTHS))
def test_manifest_gpu_matches_cpu(chunk, length):
    n = MANIFEST_LENGTHS[length](chunk)
    data = _manifest_bytes()[:n]
    m_cpu = integrity.compute_cpu(data, chunk_size=chunk)
    m_gpu = integrity.compute_gpu(_cuda(data), chunk_size=chunk)
    assert m_gpu.length == n and m_gpu.chunk_size == chunk
    assert m_gpu.chunk_crc32c == [int(c) for c in m_cpu.chunk_crc32c]
    assert len(m_gpu.chunk_crc32c) == (n + chunk - 1) // chunk
    assert m_gpu.sha256_root == m_cpu.sha256_root
    assert integrity.verify(m_cpu, m_gpu) and integrity.verify(m_gpu, m_cpu)
    if n == 0:
        return
    # one changed byte: exactly one CRC entry and the root change, and
    # they change to the reference's values (gf2 / hashlib directly)
    pos = n - 1 if n <= chunk + 1 else chunk + 5
    changed = bytearray(data)
    changed[pos] ^= 0x01
    changed = bytes(changed)
    m2 = integrity.compute_gpu(_cuda(changed), chunk_size=chunk)
    diff = [i for i, (a, b) in
            enumerate(zip(m_gpu.chunk_crc32c, m2.chunk_crc32c)) if a != b]
    assert diff == [pos // chunk]
    c = pos // chunk
    assert m2.chunk_crc32c[c] == gf2.crc32c(
        changed[c * chunk:(c + 1) * chunk])
    root = hashlib.sha256(b"".join(
        hashlib.sha256(changed[o:o + chunk]).digest()
        for o in range(0, n, chunk))).hexdigest()
    assert m2.sha256_root == root != m_gpu.sha256_root
    assert not integrity.verify(m_gpu, m2)
