"""CPU tests for shardfmt.validate_index and the host side of the GPU
reader/writer contracts.

decode_device hands comp_off / comp_len / raw_len from the shard's block
table to kernels as device offsets, so a bad table must be rejected
before anything is launched.  Every rejection here runs decode_device
through the strict CPU stub ops (tests/shard_stub_ops.py) and asserts
both the ValueError and that the stub recorded zero launches; no bad
table and no misaligned pointer is ever fed to a kernel.  The good-table
tests and the corpus pins keep the inputs of test_shard_edges_gpu.py
honest on every host."""
import os
import random
import sys
import time
from unittest import mock

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ops_edge_corpus as corpus  # noqa: E402
from shard_stub_ops import CpuOps, decode  # noqa: E402

from shipyard_amd.data import lz4py, shardfmt  # noqa: E402

B = 4096
U64 = (1 << 64) - 1


def _split(packed: bytes):
    """-> (flags, block_raw, raw_size, writable table copy, payload)."""
    _, flags, block_raw, raw_size, n = shardfmt.HEADER.unpack_from(packed, 0)
    idx = shardfmt.read_index(packed)
    return (flags, block_raw, raw_size, idx.table.copy(),
            packed[idx.payload_off:])


def _join(flags, block_raw, raw_size, table, payload) -> bytes:
    return (shardfmt.HEADER.pack(shardfmt.MAGIC, flags, block_raw, raw_size,
                                 len(table))
            + table.tobytes() + payload)


@pytest.fixture(scope="module")
def good():
    """The good 6-block shard at block_raw=4096: text, random, byte run,
    random, mixed, then 2048 random bytes.  The final block is stored
    and a 16-byte multiple, so the writer pads nothing behind it and
    the payload ends exactly where the table says (a shard that ends in
    pad bytes can lose them without breaking any rule)."""
    data = corpus.shard_corpus(B, "none") + random.Random(20).randbytes(2048)
    packed = shardfmt.pack(data, block_raw=B)
    idx = shardfmt.read_index(packed)
    assert [b.stored for b in idx.blocks][:4] == [False, True, False, True]
    assert idx.n_blocks == 6 and idx.blocks[5].stored
    return data, packed


def _set(col, i, value):
    def mutate(s):
        s[3][col][i] = value
    return mutate


def _append_entry(s):
    extra = s[3][-1:].copy()
    s[3] = np.concatenate([s[3], extra])


def _drop_entry(s):
    s[3] = s[3][:-1].copy()


def _no_entries(s):
    s[3] = s[3][:0].copy()


def _raw_size_zero(s):
    s[2] = 0


def _inner_short(s):
    s[3]["raw_len"][1] = B - 16
    s[3]["comp_len"][1] = B - 16  # still stored, still <= raw_len


def _truncate(n):
    def mutate(s):
        s[4] = s[4][:-n]
    return mutate


# (id, mutation of [flags, block_raw, raw_size, table, payload], rule)
BAD_TABLES = [
    ("block_raw_0", lambda s: s.__setitem__(1, 0),
     "block_raw must be positive"),
    ("n_blocks_one_more", _append_entry, "n_blocks"),
    ("n_blocks_one_less", _drop_entry, "n_blocks"),
    ("no_blocks_but_raw_size", _no_entries, "n_blocks"),
    ("blocks_but_raw_size_0", _raw_size_zero, "n_blocks"),
    ("inner_raw_len_short", _inner_short, "inner block raw_len"),
    ("final_raw_len_0", _set("raw_len", -1, 0), "final raw_len"),
    ("final_raw_len_over", _set("raw_len", -1, B + 1), "final raw_len"),
    ("sum_raw_len", lambda s: (_set("raw_len", -1, 2032)(s),
                               _set("comp_len", -1, 2032)(s)),
     r"sum\(raw_len\)"),
    ("comp_len_0", _set("comp_len", 0, 0), "comp_len outside"),
    ("comp_len_over_raw_len", _set("comp_len", 0, B + 1),
     "comp_len outside"),
    ("comp_off_misaligned", _set("comp_off", 2, 8), "16-byte aligned"),
    ("comp_off_past_payload", _set("comp_off", 5, 1 << 20),
     "beyond the payload"),
    ("comp_off_bit40", lambda s: _set(
        "comp_off", 3, int(s[3]["comp_off"][3]) | (1 << 40))(s),
     "beyond the payload"),
    ("comp_off_bit63", lambda s: _set(
        "comp_off", 3, int(s[3]["comp_off"][3]) | (1 << 63))(s),
     "beyond the payload"),
    ("comp_off_wraps_u64", _set("comp_off", 1, U64 - 15),
     "beyond the payload"),
    ("payload_minus_1", _truncate(1), "beyond the payload"),
    ("payload_minus_block", _truncate(B), "beyond the payload"),
]


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "noverify"])
@pytest.mark.parametrize("name,mutate,rule", BAD_TABLES,
                         ids=[c[0] for c in BAD_TABLES])
def test_bad_table_raises_before_launch(good, name, mutate, rule, verify):
    _, packed = good
    parts = list(_split(packed))
    mutate(parts)
    bad = _join(*parts)
    fake = CpuOps()
    with pytest.raises(ValueError, match=rule):
        decode(bad, fake, verify=verify)
    assert fake.launches == 0
    # the same table fails the bare validator the same way
    idx = shardfmt.read_index(bad)
    with pytest.raises(ValueError, match=rule):
        shardfmt.validate_index(idx, len(bad) - idx.payload_off)


def test_good_shard_is_the_baseline(good):
    """The unmutated shard passes, so each case above fails for its own
    mutation only; its final block ends exactly at the payload's end
    (which is what makes a 1-byte truncation detectable)."""
    data, packed = good
    idx = shardfmt.read_index(packed)
    payload_len = len(packed) - idx.payload_off
    shardfmt.validate_index(idx, payload_len)
    last = idx.blocks[-1]
    assert last.comp_off + last.comp_len == payload_len
    fake = CpuOps()
    assert decode(packed, fake) == data
    assert fake.launches == 3  # gather + lz4 + crc


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "noverify"])
def test_block_raw_1000_rejected_on_gpu_reader_only(verify):
    data = corpus.text_like(random.Random(21), 5500)
    packed = shardfmt.pack(data, block_raw=1000)
    assert shardfmt.unpack_cpu(packed) == data  # CPU reader: permissive
    idx = shardfmt.read_index(packed)
    shardfmt.validate_index(idx, len(packed) - idx.payload_off,
                            for_gpu=False)
    fake = CpuOps()
    with pytest.raises(ValueError, match="multiple of 4096"):
        decode(packed, fake, verify=verify)
    assert fake.launches == 0


def test_block_raw_128k_with_compressed_blocks_rejected():
    rng = random.Random(22)
    big = 131072
    data = corpus.text_like(rng, big) + rng.randbytes(big) + b"tail" * 100
    packed = shardfmt.pack(data, block_raw=big)
    idx = shardfmt.read_index(packed)
    assert [b.stored for b in idx.blocks] == [False, True, False]
    shardfmt.validate_index(idx, len(packed) - idx.payload_off,
                            for_gpu=False)
    fake = CpuOps()
    with pytest.raises(ValueError, match="65536"):
        decode(packed, fake)
    assert fake.launches == 0


@pytest.mark.parametrize("n", [0, 7, 8, shardfmt.HEADER.size - 1])
def test_buffer_shorter_than_header(good, n):
    _, packed = good
    fake = CpuOps()
    with pytest.raises(ValueError, match="header"):
        decode(packed[:n], fake)
    assert fake.launches == 0
    with pytest.raises(ValueError):
        shardfmt.unpack_cpu(packed[:n])


def test_buffer_truncated_inside_table(good):
    _, packed = good
    cut = shardfmt.HEADER.size + 3 * shardfmt.ENTRY.size + 5
    fake = CpuOps()
    with pytest.raises(ValueError, match="block table"):
        decode(packed[:cut], fake)
    assert fake.launches == 0


# ------------------------------------------------- _stored_contiguous path
class TestStoredContiguousShortcut:
    @pytest.fixture(scope="class")
    def stored(self):
        data = corpus.shard_corpus(B, "none")  # no pad behind the end
        packed = shardfmt.pack(data, block_raw=B, compress=False)
        assert shardfmt._stored_contiguous(shardfmt.read_index(packed))
        return data, packed

    def test_view_without_verify_launches_nothing(self, stored):
        data, packed = stored
        fake = CpuOps()
        assert decode(packed, fake, verify=False) == data
        assert fake.launches == 0

    def test_verify_is_one_crc_launch(self, stored):
        data, packed = stored
        fake = CpuOps()
        assert decode(packed, fake, verify=True) == data
        assert fake.calls == [("crc", len(data))]

    @pytest.mark.parametrize("verify", [True, False],
                             ids=["verify", "noverify"])
    @pytest.mark.parametrize("cut", [1, B, B + 7])
    def test_truncated_payload_is_an_error_not_a_short_tensor(
            self, stored, cut, verify):
        _, packed = stored
        fake = CpuOps()
        with pytest.raises(ValueError, match="beyond the payload"):
            decode(packed[:-cut], fake, verify=verify)
        assert fake.launches == 0

    def test_payload_gone_entirely(self, stored):
        _, packed = stored
        idx = shardfmt.read_index(packed)
        fake = CpuOps()
        with pytest.raises(ValueError, match="beyond the payload"):
            decode(packed[:idx.payload_off], fake, verify=False)
        assert fake.launches == 0

    @pytest.mark.parametrize("verify", [True, False],
                             ids=["verify", "noverify"])
    def test_unpack_gpu_entry_point_payload_gone(self, stored, good,
                                                 verify):
        """unpack_gpu (the replicator's entry point) on a shard cut
        exactly at the end of its block table: ValueError, not an empty
        tensor; it fails before any device is touched."""
        cpu = torch.device("cpu")
        for _, packed in (stored, good):
            idx = shardfmt.read_index(packed)
            assert idx.n_blocks > 0
            with mock.patch("shipyard_amd.ops._load",
                            side_effect=AssertionError("library loaded")):
                with pytest.raises(ValueError, match="beyond the payload"):
                    shardfmt.unpack_gpu(packed[:idx.payload_off],
                                        device=cpu, verify=verify)

    def test_unpack_gpu_entry_point_empty_shard(self):
        got = shardfmt.unpack_gpu(shardfmt.pack(b""),
                                  device=torch.device("cpu"))
        assert got.numel() == 0 and got.dtype == torch.uint8

    def test_stored_only_262144_blocks_pass(self):
        big = 262144
        data = random.Random(23).randbytes(2 * big + 1234)
        packed = shardfmt.pack(data, block_raw=big, compress=False)
        idx = shardfmt.read_index(packed)
        shardfmt.validate_index(idx, len(packed) - idx.payload_off)
        fake = CpuOps()
        assert decode(packed, fake, verify=True) == data
        assert fake.calls == [("crc", len(data))]

    def test_losing_only_pad_bytes_is_not_an_error(self):
        data = corpus.shard_corpus(B, "random_bm1")  # 1 pad byte
        packed = shardfmt.pack(data, block_raw=B, compress=False)
        fake = CpuOps()
        assert decode(packed[:-1], fake, verify=True) == data
        with pytest.raises(ValueError, match="beyond the payload"):
            decode(packed[:-2], fake, verify=True)

    def test_reversed_stored_blocks_take_gather(self):
        """Stored-only but not contiguous: the blocks sit in the payload
        in reverse order (the layout test_shard_edges_gpu.py builds)."""
        data = corpus.shard_corpus(B, "random_bm1")
        packed = corpus.reversed_stored_shard(data, B)
        idx = shardfmt.read_index(packed)
        assert not shardfmt._stored_contiguous(idx)
        shardfmt.validate_index(idx, len(packed) - idx.payload_off)
        assert shardfmt.unpack_cpu(packed) == data
        for verify in (True, False):
            fake = CpuOps()
            assert decode(packed, fake, verify=verify) == data
            assert fake.calls[0] == ("gather", idx.n_blocks)
            assert fake.launches == (2 if verify else 1)


# ------------------------------------------------------------ good tables
@pytest.mark.parametrize("block_raw", corpus.SHARD_BLOCK_SIZES)
@pytest.mark.parametrize("final", list(corpus.SHARD_FINALS))
def test_corpus_shards_validate_and_roundtrip(block_raw, final):
    data = corpus.shard_corpus(block_raw, final)
    packed = shardfmt.pack(data, block_raw=block_raw)
    idx = shardfmt.read_index(packed)
    shardfmt.validate_index(idx, len(packed) - idx.payload_off)
    fake = CpuOps()
    assert decode(packed, fake) == data
    kinds = dict(fake.calls)
    stored = int((idx.table["comp_len"] == idx.table["raw_len"]).sum())
    assert kinds["gather"] == stored
    assert kinds["lz4"] == idx.n_blocks - stored
    if block_raw == B:
        assert decode(packed, CpuOps(), verify=False) == data


def test_empty_shard_validates():
    packed = shardfmt.pack(b"")
    idx = shardfmt.read_index(packed)
    shardfmt.validate_index(idx, 0)
    fake = CpuOps()
    assert decode(packed, fake) == b""
    assert fake.launches == 0


def test_validate_keeps_the_index_parse_budget():
    """The 131k-block table of test_index_parse_scales, validated inside
    the same 0.25 s budget (vectorized numpy, no per-block python)."""
    n = 131072
    table = np.zeros(n, dtype=shardfmt._entry_dt())
    table["comp_len"] = 4096
    table["raw_len"] = 4096
    table["comp_off"] = np.arange(n, dtype=np.uint64) * 4096
    buf = shardfmt.HEADER.pack(shardfmt.MAGIC, 1, 4096, n * 4096, n) + \
        table.tobytes()
    t0 = time.perf_counter()
    idx = shardfmt.read_index(buf)
    shardfmt.validate_index(idx, n * 4096)
    assert (time.perf_counter() - t0) < 0.25
    with pytest.raises(ValueError, match="beyond the payload"):
        shardfmt.validate_index(idx, n * 4096 - 1)


# ------------------------------------------------------------ corpus pins
def _block_states(comps, blocks):
    """True per block when the writer stores it."""
    return [c is None or len(c) >= len(b) for c, b in zip(comps, blocks)]


def _check_pins(block_raw, final, stored):
    data = corpus.shard_corpus(block_raw, final)
    want_last = corpus.SHARD_FINALS[final]
    n_full = corpus.SHARD_FULL_BLOCKS
    assert len(stored) == n_full + (want_last is not None)
    assert stored[1] and stored[3], stored        # random: stored
    assert not stored[0] and not stored[2], stored  # text, byte run
    if want_last is not None:
        assert stored[-1] is want_last, (final, stored)


@pytest.mark.parametrize("block_raw", corpus.SHARD_BLOCK_SIZES)
@pytest.mark.parametrize("final", list(corpus.SHARD_FINALS))
class TestShardCorpusPins:
    def test_geometry(self, block_raw, final):
        data = corpus.shard_corpus(block_raw, final)
        assert data == corpus.shard_corpus(block_raw, final)  # seeded
        last_len = {"equal_5": 5, "zeros_25": 25,
                    "random_bm1": block_raw - 1, "text_4k": 4001,
                    "none": 0}[final]
        assert len(data) == corpus.SHARD_FULL_BLOCKS * block_raw + last_len
        assert len(data) <= 6 * 65536
        blocks = corpus.shard_blocks(data, block_raw)
        assert len(set(blocks[2])) == 1          # the one-byte run
        assert blocks[1] != blocks[3]
        if final == "equal_5":
            assert len(set(blocks[-1])) == 1 and len(blocks[-1]) < 16
        if final == "zeros_25":
            assert blocks[-1] == b"\0" * 25
        if final == "none":
            assert len(data) % block_raw == 0
        else:
            assert len(data) % block_raw == last_len < block_raw
        # the full blocks do not depend on the final variant
        assert data[:5 * block_raw] == \
            corpus.shard_corpus(block_raw, "none")

    def test_states_under_lz4py(self, block_raw, final):
        blocks = corpus.shard_blocks(corpus.shard_corpus(block_raw, final),
                                     block_raw)
        comps = [lz4py.compress_block(b) for b in blocks]
        _check_pins(block_raw, final, _block_states(comps, blocks))

    def test_states_in_the_table_pack_writes(self, block_raw, final):
        """Same pins for the table pack() writes, whichever compressor
        it used; where the ops library is built that is the native one,
        which is then also checked directly."""
        from shipyard_amd import ops

        data = corpus.shard_corpus(block_raw, final)
        idx = shardfmt.read_index(shardfmt.pack(data, block_raw=block_raw))
        _check_pins(block_raw, final, [b.stored for b in idx.blocks])
        if ops.native_compress_available():
            blocks = corpus.shard_blocks(data, block_raw)
            comps = ops.lz4_compress_blocks(data, block_raw)
            _check_pins(block_raw, final, _block_states(comps, blocks))


# -------------------------------------------------- writer-side block_raw
class TestWriterBlockRaw:
    @pytest.mark.parametrize("block_raw", [0, 1000, 4095, 4097, 12000,
                                           65536 + 4096, 131072])
    def test_pack_gpu_rejects_up_front(self, block_raw):
        """ValueError before torch or the ops library is touched."""
        with mock.patch("shipyard_amd.ops._load",
                        side_effect=AssertionError("library loaded")):
            with pytest.raises(ValueError, match="block_raw"):
                shardfmt.pack_gpu(b"x" * 10000, block_raw=block_raw)
            with pytest.raises(ValueError, match="block_raw"):
                shardfmt.pack_gpu(b"", block_raw=block_raw)

    @pytest.mark.parametrize("block_raw", [1000, 131072])
    def test_pack_auto_routes_to_cpu_writer(self, block_raw):
        data = corpus.text_like(random.Random(24), 300_000)
        with mock.patch("torch.cuda.is_available", return_value=True), \
             mock.patch.object(shardfmt, "pack_gpu",
                               side_effect=AssertionError("GPU writer")):
            blob = shardfmt.pack_auto(data, block_raw=block_raw,
                                      gpu_threshold=1 << 10)
        assert blob == shardfmt.pack(data, block_raw=block_raw)
        assert shardfmt.unpack_cpu(blob) == data

    def test_pack_auto_still_uses_gpu_writer_for_good_sizes(self):
        data = b"y" * 5000
        with mock.patch("torch.cuda.is_available", return_value=True), \
             mock.patch.object(shardfmt, "pack_gpu",
                               return_value=b"gpu") as pg:
            assert shardfmt.pack_auto(data, block_raw=8192,
                                      gpu_threshold=1 << 10) == b"gpu"
        assert pg.call_count == 1

    def test_unpack_cpu_stays_permissive(self):
        data = corpus.mixed_content(random.Random(25), 7777)
        for block_raw in (1000, 4097, 131072):
            assert shardfmt.unpack_cpu(
                shardfmt.pack(data, block_raw=block_raw)) == data


# ----------------------------------------------- wrapper alignment contract
class _CountingLib:
    """Stands in for the ctypes library: any entry point called through
    it is a launch."""

    def __init__(self):
        self.launches = 0

    def __getattr__(self, name):
        def entry(*args):
            self.launches += 1
            return 0
        return entry


class TestWrapperAlignment:
    """A contiguous uint8 view whose base is not 16-byte aligned raises
    ValueError before the library is even looked up.  Shown on CPU
    tensors: the alignment check comes ahead of the device check."""

    @pytest.fixture()
    def lib(self):
        lib = _CountingLib()
        with mock.patch("shipyard_amd.ops._load", return_value=lib):
            yield lib

    @pytest.fixture(scope="class")
    def view(self):
        buf = torch.zeros(65536 + 16, dtype=torch.uint8)
        assert buf.data_ptr() % 16 == 0
        v = buf[1:1 + 65536]
        assert v.is_contiguous() and v.data_ptr() % 16 == 1
        return v

    def test_crc32c_chunks(self, lib, view):
        from shipyard_amd import ops

        for chunk in (4096, 32768):
            with pytest.raises(ValueError, match="16-byte aligned"):
                ops.crc32c_chunks(view, chunk_size=chunk)
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.crc32c_file_digest(view, chunk_size=4096)
        assert lib.launches == 0

    def test_crc32c_chunks_coal_raw(self, lib, view):
        from shipyard_amd import ops

        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.crc32c_chunks_coal_raw(view, chunk_size=32768)
        assert lib.launches == 0

    def test_sha256_pages(self, lib, view):
        from shipyard_amd import ops

        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.sha256_pages(view, page_size=4096)
        assert lib.launches == 0

    def test_lz4_compress_blocks_gpu(self, lib, view):
        from shipyard_amd import ops

        for screen in (False, True):
            with pytest.raises(ValueError, match="16-byte aligned"):
                ops.lz4_compress_blocks_gpu(view, 4096, screen=screen)
        assert lib.launches == 0

    @pytest.mark.parametrize("block_raw", [0, -4096, 1, 15, 17, 1000,
                                           4095, 4104, 65535])
    def test_lz4_compress_blocks_gpu_block_raw(self, lib, block_raw):
        """Blocks are staged with uint4 loads from blk * block_raw: a
        block_raw that is not a positive multiple of 16 (0 would also
        divide by zero) is a ValueError before any launch, ahead of
        the device assert."""
        from shipyard_amd import ops

        data = torch.zeros(65536, dtype=torch.uint8)
        assert data.data_ptr() % 16 == 0
        for screen in (False, True):
            with pytest.raises(ValueError, match="multiple of 16"):
                ops.lz4_compress_blocks_gpu(data, block_raw, screen=screen)
        assert lib.launches == 0

    def test_lz4_decode_blocks_out_only(self, lib, view):
        from shipyard_amd import ops

        i64 = torch.zeros(1, dtype=torch.int64)
        u32 = torch.ones(1, dtype=torch.int32).view(torch.uint32)
        comp = torch.zeros(64, dtype=torch.uint8)
        for pc in (False, True):
            with pytest.raises(ValueError, match="out base pointer"):
                ops.lz4_decode_blocks(comp, i64, u32, view, i64, u32,
                                      raw_cap=4096, pc=pc)
        assert lib.launches == 0

    def test_lz4_decode_blocks_comp_on_uint4_staging_paths(
            self, lib, view, monkeypatch):
        """The producer/consumer and staged kernels load uint4 from
        comp + (in_off & ~15): there the comp base must be aligned."""
        from shipyard_amd import ops

        i64 = torch.zeros(1, dtype=torch.int64)
        u32 = torch.ones(1, dtype=torch.int32).view(torch.uint32)
        out = torch.zeros(4096, dtype=torch.uint8)
        monkeypatch.delenv("SY_LZ4_NOSTAGE", raising=False)
        monkeypatch.delenv("SY_LZ4_SKIP", raising=False)
        with pytest.raises(ValueError, match="comp base pointer"):
            ops.lz4_decode_blocks(view, i64, u32, out, i64, u32,
                                  raw_cap=4096, pc=True)
        monkeypatch.setenv("SHIPYARD_LZ4_PC", "1")
        with pytest.raises(ValueError, match="comp base pointer"):
            ops.lz4_decode_blocks(view, i64, u32, out, i64, u32,
                                  raw_cap=4096)
        monkeypatch.delenv("SHIPYARD_LZ4_PC")
        for name, value in (("SY_LZ4_NOSTAGE", "0"), ("SY_LZ4_SKIP", "1"),
                            ("SY_LZ4_SKIP", "2"), ("SY_LZ4_NOSTAGE", "x")):
            monkeypatch.setenv(name, value)
            with pytest.raises(ValueError, match="comp base pointer"):
                ops.lz4_decode_blocks(view, i64, u32, out, i64, u32,
                                      raw_cap=4096, pc=False)
            monkeypatch.delenv(name)
        assert lib.launches == 0
        assert not ops._lz4_staged_by_env()  # default path: bytewise

    def test_manifest_and_writer_inherit_the_contract(self, lib, view):
        from shipyard_amd.data import integrity

        with pytest.raises(ValueError, match="16-byte aligned"):
            integrity.compute_gpu(view, chunk_size=4096)
        with pytest.raises(ValueError, match="16-byte aligned"):
            shardfmt.pack_gpu(view, block_raw=4096)
        assert lib.launches == 0
