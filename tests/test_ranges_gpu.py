"""GPU tests of random-access range reads: the ops.gather_ranges kernel
against numpy slicing (every source x destination misalignment, the
bounds rule for loads, the work split), shardfmt.decode_ranges_device
against read_ranges_cpu and the original bytes on every filter
combination, and ShardStager.stage_ranges on files.  Every comparison
is exact."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from shipyard_amd import ops  # noqa: E402
from shipyard_amd.data import shardfmt  # noqa: E402
from shipyard_amd.data.stager import ShardStager  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 128  # dst sits at this (16 B aligned) offset inside its canary buffer
DEV = "cuda:0"


def _cuda(raw):
    arr = np.frombuffer(raw, dtype=np.uint8) if isinstance(
        raw, (bytes, bytearray)) else raw
    if not len(arr):
        return torch.empty(0, dtype=torch.uint8, device=DEV)
    return torch.from_numpy(np.array(arr, dtype=np.uint8)).to(DEV)


def _i64(v):
    return torch.tensor(np.asarray(v, dtype=np.int64), dtype=torch.int64,
                        device=DEV)


def _host(t) -> bytes:
    return bytes(t.cpu().numpy().tobytes())


def _rand(n: int, seed: int):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _gather_in_canary(d_src, src_np, soff, lens, doff, dst_len, shift=0):
    """Run the kernel into a view at PAD + shift inside a canary-filled
    buffer and compare the WHOLE buffer with numpy slicing: the ranges,
    the gaps between them and both margins."""
    big = torch.full((dst_len + 2 * PAD + shift,), CANARY, dtype=torch.uint8,
                     device=DEV)
    dst = big[PAD + shift:PAD + shift + dst_len]
    assert dst.data_ptr() % 16 == shift % 16
    ops.gather_ranges(d_src, _i64(soff), _i64(lens), dst, _i64(doff))
    torch.cuda.current_stream().synchronize()
    want = np.full(big.numel(), CANARY, dtype=np.uint8)
    for s, n, d in zip(soff, lens, doff):
        want[PAD + shift + d:PAD + shift + d + n] = src_np[s:s + n]
    got = big.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), bad[:8].tolist())


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 31, 33, 255, 4097])
def test_every_misalignment_pair(length):
    """256 ranges in one launch: range 16*a + b reads at a source
    address that is a mod 16 and writes at one that is b mod 16."""
    stride = (length + 15) // 16 * 16 + 48
    a, b = np.divmod(np.arange(256), 16)
    soff = np.arange(256) * stride + a
    doff = np.arange(256) * stride + b
    lens = np.full(256, length)
    src_np = _rand(256 * stride, seed=length)
    d_src = _cuda(src_np)
    assert d_src.data_ptr() % 16 == 0
    _gather_in_canary(d_src, src_np, soff, lens, doff, 256 * stride)
    assert _host(d_src) == src_np.tobytes()  # the source is read-only


@pytest.mark.parametrize("shift", [0, 5])
def test_misaligned_base_pointers(shift):
    """The alignment that counts is that of the address: src and dst
    views at odd storage offsets."""
    src_np = _rand(3 * 4096 + 11, seed=3)
    big_src = torch.full((len(src_np) + 64,), 0x3C, dtype=torch.uint8,
                         device=DEV)
    d_src = big_src[7:7 + len(src_np)]
    d_src.copy_(_cuda(src_np))
    soff = [0, 100, 5000, 4097]
    lens = [33, 4097, 7000, 1]
    doff = [0, 40, 4200, 11300]
    _gather_in_canary(d_src, src_np, soff, lens, doff, 11400, shift=shift)


@pytest.mark.parametrize("ns", [1000, 4099, 37])
def test_ranges_at_both_ends_of_the_source(ns):
    """The bounds rule for loads: a range that begins at byte 0 of src
    and one that ends at its last byte, src being a view at an odd
    storage offset inside a larger tensor and numel() no multiple of
    16, at every destination misalignment."""
    assert ns % 16
    src_np = _rand(ns, seed=ns)
    big_src = torch.full((ns + 96,), 0x3C, dtype=torch.uint8, device=DEV)
    d_src = big_src[35:35 + ns]
    assert d_src.data_ptr() % 16 == 3
    d_src.copy_(_cuda(src_np))
    soff, lens, doff = [], [], []
    head = min(ns, 300)
    for k in range(16):
        soff += [0, ns - head, 0]
        lens += [head, head, ns]
        base = k * (2 * 320 + ns + 64) + k
        doff += [base, base + 320, base + 640]
    _gather_in_canary(d_src, src_np, soff, lens, doff,
                      doff[-1] + ns + 16)
    assert (big_src[:35] == 0x3C).all().item()
    assert (big_src[35 + ns:] == 0x3C).all().item()


def test_one_large_range_among_many_small():
    """The work split: 1 MiB + 7 bytes at source +3 / destination +5
    (257 pieces, spread over the waves) in one launch with 1000 ranges
    of 1..64 bytes on either side of it."""
    rng = np.random.default_rng(9)
    big_len = (1 << 20) + 7
    small = rng.integers(1, 65, 1000)
    lens = np.concatenate((small[:500], [big_len], small[500:]))
    n_src = big_len + 70000
    src_np = _rand(n_src, seed=10)
    soff = rng.integers(0, n_src - 64, len(lens))
    soff[500] = 16 * 1000 + 3
    gaps = rng.integers(0, 9, len(lens))
    doff = np.concatenate(([0], np.cumsum(lens[:-1] + gaps[:-1])))
    doff[500:] += (5 - doff[500]) % 16  # the large range lands at 5 mod 16
    assert doff[500] % 16 == 5 and soff[500] % 16 == 3
    assert (doff[1:] >= doff[:-1] + lens[:-1]).all()
    _gather_in_canary(_cuda(src_np), src_np, soff, lens, doff,
                      int(doff[-1] + lens[-1]) + 8)


def test_repeated_and_overlapping_sources():
    src_np = _rand(20000, seed=4)
    soff = [100, 100, 100, 150, 0, 9000, 9001, 100]
    lens = [5000, 5000, 17, 9000, 20000, 4096, 4096, 0]
    doff = np.concatenate(([0], np.cumsum(np.asarray(lens[:-1]) + 3)))
    _gather_in_canary(_cuda(src_np), src_np, soff, lens, doff,
                      int(doff[-1] + lens[-1]) + 5)


def test_empty_ranges_between_pieces():
    """Runs of empty ranges: the wave that walks from one range to the
    next has to step over them."""
    src_np = _rand(30000, seed=5)
    lens = np.zeros(600, dtype=np.int64)
    lens[[0, 299, 300, 599]] = [9000, 1, 12000, 4096]
    soff = np.zeros(600, dtype=np.int64)
    soff[[0, 299, 300, 599]] = [1, 29999, 16, 7]
    doff = np.concatenate(([0], np.cumsum(lens[:-1])))
    _gather_in_canary(_cuda(src_np), src_np, soff, lens, doff,
                      int(lens.sum()))
    # nothing but empty ranges
    _gather_in_canary(_cuda(src_np), src_np, [0, 5, 30000], [0, 0, 0],
                      [0, 0, 64], 64)


def test_no_ranges_is_a_no_op_without_the_library(monkeypatch):
    def boom():
        raise AssertionError("library loaded for an empty gather")

    monkeypatch.setattr(ops, "_load", boom)
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    dst = torch.full((64,), CANARY, dtype=torch.uint8, device=DEV)
    e = torch.empty(0, dtype=torch.int64, device=DEV)
    ops.gather_ranges(src, e, e, dst, e)
    assert (dst == CANARY).all().item()


def test_argument_errors_come_before_any_launch(monkeypatch):
    def boom():
        raise AssertionError("library loaded despite bad arguments")

    monkeypatch.setattr(ops, "_load", boom)
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(64, dtype=torch.uint8, device=DEV)
    ok = _i64([0, 8])
    with pytest.raises(ValueError, match="int64"):
        ops.gather_ranges(src, ok.to(torch.int32), ok, dst, ok)
    with pytest.raises(ValueError, match="int64"):
        ops.gather_ranges(src, ok, ok.to(torch.uint8), dst, ok)
    with pytest.raises(ValueError, match="int64"):
        ops.gather_ranges(src, ok, ok, dst, ok.to(torch.float32))
    with pytest.raises(ValueError, match="lengths"):
        ops.gather_ranges(src, ok, _i64([1]), dst, ok)
    with pytest.raises(ValueError, match="lengths"):
        ops.gather_ranges(src, ok, ok, dst, _i64([0, 8, 16]))
    with pytest.raises(ValueError, match="is on"):
        ops.gather_ranges(src, ok.cpu(), ok, dst, ok)


# ---------------------------------------------------------- shard level
# (delta_elem, bitshuffle_elem, shuffle_elem): everything the writers take
FILTERS = [(0, 0, 0)] + \
    [(0, 0, e) for e in (2, 4, 8)] + \
    [(e, 0, 0) for e in (2, 4, 8)] + \
    [(0, e, 0) for e in (2, 4, 8)] + \
    [(8, 0, 8), (4, 0, 2), (2, 0, 4)] + \
    [(8, 8, 0), (4, 2, 0), (2, 4, 0)]


def _ids(f):
    return "d%d-b%d-s%d" % f


@functools.lru_cache(maxsize=None)
def _raw(block_raw: int) -> bytes:
    """5 blocks, the last one 1000 bytes: two blocks of random bytes
    (stored under every filter) and then slowly rising int32 values
    (LZ4 blocks)."""
    rng = np.random.default_rng(block_raw)
    n = 4 * block_raw + 1000
    noise = rng.integers(0, 256, 2 * block_raw, dtype=np.uint8).tobytes()
    vals = np.cumsum(rng.integers(0, 5, n // 4)).astype("<u4").tobytes()
    return (noise + vals)[:n]


@functools.lru_cache(maxsize=None)
def _packed(block_raw: int, filt, compress: bool) -> bytes:
    D, B, S = filt
    return shardfmt.pack(_raw(block_raw), block_raw=block_raw,
                         compress=compress, delta_elem=D, bitshuffle_elem=B,
                         shuffle_elem=S)


def _ranges(block_raw: int):
    """Edges of blocks and of the shard, empty ranges, a repeat, a range
    over three blocks, unsorted; blocks 0..4 are all touched."""
    n = 4 * block_raw + 1000
    offs = [n - 1, 0, block_raw - 3, 777, 4 * block_raw - 7, n,
            2 * block_raw, 777, block_raw + 1]
    lens = [1, 1, 6, 0, 1007, 0, block_raw, 2 * block_raw + 5, 33]
    return offs, lens


def _want(raw, offs, lens):
    return b"".join(raw[o:o + n] for o, n in zip(offs, lens))


def _on_device(packed: bytes):
    idx = shardfmt.read_index(packed)
    return _cuda(packed[idx.payload_off:]), idx


@pytest.mark.parametrize("compress", [True, False], ids=["lz4", "stored"])
@pytest.mark.parametrize("filt", FILTERS, ids=_ids)
def test_decode_ranges_device_matrix(filt, compress):
    for block_raw in (4096, 8192):
        raw = _raw(block_raw)
        packed = _packed(block_raw, filt, compress)
        d_comp, idx = _on_device(packed)
        if compress and filt == (0, 0, 0):
            stored = idx.table["comp_len"] == idx.table["raw_len"]
            assert stored[:2].all() and not stored[2:].any()  # mixed
        offs, lens = _ranges(block_raw)
        want = _want(raw, offs, lens)
        assert shardfmt.read_ranges_cpu(packed, offs, lens) == want
        got = shardfmt.decode_ranges_device(d_comp, idx, offs, lens, DEV)
        assert got.dtype == torch.uint8 and got.dim() == 1
        assert _host(got) == want, (block_raw, "packed")
        # a subset that leaves blocks out: stored 1 and LZ4 3 selected
        offs2 = [3 * block_raw + 9, block_raw + 5]
        lens2 = [block_raw - 9, 100]
        assert idx.select_blocks(offs2, lens2).tolist() == [1, 3]
        got = shardfmt.decode_ranges_device(d_comp, idx, offs2, lens2, DEV,
                                            verify=False)
        assert _host(got) == _want(raw, offs2, lens2), (block_raw, "subset")
        # rows
        stride = 2 * block_raw + 8
        rows = shardfmt.decode_ranges_device(d_comp, idx, offs, lens, DEV,
                                             row_stride=stride, fill=0xEE)
        assert tuple(rows.shape) == (len(offs), stride)
        host = rows.cpu().numpy()
        for i, (o, n) in enumerate(zip(offs, lens)):
            assert host[i, :n].tobytes() == raw[o:o + n], (block_raw, i)
            assert (host[i, n:] == 0xEE).all(), (block_raw, i)
        assert 0 in lens  # a zero-length row is all fill
        # the payload is never written
        assert _host(d_comp) == packed[idx.payload_off:]


def test_decode_ranges_device_reads_gpu_authored_shard():
    block_raw = 8192
    raw = _raw(block_raw)
    packed = shardfmt.pack_gpu(raw, block_raw=block_raw, delta_elem=4,
                               shuffle_elem=4)
    d_comp, idx = _on_device(packed)
    assert (idx.delta_elem, idx.shuffle_elem) == (4, 4)
    offs, lens = _ranges(block_raw)
    got = shardfmt.decode_ranges_device(d_comp, idx, offs, lens, DEV)
    assert _host(got) == _want(raw, offs, lens)
    assert _host(got) == shardfmt.read_ranges_cpu(packed, offs, lens)


def _no_launch(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a kernel was launched")

    for name in ("gather_copy", "lz4_decode_blocks", "crc32c_chunks",
                 "gather_ranges", "byte_shuffle", "delta_filter",
                 "bit_shuffle"):
        monkeypatch.setattr(ops, name, boom)


def test_bad_requests_raise_before_any_launch(monkeypatch):
    block_raw = 4096
    packed = _packed(block_raw, (0, 0, 4), True)
    d_comp, idx = _on_device(packed)
    n = idx.raw_size
    _no_launch(monkeypatch)
    with pytest.raises(ValueError, match="row_stride"):
        shardfmt.decode_ranges_device(d_comp, idx, [0, 10], [8, 9], DEV,
                                      row_stride=8)
    for offs, lens in (([n - 3], [4]), ([-1], [1]), ([0], [-2])):
        with pytest.raises(ValueError, match="ranges"):
            shardfmt.decode_ranges_device(d_comp, idx, offs, lens, DEV)
    # a corrupt index alongside an out-of-range request: the index is
    # looked at first, so its error is the one that comes out
    table = idx.table.copy()
    table["comp_off"][1] += 8
    bad = shardfmt.ShardIndex(idx.block_raw, idx.raw_size, 0, table=table,
                              shuffle_elem=4)
    with pytest.raises(ValueError, match="comp_off not 16-byte aligned"):
        shardfmt.decode_ranges_device(d_comp, bad, [n - 3], [4], DEV)
    # no ranges: an empty tensor and still no launch
    got = shardfmt.decode_ranges_device(d_comp, idx, [], [], DEV)
    assert got.numel() == 0 and got.dim() == 1 and got.is_cuda
    got = shardfmt.decode_ranges_device(d_comp, idx, [], [], DEV,
                                        row_stride=32)
    assert tuple(got.shape) == (0, 32)


@pytest.mark.parametrize("filt", [(0, 0, 0), (4, 0, 4)], ids=_ids)
def test_corruption_is_seen_only_in_selected_blocks(filt):
    block_raw = 4096
    raw = _raw(block_raw)
    packed = _packed(block_raw, filt, False)
    idx = shardfmt.read_index(packed)
    offs, lens = [block_raw + 5, 4 * block_raw - 2], [100, 4]
    assert idx.select_blocks(offs, lens).tolist() == [1, 3, 4]

    def flipped(block):
        buf = bytearray(packed)
        buf[idx.payload_off + int(idx.table["comp_off"][block]) + 8] ^= 0x55
        return _cuda(bytes(buf)[idx.payload_off:])

    # the shard's block id, not the scratch slot (3 sits in slot 1)
    with pytest.raises(ValueError, match=r"CRC mismatch in blocks \[3\]"):
        shardfmt.decode_ranges_device(flipped(3), idx, offs, lens, DEV)
    with pytest.raises(ValueError, match=r"CRC mismatch in blocks \[4\]"):
        shardfmt.decode_ranges_device(flipped(4), idx, offs, lens, DEV)
    for block in (0, 2):
        d_bad = flipped(block)
        got = shardfmt.decode_ranges_device(d_bad, idx, offs, lens, DEV)
        assert _host(got) == _want(raw, offs, lens)
        with pytest.raises(ValueError, match="CRC mismatch"):
            shardfmt.decode_device(d_bad, idx, DEV)


# --------------------------------------------------------------- stager
@functools.lru_cache(maxsize=None)
def _file_raw() -> bytes:
    """16 blocks of 8 KiB: random bytes (stored) in the even blocks and
    rising int32 values (LZ4) in the odd ones."""
    rng = np.random.default_rng(31)
    out = []
    for b in range(16):
        if b % 2:
            out.append(np.cumsum(rng.integers(0, 5, 2048)).astype(
                "<u4").tobytes())
        else:
            out.append(rng.integers(0, 256, 8192, dtype=np.uint8).tobytes())
    return b"".join(out)


@pytest.mark.parametrize("native", [True, False],
                         ids=["native-cxx", "python"])
def test_stage_ranges(tmp_path, native):
    raw = _file_raw()
    src = tmp_path / "raw.bin"
    src.write_bytes(raw)
    path = tmp_path / "tokens.syshard"
    idx = shardfmt.pack_file(src, path, block_raw=8192, shuffle_elem=4)
    assert idx.n_blocks == 16
    st = ShardStager(staging_mb=1, verify=True, native=native)
    head = shardfmt.HEADER.size + 16 * shardfmt.ENTRY.size

    # two blocks that are no neighbours: two runs, nothing in between
    offs, lens = [9 * 8192 + 100, 2 * 8192 + 7, 9 * 8192], [500, 8000, 0]
    out, res = st.stage_ranges(path, offs, lens)
    assert _host(out) == _want(raw, offs, lens)
    assert res.decoded and res.verified
    assert res.raw_bytes == sum(lens)
    assert res.file_bytes == head + int(idx.table["comp_len"][2]) + \
        int(idx.table["comp_len"][9])
    whole, res_all = st.stage_file(path)
    assert _host(whole) == raw
    assert res.file_bytes < res_all.file_bytes

    # a run of neighbours (3, 4, 5), a lone block and the last block
    offs = [3 * 8192 + 8000, 16 * 8192 - 10, 12 * 8192, 5 * 8192 - 1]
    lens = [8192 + 300, 10, 8192, 2]
    out, res = st.stage_ranges(path, offs, lens, row_stride=8500, fill=0xEE)
    host = out.cpu().numpy()
    assert host.shape == (4, 8500)
    for i, (o, n) in enumerate(zip(offs, lens)):
        assert host[i, :n].tobytes() == raw[o:o + n]
        assert (host[i, n:] == 0xEE).all()
    t = idx.table
    span = int(t["comp_off"][5] + t["comp_len"][5] - t["comp_off"][3])
    assert res.file_bytes == head + span + int(t["comp_len"][12]) + \
        int(t["comp_len"][15])
    assert res.raw_bytes == sum(lens)

    # everything, and nothing
    out, res = st.stage_ranges(path, [0], [len(raw)])
    assert _host(out) == raw
    assert res.file_bytes == head + int(t["comp_off"][15]) + \
        int(t["comp_len"][15]) <= res_all.file_bytes
    out, res = st.stage_ranges(path, [], [])
    assert out.numel() == 0 and res.raw_bytes == 0 and res.file_bytes == head

    with pytest.raises(ValueError, match="ranges"):
        st.stage_ranges(path, [len(raw) - 3], [4])
    with pytest.raises(ValueError, match="row_stride"):
        st.stage_ranges(path, [0], [9], row_stride=8)


@pytest.mark.parametrize("native", [True, False],
                         ids=["native-cxx", "python"])
def test_stage_ranges_rejects_bad_files(tmp_path, native):
    st = ShardStager(staging_mb=1, native=native)
    plain = tmp_path / "plain.bin"
    plain.write_bytes(_file_raw()[:5000])
    with pytest.raises(ValueError, match="not a SYSHARD"):
        st.stage_ranges(plain, [0], [10])
    packed = shardfmt.pack(_file_raw(), block_raw=8192)
    cut = tmp_path / "cut.syshard"
    cut.write_bytes(packed[:shardfmt.HEADER.size + 5 * shardfmt.ENTRY.size
                           + 3])
    with pytest.raises(ValueError, match="truncated inside the SYSHARD "
                                         "block table"):
        st.stage_ranges(cut, [0], [10])
    with pytest.raises(ValueError, match="truncated inside the SYSHARD "
                                         "block table"):
        st.stage_file(cut)
    cut.write_bytes(packed[:12])
    with pytest.raises(ValueError, match="truncated inside the SYSHARD "
                                         "header"):
        st.stage_ranges(cut, [0], [10])
