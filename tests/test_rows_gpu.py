"""GPU tests of typed row reads: the ops.gather_widen kernel against
numpy (every conversion, row lengths around the 16-byte slot, every
source alignment, destination views that are and are not 16-byte
aligned, the bounds rule for loads, both ends of the work split),
shardfmt.decode_rows_device against read_rows_cpu, direct slicing and
the composed byte path, and ShardStager.stage_rows on files.  Every
comparison is exact."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rows_cases as rc  # noqa: E402

from shipyard_amd import ops  # noqa: E402
from shipyard_amd.data import shardfmt  # noqa: E402
from shipyard_amd.data.stager import ShardStager  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 32  # elements of canary on either side of dst: 128 or 256 bytes
TORCH = {"int32": torch.int32, "int64": torch.int64}


def _canary(out: str) -> int:
    return 0x5A5A5A5A if out == "int32" else 0x5A5A5A5A5A5A5A5A


def _i64(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64)).to(DEV)


def _src_view(src_np):
    """src as a view at byte 4 of its allocation: bytes in front of it
    and behind it that are not the tensor's."""
    big = torch.full((len(src_np) + 8,), 0x3C, dtype=torch.uint8, device=DEV)
    view = big[4:4 + len(src_np)]
    view.copy_(torch.from_numpy(src_np).to(DEV))
    return big, view


def _expect(src_np, src: str, out: str, soff, counts, T, pad):
    """[n, T] numpy array: one fancy index, one where."""
    size = rc.SIZE[src]
    el = src_np[:len(src_np) // size * size].view(rc.NUMPY[src])
    first = np.asarray(soff, dtype=np.int64) // size
    cols = np.arange(T, dtype=np.int64)
    live = cols[None, :] < np.asarray(counts, dtype=np.int64)[:, None]
    at = np.where(live, first[:, None] + cols[None, :], 0)
    vals = el[at].astype(out) if len(el) else np.zeros(at.shape, dtype=out)
    return np.where(live, vals, np.asarray(pad, dtype=out))


def _widen_in_canary(d_src, src_np, src, out, soff, counts, T, pad, shift):
    """Run the kernel into a [n, T] view ``shift`` elements past a
    16-byte boundary inside a canary-filled buffer and compare the WHOLE
    buffer with numpy: rows, padding and both margins."""
    n = len(soff)
    big = torch.full((n * T + 2 * MARGIN + shift,), _canary(out),
                     dtype=TORCH[out], device=DEV)
    dst = big[MARGIN + shift:MARGIN + shift + n * T].view(n, T)
    assert dst.data_ptr() % 16 == shift * dst.element_size() % 16
    ops.gather_widen(d_src, _i64(soff), _i64(counts), dst, src, pad)
    torch.cuda.current_stream().synchronize()
    want = np.full(big.numel(), _canary(out), dtype=out)
    want[MARGIN + shift:MARGIN + shift + n * T] = _expect(
        src_np, src, out, soff, counts, T, pad).reshape(-1)
    got = big.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), bad[:8].tolist(),
                          got[bad[:8]].tolist(), want[bad[:8]].tolist())


def _kernel_rows(size: int, T: int, n_bytes: int, rng):
    """Counts {0, 1, 2, 3, 7, 8, 9, T-1, T} that fit T, each at every
    source address residue mod 16 that is a multiple of the element
    (the view starts at 4 mod 16, so offsets walk all of them); a row
    from byte 0, one up to the last byte, repeats; shuffled."""
    soff, counts = [], []
    for c in sorted({c for c in (0, 1, 2, 3, 7, 8, 9, T - 1, T)
                     if 0 <= c <= T}):
        for res in range(0, 16, size):
            room = (n_bytes - c * size - res) // 16
            soff.append(res + 16 * int(rng.integers(0, room + 1)))
            counts.append(c)
    soff += [0, n_bytes - T * size, 0, n_bytes - T * size, soff[0]]
    counts += [T, T, min(T, 2), T - 1, counts[0]]
    soff[-2] += size  # T - 1 elements that end at the last byte
    order = rng.permutation(len(soff))
    return (np.asarray(soff)[order].tolist(),
            np.asarray(counts)[order].tolist())


@pytest.mark.parametrize("shift", [0, 1], ids=["dst-aligned", "dst-plus-1"])
@pytest.mark.parametrize("T", [1, 3, 8, 9, 1025])
@pytest.mark.parametrize("pair", rc.PAIRS, ids=rc.pair_id)
def test_gather_widen_against_numpy(pair, T, shift):
    src, out = pair
    size = rc.SIZE[src]
    rng = np.random.default_rng(1000 * T + 10 * size + shift)
    n_bytes = (T + 24) * size // 16 * 16 + 52  # a multiple of 4, not of 16
    assert n_bytes % 4 == 0 and n_bytes % 16
    src_np = rng.integers(0, 256, n_bytes, dtype=np.uint8)
    src_np[:8] = 0xFF  # -1 / the largest unsigned value at the front
    big_src, d_src = _src_view(src_np)
    assert d_src.data_ptr() % 16 == 4
    soff, counts = _kernel_rows(size, T, n_bytes, rng)
    assert {(o + 4) % 16 for o in soff} >= set(range(0, 16, size))
    pad = {0: -100, 1: 50256}[shift] if out == "int32" else \
        {0: -2 ** 63, 1: 2 ** 63 - 1}[shift]
    _widen_in_canary(d_src, src_np, src, out, soff, counts, T, pad, shift)
    # the source is read-only, and so is what lies around it
    assert (big_src[4:4 + n_bytes].cpu().numpy() == src_np).all()
    assert (big_src[:4] == 0x3C).all().item()
    assert (big_src[4 + n_bytes:] == 0x3C).all().item()


@pytest.mark.parametrize("pair", [("u2", "int64"), ("i2", "int32"),
                                  ("u1", "int32")], ids=rc.pair_id)
def test_many_rows_small_T(pair):
    """70000 rows of 5 elements in one launch: a wave's 1 KiB holds
    dozens of rows, every lane finds its own."""
    src, out = pair
    size = rc.SIZE[src]
    n, T = 70000, 5
    rng = np.random.default_rng(5)
    src_np = rng.integers(0, 256, 40000 * size, dtype=np.uint8)
    counts = rng.integers(0, T + 1, n)
    soff = rng.integers(0, 40000 - T, n) * size
    d_src = torch.from_numpy(src_np).to(DEV)
    _widen_in_canary(d_src, src_np, src, out, soff, counts, T, -1, 1)


@pytest.mark.parametrize("pair", [("u2", "int64"), ("i4", "int32"),
                                  ("u1", "int64")], ids=rc.pair_id)
def test_few_rows_large_T(pair):
    """3 rows of 200000 elements: almost every wave step lies inside
    one row (data, padding, or the one step where the data ends)."""
    src, out = pair
    size = rc.SIZE[src]
    n, T = 3, 200000
    rng = np.random.default_rng(6)
    src_np = rng.integers(0, 256, (T + 1000) * size, dtype=np.uint8)
    counts = [T, 123457, 0]
    soff = [3 * size, 1000 * size, 0]
    d_src = torch.from_numpy(src_np).to(DEV)
    for shift in (0, 1):
        _widen_in_canary(d_src, src_np, src, out, soff, counts, T, 50256,
                         shift)


def test_no_rows_is_a_no_op_without_the_library(monkeypatch):
    def boom():
        raise AssertionError("library loaded for an empty gather")

    monkeypatch.setattr(ops, "_load", boom)
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    e = torch.empty(0, dtype=torch.int64, device=DEV)
    ops.gather_widen(src, e, e, torch.empty((0, 7), dtype=torch.int32,
                                            device=DEV), "u2", 0)
    dst = torch.full((2, 0), 9, dtype=torch.int64, device=DEV)
    ops.gather_widen(src, _i64([0, 0]), _i64([0, 0]), dst, "u2", 0)


def test_argument_errors_come_before_any_launch(monkeypatch):
    def boom():
        raise AssertionError("library loaded despite bad arguments")

    monkeypatch.setattr(ops, "_load", boom)
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    dst = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    ok = _i64([0, 8])
    with pytest.raises(ValueError, match="int64"):
        ops.gather_widen(src, ok.to(torch.int32), ok, dst, "u2", 0)
    with pytest.raises(ValueError, match="int64"):
        ops.gather_widen(src, ok, ok.to(torch.float32), dst, "u2", 0)
    with pytest.raises(ValueError, match="is on"):
        ops.gather_widen(src, ok.cpu(), ok, dst, "u2", 0)
    with pytest.raises(ValueError, match="is on"):
        ops.gather_widen(src, ok, ok.cpu(), dst, "u2", 0)
    with pytest.raises(ValueError, match="rows of dst"):
        ops.gather_widen(src, ok, _i64([1]), dst, "u2", 0)
    with pytest.raises(ValueError, match="rows of dst"):
        ops.gather_widen(src, _i64([0, 8, 16]), _i64([1, 1, 1]), dst, "u2",
                         0)
    with pytest.raises(ValueError, match="does not fit int32"):
        ops.gather_widen(src, ok, ok, dst, "u4", 0)
    with pytest.raises(ValueError, match="src_dtype"):
        ops.gather_widen(src, ok, ok, dst, "i1", 0)
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.gather_widen(src, ok, ok, dst.to(torch.int16), "u1", 0)
    for pad in (2 ** 31, -2 ** 31 - 1):
        with pytest.raises(ValueError, match="pad"):
            ops.gather_widen(src, ok, ok, dst, "u2", pad)
    for pad in (2 ** 63, -2 ** 63 - 1):
        with pytest.raises(ValueError, match="pad"):
            ops.gather_widen(src, ok, ok, dst.to(torch.int64), "u4", pad)
    with pytest.raises(ValueError, match="dst is on"):
        ops.gather_widen(src, ok, ok, dst.cpu(), "u2", 0)
    with pytest.raises(ValueError, match="not on a GPU"):
        ops.gather_widen(src.cpu(), ok.cpu(), ok.cpu(), dst.cpu(), "u2", 0)
    with pytest.raises(ValueError, match="contiguous uint8"):
        ops.gather_widen(src.to(torch.int8), ok, ok, dst, "u2", 0)
    with pytest.raises(ValueError, match="contiguous uint8"):
        ops.gather_widen(src[::2], ok, ok, dst, "u2", 0)
    with pytest.raises(ValueError, match="multiple of the 2-byte"):
        ops.gather_widen(src[1:], ok, ok, dst, "u2", 0)
    with pytest.raises(ValueError, match="multiple of the 4-byte"):
        ops.gather_widen(src[2:], ok, ok, dst, "i4", 0)


# ---------------------------------------------------------- shard level
def _on_device(packed: bytes):
    idx = shardfmt.read_index(packed)
    payload = np.frombuffer(packed, dtype=np.uint8)[idx.payload_off:]
    return torch.from_numpy(payload.copy()).to(DEV), idx


def _composed(d_comp, idx, starts, counts, src, out, row_elems, pad):
    """The path that existed before gather_widen: byte rows, a view, a
    widening cast, a masked pad."""
    size = rc.SIZE[src]
    rows = shardfmt.decode_ranges_device(
        d_comp, idx, np.asarray(starts) * size, np.asarray(counts) * size,
        DEV, row_stride=row_elems * size)
    host = rows.cpu().numpy().view(rc.NUMPY[src]).astype(out)
    live = np.arange(row_elems)[None, :] < np.asarray(counts)[:, None]
    return np.where(live, host, np.asarray(pad, dtype=out))


@pytest.mark.parametrize("pair", rc.PAIRS, ids=rc.pair_id)
def test_decode_rows_device_matrix(pair):
    src, out = pair
    size = rc.SIZE[src]
    starts, counts, row_elems = rc.rows(size)
    for filt, _ in rc.filters(size):
        packed = rc.packed(filt, size)
        d_comp, idx = _on_device(packed)
        for pad in rc.pads(out):
            got = shardfmt.decode_rows_device(
                d_comp, idx, starts, counts, DEV, src, TORCH[out], row_elems,
                pad)
            assert got.dtype == TORCH[out] and got.is_cuda
            assert tuple(got.shape) == (len(starts), row_elems)
            host = got.cpu().numpy()
            assert (host == rc.want(src, out, starts, counts, row_elems,
                                    pad)).all(), (filt, pad)
        assert (host == shardfmt.read_rows_cpu(
            packed, starts, counts, src, out, row_elems, pad)).all(), filt
        assert (host == _composed(d_comp, idx, starts, counts, src, out,
                                  row_elems, pad)).all(), filt
        # a subset that leaves blocks out, unverified
        eb = rc.BLOCK // size
        got = shardfmt.decode_rows_device(
            d_comp, idx, [3 * eb + 9, eb + 5], [eb - 9, 100], DEV, src, out,
            eb, 3, verify=False)
        assert (got.cpu().numpy() == rc.want(
            src, out, [3 * eb + 9, eb + 5], [eb - 9, 100], eb, 3)).all(), filt
        # the payload is never written
        assert bytes(d_comp.cpu().numpy().tobytes()) == \
            packed[idx.payload_off:]


def test_decode_rows_device_empty_requests(monkeypatch):
    packed = rc.packed("shuffle", 2)
    d_comp, idx = _on_device(packed)

    def boom(*a, **k):
        raise AssertionError("a block was decoded")

    for name in ("gather_copy", "lz4_decode_blocks", "crc32c_chunks",
                 "byte_shuffle", "gather_ranges"):
        monkeypatch.setattr(ops, name, boom)
    # rows that are all empty: pad everywhere, written by the kernel
    got = shardfmt.decode_rows_device(d_comp, idx, [0, 7, rc.N_RAW // 2],
                                      [0, 0, 0], DEV, "u2", "int64", 37, -100)
    assert tuple(got.shape) == (3, 37) and (got == -100).all().item()
    # no rows: no launch at all
    monkeypatch.setattr(ops, "gather_widen", boom)
    got = shardfmt.decode_rows_device(d_comp, idx, [], [], DEV, "u2",
                                      "int32", 37, 0)
    assert tuple(got.shape) == (0, 37) and got.dtype == torch.int32
    assert got.is_cuda


# --------------------------------------------------------------- stager
def test_stage_rows(tmp_path):
    src, out, size = "u2", "int64", 2
    packed = rc.packed("shuffle", size)
    path = tmp_path / "tokens.syshard"
    path.write_bytes(packed)
    idx = shardfmt.read_index(packed)
    st = ShardStager(staging_mb=1, verify=True)
    starts, counts, row_elems = rc.rows(size)
    got, res = st.stage_rows(path, starts, counts, src, out, row_elems, 50256)
    want = rc.want(src, out, starts, counts, row_elems, 50256)
    assert got.dtype == torch.int64
    assert (got.cpu().numpy() == want).all()
    assert res.decoded and res.verified
    assert res.raw_bytes == sum(counts) * size
    # the same file bytes as the byte-range read of the same rows
    _, res_b = st.stage_ranges(path, np.asarray(starts) * size,
                               np.asarray(counts) * size)
    assert res.file_bytes == res_b.file_bytes

    # blocks 1 and 3 only: two runs, nothing read in between
    eb = rc.BLOCK // size
    starts2, counts2 = [3 * eb + 9, eb + 5], [eb - 9, 100]
    assert idx.select_blocks(np.asarray(starts2) * size,
                             np.asarray(counts2) * size).tolist() == [1, 3]
    got, res = st.stage_rows(path, starts2, counts2, src, torch.int32, eb,
                             -100)
    assert (got.cpu().numpy() == rc.want(src, "int32", starts2, counts2, eb,
                                         -100)).all()
    head = shardfmt.HEADER.size + idx.n_blocks * shardfmt.ENTRY.size
    assert res.file_bytes == head + int(idx.table["comp_len"][1]) + \
        int(idx.table["comp_len"][3])

    def flipped(block):
        buf = bytearray(packed)
        buf[idx.payload_off + int(idx.table["comp_off"][block]) + 8] ^= 0x55
        bad = tmp_path / f"flipped{block}.syshard"
        bad.write_bytes(bytes(buf))
        return bad

    with pytest.raises(ValueError, match=r"CRC mismatch in blocks \[3\]"):
        st.stage_rows(flipped(3), starts2, counts2, src, out, eb, 0)
    for block in (0, 2, 4):  # not touched: not read, not noticed
        got, _ = st.stage_rows(flipped(block), starts2, counts2, src, out,
                               eb, 0)
        assert (got.cpu().numpy() == rc.want(src, out, starts2, counts2, eb,
                                             0)).all()

    got, res = st.stage_rows(path, [], [], src, out, 5, 0)
    assert tuple(got.shape) == (0, 5) and res.raw_bytes == 0
    assert res.file_bytes == head
    with pytest.raises(ValueError, match="row 0 has 9"):
        st.stage_rows(path, [0], [9], src, out, 8, 0)
    with pytest.raises(ValueError, match="does not fit"):
        st.stage_rows(path, [0], [1], "u4", "int32", 8, 0)
