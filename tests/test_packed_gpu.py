"""GPU tests of packed row reads: the ops.gather_pack kernel against a
numpy model built directly from its lists (every conversion, every path
of the kernel, both ends of the work split, guard bytes around all three
outputs), its argument errors, and shardfmt.decode_packed_device and
ShardStager.stage_packed against read_packed_cpu.  Every comparison is
exact."""
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import packed_cases as pc  # noqa: E402
import rows_cases as rc  # noqa: E402

from shipyard_amd import ops  # noqa: E402
from shipyard_amd.data import shardfmt  # noqa: E402
from shipyard_amd.data.stager import ShardStager  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"int32": torch.int32, "int64": torch.int64}
MARGIN_BYTES = 9 * 16  # guard on either side of an output: 16 B aligned
GUARD, JUNK = 0x5A, 0xC3  # byte values: around an output, in it beforehand
STEP = 256  # elements of one wave step: 64 lanes of 4


def _dev(v, dtype):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=dtype)).to(DEV)


def _src_view(src_np):
    """src as a view at byte 4 of its allocation: a base that is a
    multiple of every element size and not of 8 or 16."""
    big = torch.full((len(src_np) + 8,), 0x3C, dtype=torch.uint8, device=DEV)
    view = big[4:4 + len(src_np)]
    view.copy_(torch.from_numpy(src_np).to(DEV))
    return big, view


def _model(src_np, src, out, soff, counts, dstart, labels, n_elems, pad):
    """The three flat arrays from the lists: np.repeat and one fancy
    index each."""
    size = rc.SIZE[src]
    el = src_np[:len(src_np) // size * size].view(rc.NUMPY[src])
    tokens = np.full(n_elems, pad, dtype=out)
    seg = np.zeros(n_elems, dtype=np.int32)
    pos = np.zeros(n_elems, dtype=np.int32)
    counts = np.asarray(counts, dtype=np.int64)
    if len(counts):
        first = np.cumsum(counts) - counts
        within = np.arange(int(counts.sum())) - np.repeat(first, counts)
        at = np.repeat(np.asarray(dstart, dtype=np.int64), counts) + within
        tokens[at] = el[np.repeat(np.asarray(soff, dtype=np.int64) // size,
                                  counts) + within].astype(out)
        seg[at] = np.repeat(np.asarray(labels, dtype=np.int32), counts)
        pos[at] = within
    return tokens, seg, pos


def _guarded(n_elems, dtype):
    """A flat output of n_elems inside a larger buffer: guard bytes in
    front and behind, junk where the kernel must write.  Returns the
    byte buffer and the [n_elems] view."""
    nbytes = n_elems * dtype.itemsize
    big = torch.full((2 * MARGIN_BYTES + nbytes,), GUARD, dtype=torch.uint8,
                     device=DEV)
    big[MARGIN_BYTES:MARGIN_BYTES + nbytes] = JUNK
    view = big[MARGIN_BYTES:MARGIN_BYTES + nbytes].view(dtype)
    assert view.data_ptr() % 16 == 0
    return big, view


def _pack_and_compare(d_src, src_np, src, out, soff, counts, dstart, labels,
                      n, T, pad):
    """Run the kernel into three guarded outputs and compare the WHOLE
    buffers with the model: data, padding and both margins."""
    n_elems = n * T
    bufs = [_guarded(n_elems, dt)
            for dt in (TORCH[out], torch.int32, torch.int32)]
    tokens, seg, pos = (v.view(n, T) for _, v in bufs)
    ops.gather_pack(d_src, _dev(soff, np.int64), _dev(counts, np.int64),
                    _dev(dstart, np.int64), _dev(labels, np.int32), tokens,
                    seg, pos, src, pad)
    torch.cuda.current_stream().synchronize()
    want = _model(src_np, src, out, soff, counts, dstart, labels, n_elems,
                  pad)
    for (big, _), w, name in zip(bufs, want, ("tokens", "segment_ids",
                                              "positions")):
        host = big.cpu().numpy()
        assert (host[:MARGIN_BYTES] == GUARD).all(), name
        assert (host[len(host) - MARGIN_BYTES:] == GUARD).all(), name
        got = host[MARGIN_BYTES:len(host) - MARGIN_BYTES].view(w.dtype)
        bad = np.flatnonzero(got != w)
        assert not len(bad), (name, (n, T), len(bad), bad[:8].tolist(),
                              got[bad[:8]].tolist(), w[bad[:8]].tolist())


def _segments(n_elems: int):
    """(dst_start, counts) over a flat buffer of n_elems, as much of the
    following as fits, in this order: pad in front of the first segment;
    segments of 1..7 elements after gaps of 0..3, so that starts and
    ends fall on every residue mod 4; a gap of exactly one element; one
    segment of 1500 elements (whole steps of data, a pair of them too);
    1100 elements of pad (whole steps of pad); 520 one-element segments
    back to back (a step with 256 of them); then short ones again, and a
    last segment that ends on the last element."""
    start, count = [], []
    at = 5 if n_elems > 8 else 0

    def add(gap, c):
        nonlocal at
        if at + gap + c > n_elems:
            return False
        start.append(at + gap)
        count.append(c)
        at += gap + c
        return True

    ok = True
    for gap in range(4):
        for c in range(1, 8):
            ok = ok and add(gap, c)
    ok = ok and add(1, 3) and add(1, 2)
    ok = ok and add(2, 1500)
    ok = ok and add(1100, 9)
    for _ in range(520):
        ok = ok and add(0, 1)
    ok = ok and add(3, 300) and add(0, 2) and add(7, 1)
    if at < n_elems:  # up to the last element
        c = min(n_elems - at, 11)
        start.append(n_elems - c)
        count.append(c)
    return np.asarray(start, dtype=np.int64), np.asarray(count, dtype=np.int64)


def test_segments_cover_what_they_claim():
    """The case builder itself, at the largest of the small shapes."""
    start, count = _segments(4400)
    end = start + count
    assert start[0] > 0 and end[-1] == 4400
    assert (start[1:] >= end[:-1]).all()
    assert {int(s) % 4 for s in start} == {0, 1, 2, 3}
    assert {int(e) % 4 for e in end} == {0, 1, 2, 3}
    assert (start[1:] - end[:-1] == 1).any()
    # whole steps of one segment's data, two of them in a row
    long = int(np.argmax(count))
    first_step = -(-int(start[long]) // STEP)
    assert (first_step + 3) * STEP <= end[long]
    # whole steps of pad
    gap = int(np.argmax(start[1:] - end[:-1]))
    assert (-(-int(end[gap]) // STEP) + 2) * STEP <= start[gap + 1]
    # a step with at least 200 one-element segments
    ones = start[count == 1]
    assert np.bincount(ones // STEP).max() >= 200


# (n, T): every T of {1, 3, 5, 64, 257, 1000} with n * T a multiple of 4
# and, where T allows it, not; shapes of a few elements on top
SHAPES = [(4400, 1), (4403, 1), (1468, 3), (1467, 3), (880, 5), (881, 5),
          (69, 64), (20, 257), (19, 257), (5, 1000),
          (1, 1), (2, 3), (1, 5), (3, 5), (7, 64), (3, 257)]


def _src_bytes(size: int, n_el: int, rng):
    src_np = rng.integers(0, 256, n_el * size, dtype=np.uint8)
    src_np[:2 * size] = 0xFF  # -1 / the largest unsigned value, twice
    src_np[2 * size:3 * size] = 0  # the most negative value: 0x80 on top
    src_np[3 * size - 1] = 0x80
    src_np[3 * size:4 * size] = 0xFF  # the largest signed value
    src_np[4 * size - 1] = 0x7F
    return src_np


@pytest.mark.parametrize("pad_kind", ["minus-100", "max"])
@pytest.mark.parametrize("pair", rc.PAIRS, ids=rc.pair_id)
def test_gather_pack_against_numpy(pair, pad_kind):
    src, out = pair
    size = rc.SIZE[src]
    pad = -100 if pad_kind == "minus-100" else int(np.iinfo(out).max)
    rng = np.random.default_rng(100 * size + len(out) + len(pad_kind))
    n_el = 2003  # odd: the last element sits at an odd index
    src_np = _src_bytes(size, n_el, rng)
    big_src, d_src = _src_view(src_np)
    assert d_src.data_ptr() % 16 == 4
    for n, T in SHAPES:
        dstart, counts = _segments(n * T)
        m = len(counts)
        # sources anywhere, odd element indices among them; the extremes
        # at the front and the last byte of src are each read by someone
        soff = rng.integers(0, n_el - counts + 1)
        soff[::3] |= 1
        soff = np.minimum(soff, n_el - counts)
        soff[0] = 0
        soff[-1] = n_el - counts[-1]
        soff[m // 2] = n_el - counts[m // 2]
        labels = rng.integers(-2 ** 31, 2 ** 31, m)
        _pack_and_compare(d_src, src_np, src, out, soff * size, counts,
                          dstart, labels, n, T, pad)
    # the source is read-only, and so is what lies around it
    assert (big_src.cpu().numpy()[4:4 + len(src_np)] == src_np).all()
    assert (big_src[:4] == 0x3C).all().item()
    assert (big_src[4 + len(src_np):] == 0x3C).all().item()


@pytest.mark.parametrize("pair", [("u2", "int64"), ("i4", "int32")],
                         ids=rc.pair_id)
def test_no_segments_is_all_pad(pair):
    src, out = pair
    src_np = np.zeros(64, dtype=np.uint8)
    d_src = torch.from_numpy(src_np).to(DEV)
    none = np.zeros(0, dtype=np.int64)
    for n, T in ((1, 1), (3, 5), (9, 257)):
        _pack_and_compare(d_src, src_np, src, out, none, none, none, none,
                          n, T, 50256)
    # and without a source at all
    empty = torch.empty(0, dtype=torch.uint8, device=DEV)
    _pack_and_compare(empty, src_np[:0], src, out, none, none, none, none,
                      2, 300, -1)


def _grid_waves() -> int:
    text = (Path(ops.__file__).resolve().parent / "csrc" /
            "gather_pack.hip").read_text()
    grid = int(re.search(r"constexpr uint32_t kGrid = (\d+);", text).group(1))
    threads = int(re.search(r"constexpr uint32_t kThreads = (\d+);",
                            text).group(1))
    return grid * threads // 64


@pytest.mark.parametrize("pair", [("u1", "int32"), ("i2", "int32")],
                         ids=rc.pair_id)
def test_more_steps_than_waves(pair):
    """A buffer of 1.25 steps per wave of the full grid (and 3 steps and
    a partial group on top): every wave that works takes two steps, the
    last ones none.  Segments of every kind at random."""
    src, out = pair
    size = rc.SIZE[src]
    waves = _grid_waves()
    n_elems = (waves + waves // 4 + 3) * STEP + 2
    assert 16 << 20 <= n_elems * 12 <= 40 << 20
    T = 1003
    n = n_elems // T
    n_elems = n * T
    assert -(-n_elems // STEP) > waves
    rng = np.random.default_rng(11)
    m = 90000
    counts = rng.choice([1, 2, 3, 5, 17, 64, 300, 3000], m,
                        p=[.3, .2, .1, .1, .1, .1, .09, .01])
    gaps = rng.choice([0, 1, 2, 700], m, p=[.6, .2, .19, .01])
    ends = np.cumsum(counts + gaps)
    keep = ends <= n_elems
    counts, dstart = counts[keep], (ends - counts)[keep]
    assert len(counts) > 10000 and ends[keep][-1] > n_elems - 4000
    n_el = 1 << 19
    src_np = rng.integers(0, 256, n_el * size, dtype=np.uint8)
    soff = rng.integers(0, n_el - counts + 1)
    labels = rng.integers(1, 1000, len(counts))
    _pack_and_compare(torch.from_numpy(src_np).to(DEV), src_np, src, out,
                      soff * size, counts, dstart, labels, n, T, -100)


def test_no_elements_is_a_no_op_without_the_library(monkeypatch):
    def boom():
        raise AssertionError("library loaded for an empty output")

    monkeypatch.setattr(ops, "_load", boom)
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    e64 = torch.empty(0, dtype=torch.int64, device=DEV)
    e32 = torch.empty(0, dtype=torch.int32, device=DEV)
    for shape in ((0, 7), (2, 0)):
        ops.gather_pack(src, e64, e64, e64, e32,
                        torch.empty(shape, dtype=torch.int64, device=DEV),
                        torch.empty(shape, dtype=torch.int32, device=DEV),
                        torch.empty(shape, dtype=torch.int32, device=DEV),
                        "u2", 0)


def _good_args():
    """Arguments that pass every check, by name."""
    lists = _dev([0, 8], np.int64)
    return dict(
        src=torch.zeros(64, dtype=torch.uint8, device=DEV),
        src_off=lists, counts=_dev([1, 2], np.int64),
        dst_start=_dev([0, 4], np.int64), labels=_dev([1, 2], np.int32),
        tokens=torch.zeros((2, 4), dtype=torch.int32, device=DEV),
        segment_ids=torch.zeros((2, 4), dtype=torch.int32, device=DEV),
        positions=torch.zeros((2, 4), dtype=torch.int32, device=DEV),
        src_dtype="u2", pad=0)


def _plus_one(t):
    """The same shape and dtype one element past a 16-byte boundary."""
    big = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    return big[1:].view(t.shape)


GUARD_ERRORS = [
    ("src-dtype", "contiguous uint8", lambda a: a.update(
        src=a["src"].to(torch.int8))),
    ("src-strided", "contiguous uint8", lambda a: a.update(
        src=a["src"][::2])),
    ("src-misaligned", "multiple of the 2-byte", lambda a: a.update(
        src=a["src"][1:])),
    ("src-on-cpu", "not on a GPU", lambda a: a.update(
        {k: v.cpu() for k, v in a.items() if hasattr(v, "cpu")})),
    ("tokens-dtype", "tokens must be int32 or int64", lambda a: a.update(
        tokens=a["tokens"].to(torch.int16))),
    ("tokens-1d", r"contiguous \[n, T\]", lambda a: a.update(
        tokens=a["tokens"].view(-1))),
    ("tokens-strided", r"contiguous \[n, T\]", lambda a: a.update(
        tokens=torch.zeros((2, 8), dtype=torch.int32, device=DEV)[:, ::2])),
    ("tokens-device", "tokens is on", lambda a: a.update(
        tokens=a["tokens"].cpu())),
    ("tokens-misaligned", "tokens base pointer must be 16-byte",
     lambda a: a.update(tokens=_plus_one(a["tokens"]))),
    ("segment-ids-dtype", "segment_ids must be int32", lambda a: a.update(
        segment_ids=a["segment_ids"].to(torch.int64))),
    ("segment-ids-shape", "segment_ids must be a contiguous tensor of",
     lambda a: a.update(segment_ids=a["segment_ids"].view(4, 2))),
    ("segment-ids-device", "segment_ids is on", lambda a: a.update(
        segment_ids=a["segment_ids"].cpu())),
    ("segment-ids-misaligned", "segment_ids base pointer must be 16-byte",
     lambda a: a.update(segment_ids=_plus_one(a["segment_ids"]))),
    ("positions-dtype", "positions must be int32", lambda a: a.update(
        positions=a["positions"].to(torch.int16))),
    ("positions-strided", "positions must be a contiguous tensor of",
     lambda a: a.update(positions=torch.zeros(
         (2, 8), dtype=torch.int32, device=DEV)[:, ::2])),
    ("positions-misaligned", "positions base pointer must be 16-byte",
     lambda a: a.update(positions=_plus_one(a["positions"]))),
    ("src-off-dtype", "src_off must be int64", lambda a: a.update(
        src_off=a["src_off"].to(torch.int32))),
    ("counts-device", "counts is on", lambda a: a.update(
        counts=a["counts"].cpu())),
    ("dst-start-2d", "dst_start must be a contiguous 1-D", lambda a: a.update(
        dst_start=a["dst_start"].view(1, 2))),
    ("labels-dtype", "labels must be int32", lambda a: a.update(
        labels=a["labels"].to(torch.int64))),
    ("labels-device", "labels is on", lambda a: a.update(
        labels=a["labels"].cpu())),
    ("labels-strided", "labels must be a contiguous 1-D", lambda a: a.update(
        labels=_dev([1, 0, 2, 0], np.int32)[::2])),
    ("unequal-counts", "2 source offsets, 1 counts", lambda a: a.update(
        counts=a["counts"][:1])),
    ("unequal-labels", "3 labels", lambda a: a.update(
        labels=_dev([1, 2, 3], np.int32))),
    ("u4-into-int32", "does not fit int32", lambda a: a.update(
        src_dtype="u4")),
    ("unknown-type", "src_dtype", lambda a: a.update(src_dtype="i1")),
    ("pad-too-large", "pad", lambda a: a.update(pad=2 ** 31)),
    ("pad-not-an-integer", "pad", lambda a: a.update(pad=0.5)),
]


@pytest.mark.parametrize("case", GUARD_ERRORS, ids=[c[0] for c in
                                                    GUARD_ERRORS])
def test_argument_error_comes_before_any_launch(case, monkeypatch):
    _, message, spoil = case
    args = _good_args()
    spoil(args)

    def boom():
        raise AssertionError("library loaded despite bad arguments")

    monkeypatch.setattr(ops, "_load", boom)
    with pytest.raises(ValueError, match=message):
        ops.gather_pack(**args)


def test_good_arguments_pass():
    """What the error cases start from is itself accepted."""
    args = _good_args()
    ops.gather_pack(**args)
    assert args["tokens"].cpu().tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]
    assert args["segment_ids"].cpu().tolist() == [[1, 0, 0, 0], [2, 2, 0, 0]]
    assert args["positions"].cpu().tolist() == [[0, 0, 0, 0], [0, 1, 0, 0]]


# ---------------------------------------------------------- shard level
def _on_device(packed: bytes):
    idx = shardfmt.read_index(packed)
    payload = np.frombuffer(packed, dtype=np.uint8)[idx.payload_off:]
    return torch.from_numpy(payload.copy()).to(DEV), idx


def _same(got, want):
    for g, w in zip(got, want):
        assert g.is_cuda and tuple(g.shape) == w.shape
        assert str(g.dtype) == "torch." + w.dtype.name
        assert (g.cpu().numpy() == w).all()


@pytest.mark.parametrize("out", ["int32", "int64"])
@pytest.mark.parametrize("name", sorted(pc.SHARDS))
def test_decode_packed_device(name, out):
    src, size, _ = pc.SHARDS[name]
    packed = pc.packed(name)
    d_comp, idx = _on_device(packed)
    starts, counts = pc.samples(size)
    for T in (64, 130):
        row, col, n_rows = shardfmt.plan_packed_rows(counts, T)
        want = shardfmt.read_packed_cpu(packed, starts, counts, row, col,
                                        n_rows, src, out, T, -100)
        by_hand = pc.want(name, out, starts, counts, row.tolist(),
                          col.tolist(), n_rows, T, -100)
        for w, h in zip(want, by_hand):
            assert (w == h).all()
        _same(shardfmt.decode_packed_device(
            d_comp, idx, starts, counts, row, col, n_rows, DEV, src,
            TORCH[out], T, -100), want)
    # a plan of the caller's own: gaps, rows out of order, unverified
    row, col = [2, 0, 2, 1, 0, 0, 1, 2, 3], [30, 50, 1, 9, 0, 20, 60, 0, 3]
    want = shardfmt.read_packed_cpu(packed, starts, counts, row, col, 5, src,
                                    out, 128, 7)
    _same(shardfmt.decode_packed_device(
        d_comp, idx, starts, counts, row, col, 5, DEV, src, out, 128, 7,
        verify=False), want)
    # the payload is never written
    assert bytes(d_comp.cpu().numpy().tobytes()) == packed[idx.payload_off:]


def test_decode_packed_device_corrupt_block():
    packed = pc.packed("u2-shuffle")
    idx = shardfmt.read_index(packed)
    buf = bytearray(packed)
    buf[idx.payload_off + int(idx.table["comp_off"][3]) + 8] ^= 0x55
    d_comp, idx = _on_device(bytes(buf))
    touched = ([5, 3 * 4096 + 2], [9, 4], [0, 0], [0, 9], 1)
    with pytest.raises(ValueError, match=r"CRC mismatch in blocks \[3\]"):
        shardfmt.decode_packed_device(d_comp, idx, *touched, DEV, "u2",
                                      "int32", 16, 0)
    spared = ([5, 2 * 4096 + 2],) + touched[1:]
    _same(shardfmt.decode_packed_device(d_comp, idx, *spared, DEV, "u2",
                                        "int32", 16, 0),
          shardfmt.read_packed_cpu(packed, *spared, "u2", "int32", 16, 0))


def test_decode_packed_device_empty_requests(monkeypatch):
    packed = pc.packed("u2-shuffle")
    d_comp, idx = _on_device(packed)

    def boom(*a, **k):
        raise AssertionError("a block was decoded")

    for name in ("gather_copy", "lz4_decode_blocks", "crc32c_chunks",
                 "byte_shuffle", "gather_ranges", "gather_widen"):
        monkeypatch.setattr(ops, name, boom)
    # samples that are all empty: pad and zeros, written by the kernel
    tokens, seg, pos = shardfmt.decode_packed_device(
        d_comp, idx, [0, 7, pc.N_RAW // 2], [0, 0, 0], [0, 2, 1], [0, 37, 5],
        3, DEV, "u2", "int64", 37, -100)
    assert tuple(tokens.shape) == (3, 37) and (tokens == -100).all().item()
    assert not seg.any().item() and not pos.any().item()
    # no rows, or rows of no elements: no launch at all
    monkeypatch.setattr(ops, "gather_pack", boom)
    for n_rows, T, lists in ((0, 37, ([], [], [], [])),
                             (2, 0, ([3], [0], [1], [0]))):
        out = shardfmt.decode_packed_device(d_comp, idx, *lists, n_rows, DEV,
                                            "u2", "int32", T, 0)
        assert all(tuple(t.shape) == (n_rows, T) and t.is_cuda and
                   t.dtype == torch.int32 for t in out)
    # a bad plan raises before anything is made
    with pytest.raises(ValueError, match="sample 1 .*overlaps sample 0"):
        shardfmt.decode_packed_device(d_comp, idx, [0, 9], [4, 4], [0, 0],
                                      [0, 3], 1, DEV, "u2", "int32", 8, 0)


# --------------------------------------------------------------- stager
@pytest.mark.parametrize("name", sorted(pc.SHARDS))
def test_stage_packed(name, tmp_path):
    src, size, _ = pc.SHARDS[name]
    packed = pc.packed(name)
    path = tmp_path / "tokens.syshard"
    path.write_bytes(packed)
    idx = shardfmt.read_index(packed)
    st = ShardStager(staging_mb=1, verify=True)
    starts, counts = pc.samples(size)
    row, col, n_rows = shardfmt.plan_packed_rows(counts, 64)
    got, res = st.stage_packed(path, starts, counts, row, col, n_rows, src,
                               "int64", 64, 50256)
    _same(got, shardfmt.read_packed_cpu(packed, starts, counts, row, col,
                                        n_rows, src, "int64", 64, 50256))
    assert res.decoded and res.verified
    assert res.raw_bytes == sum(counts) * size
    # the same file bytes as the row read of the same samples
    _, res_r = st.stage_rows(path, starts, counts, src, "int64", 64, 0)
    assert res.file_bytes == res_r.file_bytes

    eb = pc.BLOCK // size
    touched = ([5, 3 * eb + 2], [9, 4], [0, 0], [0, 9], 1)
    buf = bytearray(packed)
    buf[idx.payload_off + int(idx.table["comp_off"][3]) + 8] ^= 0x55
    bad = tmp_path / "flipped.syshard"
    bad.write_bytes(bytes(buf))
    with pytest.raises(ValueError, match=r"CRC mismatch in blocks \[3\]"):
        st.stage_packed(bad, *touched, src, "int32", 16, 0)
    spared = ([5, 2 * eb + 2],) + touched[1:]
    got, _ = st.stage_packed(bad, *spared, src, "int32", 16, 0)
    _same(got, shardfmt.read_packed_cpu(packed, *spared, src, "int32", 16,
                                        0))

    head = shardfmt.HEADER.size + idx.n_blocks * shardfmt.ENTRY.size
    got, res = st.stage_packed(path, [1, 2], [0, 0], [0, 0], [0, 0], 1, src,
                               "int32", 6, -1)
    assert (got[0] == -1).all().item() and not got[1].any().item()
    assert not got[2].any().item()
    assert res.raw_bytes == 0 and res.file_bytes == head
    with pytest.raises(ValueError, match="sample 0 .*row_elems=8"):
        st.stage_packed(path, [0], [4], [0], [5], 1, src, "int32", 8, 0)
