"""CPU tests of packed row reads: the next-fit plan
(shardfmt.plan_packed_rows), the numpy reference reader
(shardfmt.read_packed_cpu) against hand-built expectations and against
read_rows_cpu, and every argument error with the sample it names.  No
device is needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import packed_cases as pc  # noqa: E402

from shipyard_amd.data import shardfmt  # noqa: E402

U2 = "u2-shuffle"


# ----------------------------------------------------------------- plan
def test_plan_next_fit():
    row, col, n_rows = shardfmt.plan_packed_rows([3, 2, 4, 0, 1, 5], 5)
    assert row.dtype == np.int64 and col.dtype == np.int64
    assert row.tolist() == [0, 0, 1, 1, 1, 2]
    assert col.tolist() == [0, 3, 0, 4, 4, 0]
    assert n_rows == 3 and isinstance(n_rows, int)


def test_plan_sample_as_long_as_a_row():
    row, col, n_rows = shardfmt.plan_packed_rows([5, 5, 1, 4, 5], 5)
    assert row.tolist() == [0, 1, 2, 2, 3]
    assert col.tolist() == [0, 0, 0, 1, 0]
    assert n_rows == 4


def test_plan_no_samples_and_empty_samples():
    row, col, n_rows = shardfmt.plan_packed_rows([], 5)
    assert len(row) == 0 and len(col) == 0 and n_rows == 0
    # empty samples take the cursor's place, also in a full row
    row, col, n_rows = shardfmt.plan_packed_rows([0, 5, 0, 1], 5)
    assert row.tolist() == [0, 0, 0, 1]
    assert col.tolist() == [0, 0, 5, 0]
    assert n_rows == 2
    row, col, n_rows = shardfmt.plan_packed_rows([0, 0], 0)
    assert row.tolist() == [0, 0] and col.tolist() == [0, 0] and n_rows == 1


def test_plan_negative_row_elems():
    with pytest.raises(ValueError, match="row_elems=-1"):
        shardfmt.plan_packed_rows([1], -1)


def test_plan_negative_count():
    with pytest.raises(ValueError, match="sample 2 has -1"):
        shardfmt.plan_packed_rows([1, 2, -1, -3], 5)


def test_plan_count_above_row_elems():
    with pytest.raises(ValueError, match="sample 1 has 6"):
        shardfmt.plan_packed_rows([5, 6, 7], 5)


# --------------------------------------------------------------- reader
def test_read_packed_cpu_by_hand():
    """A gap inside a row (columns 0..2 and 15..19 of row 0), an empty
    sample, a sample over the boundary of blocks 0 and 1 (elements
    4090..4101), one that ends on the last addressable element."""
    packed = pc.packed(U2)
    assert len(pc.raw()) == 40 * 1024 + 6
    idx = shardfmt.read_index(packed)
    assert idx.block_raw == 8192 and idx.shuffle_elem == 2
    el = pc.elements(U2)
    starts, counts = [4090, 100, 7, 20480], [12, 5, 0, 3]
    row, col = [0, 0, 0, 1], [3, 20, 20, 61]
    tokens, seg, pos = shardfmt.read_packed_cpu(
        packed, starts, counts, row, col, 2, "u2", "int64", 64, -100)
    assert tokens.dtype == np.int64 and tokens.shape == (2, 64)
    assert seg.dtype == np.int32 and pos.dtype == np.int32
    want_t = np.full((2, 64), -100, dtype=np.int64)
    want_s = np.zeros((2, 64), dtype=np.int32)
    want_p = np.zeros((2, 64), dtype=np.int32)
    want_t[0, 3:15] = el[4090:4102]
    want_s[0, 3:15] = 1
    want_p[0, 3:15] = np.arange(12)
    want_t[0, 20:25] = el[100:105]
    want_s[0, 20:25] = 2
    want_p[0, 20:25] = np.arange(5)
    want_t[1, 61:64] = el[20480:20483]
    want_s[1, 61:64] = 1
    want_p[1, 61:64] = np.arange(3)
    assert (tokens == want_t).all()
    assert (seg == want_s).all()
    assert (pos == want_p).all()


@pytest.mark.parametrize("name", sorted(pc.SHARDS))
def test_read_packed_cpu_with_a_plan(name):
    src, size, _ = pc.SHARDS[name]
    starts, counts = pc.samples(size)
    row, col, n_rows = shardfmt.plan_packed_rows(counts, 64)
    assert n_rows > 2
    got = shardfmt.read_packed_cpu(pc.packed(name), starts, counts, row, col,
                                   n_rows, src, "int32", 64, 2 ** 31 - 1)
    want = pc.want(name, "int32", starts, counts, row.tolist(), col.tolist(),
                   n_rows, 64, 2 ** 31 - 1)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and (g == w).all()
    # the same samples in another order of arguments and of columns
    order = [8, 3, 0, 7, 6, 1, 5, 2, 4]
    got2 = shardfmt.read_packed_cpu(
        pc.packed(name), [starts[i] for i in order],
        [counts[i] for i in order], row[order], col[order], n_rows, src,
        "int32", 64, 2 ** 31 - 1)
    for g, w in zip(got2, want):
        assert (g == w).all()


def test_one_sample_per_row_is_a_row_read():
    starts, counts = pc.samples(2)
    n, T = len(starts), 70
    counts_np = np.asarray(counts)
    tokens, seg, pos = shardfmt.read_packed_cpu(
        pc.packed(U2), starts, counts, np.arange(n), np.zeros(n, dtype=int),
        n, "u2", "int64", T, 50256)
    assert (tokens == shardfmt.read_rows_cpu(
        pc.packed(U2), starts, counts, "u2", "int64", T, 50256)).all()
    live = np.arange(T)[None, :] < counts_np[:, None]
    assert (seg == live).all()
    assert (pos == np.where(live, np.arange(T)[None, :], 0)).all()


def test_degenerate_shapes():
    packed = pc.packed(U2)
    for n_rows, T, args in ((0, 9, ([], [], [], [])),
                            (3, 0, ([1, 2], [0, 0], [0, 2], [0, 0]))):
        out = shardfmt.read_packed_cpu(packed, *args, n_rows, "u2", "int32",
                                       T, 0)
        assert [a.shape for a in out] == [(n_rows, T)] * 3
        assert [a.dtype for a in out] == [np.int32] * 3
    # nothing but empty samples: pad and zeros
    tokens, seg, pos = shardfmt.read_packed_cpu(
        packed, [0, 9], [0, 0], [0, 1], [0, 4], 2, "u2", "int64", 4, -7)
    assert (tokens == -7).all() and not seg.any() and not pos.any()


def test_untouched_corrupt_block_goes_unnoticed():
    packed = pc.packed(U2)
    idx = shardfmt.read_index(packed)
    buf = bytearray(packed)
    buf[idx.payload_off + int(idx.table["comp_off"][3]) + 8] ^= 0x55
    args = ([5, 3 * 4096 + 2], [9, 4], [0, 0], [0, 9], 1, "u2", "int32", 16, 0)
    with pytest.raises(ValueError, match=r"CRC mismatch in shard blocks \[3\]"):
        shardfmt.read_packed_cpu(bytes(buf), *args)
    args = ([5, 2 * 4096 + 2],) + args[1:]
    good = shardfmt.read_packed_cpu(packed, *args)
    for g, w in zip(shardfmt.read_packed_cpu(bytes(buf), *args), good):
        assert (g == w).all()


# --------------------------------------------------------------- errors
def _read(starts, counts, row, col, n_rows, src="u2", out="int32", T=8,
          pad=0):
    return shardfmt.read_packed_cpu(pc.packed(U2), starts, counts, row, col,
                                    n_rows, src, out, T, pad)


def test_error_rows_checks_are_reused():
    n_el = pc.N_RAW // 2
    with pytest.raises(ValueError, match="row_elems=-1"):
        _read([0], [0], [0], [0], 1, T=-1)
    with pytest.raises(ValueError, match="2 starts but 1 counts"):
        _read([0, 1], [1], [0, 0], [0, 1], 1)
    with pytest.raises(ValueError, match="row 1 .start -1"):
        _read([0, -1], [1, 1], [0, 0], [0, 1], 1)
    with pytest.raises(ValueError, match="row 2 .start 3, count -2"):
        _read([0, 1, 3], [1, 1, -2], [0, 0, 0], [0, 1, 2], 1)
    with pytest.raises(ValueError, match="row 1 .*ends past"):
        _read([0, n_el - 2], [1, 3], [0, 0], [0, 1], 1)
    with pytest.raises(ValueError, match="row 1 has 9 elements"):
        _read([0, 0], [1, 9], [0, 1], [0, 0], 2)


def test_error_unequal_lengths():
    with pytest.raises(ValueError, match="2 starts and counts but 1 rows"):
        _read([0, 1], [1, 1], [0], [0, 1], 1)
    with pytest.raises(ValueError, match="3 columns"):
        _read([0, 1], [1, 1], [0, 0], [0, 1, 2], 1)


def test_error_negative_n_rows():
    with pytest.raises(ValueError, match="n_rows=-1"):
        _read([], [], [], [], -1)


def test_error_row_out_of_range():
    with pytest.raises(ValueError, match="sample 1 .row 2.* outside the 2"):
        _read([0, 1, 2], [1, 1, 1], [0, 2, 3], [0, 0, 0], 2)
    with pytest.raises(ValueError, match="sample 0 .row -1"):
        _read([0, 1], [1, 1], [-1, 0], [0, 0], 2)
    # an empty sample is checked like any other
    with pytest.raises(ValueError, match="sample 0 .row 0.* outside the 0"):
        _read([0], [0], [0], [0], 0)


def test_error_negative_column():
    with pytest.raises(ValueError, match="sample 2 .row 0, column -1"):
        _read([0, 1, 2], [1, 1, 1], [0, 0, 0], [0, 1, -1], 1)


def test_error_sample_ends_behind_the_row():
    with pytest.raises(ValueError,
                       match="sample 1 .row 0, column 6, count 3.*row_elems=8"):
        _read([0, 1, 2], [1, 3, 8], [0, 0, 0], [0, 6, 1], 1)
    # an empty sample may sit at row_elems
    _read([0, 1], [8, 0], [0, 0], [0, 8], 1)


def test_error_overlap_names_the_later_sample():
    # in column order: sample 1 runs into sample 2
    with pytest.raises(ValueError, match="sample 2 .*overlaps sample 1"):
        _read([0, 10, 20], [2, 3, 2], [0, 0, 0], [0, 2, 4], 1)
    # out of column order: the later one in the caller's order is named,
    # here the one at the smaller column
    with pytest.raises(ValueError, match="sample 2 .*overlaps sample 0"):
        _read([0, 10, 20], [2, 2, 3], [0, 0, 0], [4, 0, 2], 1)
    # one long sample over two short ones: the first pair in caller order
    with pytest.raises(ValueError, match="sample 1 .*overlaps sample 0"):
        _read([0, 10, 20], [8, 1, 1], [0, 0, 0], [0, 5, 2], 1)
    # the same place twice
    with pytest.raises(ValueError, match="sample 1 .*overlaps sample 0"):
        _read([0, 0], [2, 2], [1, 1], [3, 3], 2)
    # empty samples overlap nothing; other rows do not matter
    _read([0, 10, 20, 30], [4, 0, 4, 4], [0, 0, 0, 1], [0, 2, 4, 2], 2)


def test_error_types_and_pad():
    with pytest.raises(ValueError, match="does not fit int32"):
        _read([0], [1], [0], [0], 1, src="u4")
    with pytest.raises(ValueError, match="src_dtype"):
        _read([0], [1], [0], [0], 1, src="i1")
    with pytest.raises(ValueError, match="out_dtype"):
        _read([0], [1], [0], [0], 1, out="int16")
    with pytest.raises(ValueError, match="pad"):
        _read([0], [1], [0], [0], 1, pad=2 ** 31)
