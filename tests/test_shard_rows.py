"""CPU tests of typed SYSHARD row reads: read_rows_cpu against slices of
the original array for every allowed conversion, filter and pad, sign
handling, and the host checks of read_rows_cpu and decode_rows_device,
which fire before anything is launched (no ops library, CPU tensors).
Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rows_cases as rc  # noqa: E402

from shipyard_amd import ops  # noqa: E402
from shipyard_amd.data import shardfmt  # noqa: E402


@pytest.mark.parametrize("pair", rc.PAIRS, ids=rc.pair_id)
def test_read_rows_cpu_equals_slices(pair):
    src, out = pair
    size = rc.SIZE[src]
    assert size == 1 or (rc.N_RAW - 5 * rc.BLOCK) % size
    starts, counts, row_elems = rc.rows(size)
    for filt, _ in rc.filters(size):
        packed = rc.packed(filt, size)
        idx = shardfmt.read_index(packed)
        assert idx.n_blocks == 6 and int(idx.table["raw_len"][-1]) == 1003
        for pad in rc.pads(out):
            got = shardfmt.read_rows_cpu(packed, starts, counts, src,
                                         np.dtype(out), row_elems, pad)
            assert got.dtype == np.dtype(out), (filt, pad)
            assert got.shape == (len(starts), row_elems)
            assert (got == rc.want(src, out, starts, counts, row_elems,
                                   pad)).all(), (filt, pad)
        got = shardfmt.read_rows_cpu(packed, starts, counts, src, out,
                                     row_elems, 7, verify=False)
        assert (got == rc.want(src, out, starts, counts, row_elems,
                               7)).all(), filt


def test_out_dtype_spellings():
    torch = pytest.importorskip("torch")
    packed = rc.packed("plain", 2)
    ref = shardfmt.read_rows_cpu(packed, [3], [4], "u2", np.int64, 6, -1)
    for spelling in ("int64", np.dtype("int64"), torch.int64, "<i8"):
        got = shardfmt.read_rows_cpu(packed, [3], [4], "u2", spelling, 6, -1)
        assert got.dtype == np.int64 and (got == ref).all()


def test_sign_handling():
    vals = np.array([0xFFFF, 0x8000, 0x7FFF, 0, 1], dtype="<u2")
    packed = shardfmt.pack(vals.tobytes(), block_raw=rc.BLOCK)
    for out in ("int32", "int64"):
        got = shardfmt.read_rows_cpu(packed, [0], [5], "i2", out, 5, 0)
        assert got.tolist() == [[-1, -32768, 32767, 0, 1]]
        got = shardfmt.read_rows_cpu(packed, [0], [5], "u2", out, 5, 0)
        assert got.tolist() == [[65535, 32768, 32767, 0, 1]]
    vals = np.array([0xFFFFFFFF, 0x80000000, 5], dtype="<u4")
    packed = shardfmt.pack(vals.tobytes(), block_raw=rc.BLOCK)
    got = shardfmt.read_rows_cpu(packed, [0], [3], "i4", "int32", 4, -100)
    assert got.tolist() == [[-1, -2 ** 31, 5, -100]]
    got = shardfmt.read_rows_cpu(packed, [0], [3], "i4", "int64", 4, -100)
    assert got.tolist() == [[-1, -2 ** 31, 5, -100]]
    got = shardfmt.read_rows_cpu(packed, [0], [3], "u4", "int64", 4, -100)
    assert got.tolist() == [[2 ** 32 - 1, 2 ** 31, 5, -100]]
    packed = shardfmt.pack(bytes([255, 128, 3]), block_raw=rc.BLOCK)
    got = shardfmt.read_rows_cpu(packed, [0], [3], "u1", "int32", 3, 0)
    assert got.tolist() == [[255, 128, 3]]


def test_empty_requests():
    packed = rc.packed("plain", 2)
    got = shardfmt.read_rows_cpu(packed, [], [], "u2", "int32", 9, 1)
    assert got.shape == (0, 9) and got.dtype == np.int32
    got = shardfmt.read_rows_cpu(packed, [0, 5], [0, 0], "u2", "int64", 3,
                                 50256)
    assert got.tolist() == [[50256] * 3] * 2
    got = shardfmt.read_rows_cpu(packed, [0, 5], [0, 0], "u2", "int64", 0, 0)
    assert got.shape == (2, 0)


# (starts, counts, src, out, row_elems, pad, what the message names)
N2 = rc.N_RAW // 2   # u2 elements that can be addressed; one byte is left
N4 = rc.N_RAW // 4
BAD = {
    "uneven": ([0, 1], [1], "u2", "int32", 4, 0, "starts but"),
    "neg-start": ([0, -1], [1, 1], "u2", "int32", 4, 0, "row 1"),
    "neg-count": ([0, 0, 0], [1, 1, -1], "u2", "int32", 4, 0, "row 2"),
    "one-past": ([0, N2 - 3], [1, 4], "u2", "int32", 4, 0, "row 1"),
    "start-past": ([N2 + 1], [0], "u2", "int32", 4, 0, "row 0"),
    "trailing-bytes": ([N4 - 1], [2], "u4", "int64", 4, 0, "row 0"),
    "huge-start": ([2 ** 62], [2 ** 62], "u4", "int64", 2 ** 62, 0, "row 0"),
    "count-over-row": ([0, 0], [4, 5], "u2", "int32", 4, 0, "row 1 has 5"),
    "neg-row-elems": ([0], [0], "u2", "int32", -1, 0, "row_elems"),
    "src-dtype": ([0], [1], "u8", "int64", 4, 0, "src_dtype"),
    "src-dtype-i1": ([0], [1], "i1", "int64", 4, 0, "src_dtype"),
    "out-dtype": ([0], [1], "u2", "int16", 4, 0, "out_dtype"),
    "out-dtype-float": ([0], [1], "u2", np.float32, 4, 0, "out_dtype"),
    "u4-to-int32": ([0], [1], "u4", "int32", 4, 0, "does not fit"),
    "pad-high-32": ([0], [1], "u2", "int32", 4, 2 ** 31, "pad"),
    "pad-low-32": ([0], [1], "u2", "int32", 4, -2 ** 31 - 1, "pad"),
    "pad-high-64": ([0], [1], "u2", "int64", 4, 2 ** 63, "pad"),
    "pad-low-64": ([0], [1], "u2", "int64", 4, -2 ** 63 - 1, "pad"),
    "pad-float": ([0], [1], "u2", "int64", 4, 0.5, "pad"),
}


@pytest.mark.parametrize("case", list(BAD))
def test_read_rows_cpu_rejects(case):
    starts, counts, src, out, row_elems, pad, names = BAD[case]
    with pytest.raises(ValueError, match=names):
        shardfmt.read_rows_cpu(rc.packed("plain", 2), starts, counts, src,
                               out, row_elems, pad)


def test_limits_that_are_fine():
    packed = rc.packed("plain", 2)
    # the last addressable element; the byte behind it is out of reach
    got = shardfmt.read_rows_cpu(packed, [N2 - 1, N2], [1, 0], "u2",
                                 "int32", 1, -2 ** 31)
    assert got.tolist() == [[int(rc.elements("u2")[-1])], [-2 ** 31]]
    got = shardfmt.read_rows_cpu(packed, [0], [0], "u2", "int64", 1,
                                 2 ** 63 - 1)
    assert got.tolist() == [[2 ** 63 - 1]]


class _NoOps:
    """Stands in for every device op: a call is a failed test."""

    def __getattr__(self, name):
        def boom(*a, **k):
            raise AssertionError(f"ops.{name} was called")

        return boom


@pytest.mark.parametrize("case", list(BAD))
def test_decode_rows_device_checks_before_any_launch(case, monkeypatch):
    """CPU tensors and no ops library: the checks come first."""
    torch = pytest.importorskip("torch")
    stub = _NoOps()
    for name in ("_load", "gather_widen", "gather_ranges", "gather_copy",
                 "lz4_decode_blocks", "crc32c_chunks", "byte_shuffle",
                 "delta_filter", "bit_shuffle"):
        monkeypatch.setattr(ops, name, getattr(stub, name))
    made = []
    monkeypatch.setattr(torch, "empty", lambda *a, **k: made.append(a))
    packed = rc.packed("shuffle", 2)
    idx = shardfmt.read_index(packed)
    d_comp = torch.frombuffer(bytearray(packed[idx.payload_off:]),
                              dtype=torch.uint8)
    starts, counts, src, out, row_elems, pad, names = BAD[case]
    with pytest.raises(ValueError, match=names):
        shardfmt.decode_rows_device(d_comp, idx, starts, counts, "cpu", src,
                                    out, row_elems, pad)
    assert not made


def test_decode_rows_device_checks_the_index_first():
    torch = pytest.importorskip("torch")
    packed = rc.packed("plain", 2)
    idx = shardfmt.read_index(packed)
    d_comp = torch.frombuffer(bytearray(packed[idx.payload_off:]),
                              dtype=torch.uint8)
    with pytest.raises(ValueError, match="beyond the payload"):
        shardfmt.decode_rows_device(d_comp[:100], idx, [0], [-1], "cpu",
                                    "u2", "int32", 4, 0)
