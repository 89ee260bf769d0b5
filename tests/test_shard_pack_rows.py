"""CPU tests of typed row writes: shardfmt.narrow_rows_numpy against a
plain Python loop, the limits of every destination type, the misfit
rule (live values only, first in stream order), shardfmt.pack_rows
round trips through read_rows_cpu, the offsets sidecar recipe, and the
argument errors.  Needs neither a GPU nor the ops library; every
comparison is exact."""
import numpy as np
import pytest

from shipyard_amd.data import shardfmt

DTYPES = {"u1": "<u1", "u2": "<u2", "i2": "<i2", "u4": "<u4", "i4": "<i4"}
LIMITS = {"u1": (0, 255), "u2": (0, 65535), "i2": (-32768, 32767),
          "u4": (0, 2 ** 32 - 1), "i4": (-2 ** 31, 2 ** 31 - 1)}
PAIRS = [(src, dt) for src in ("int32", "int64") for dt in DTYPES]


def _pair_id(pair):
    return f"{pair[0]}-{pair[1]}"


def _fitting(rng, src: str, dt: str, shape):
    """Random values that both the source array and ``dt`` hold, the
    limits among them."""
    lo, hi = LIMITS[dt]
    hi = min(hi, np.iinfo(src).max)
    vals = rng.integers(lo, hi + 1, shape, dtype=np.int64)
    flat = vals.reshape(-1)
    if len(flat) >= 2:
        flat[0], flat[-1] = lo, hi
    return vals.astype(src)


def _loop(rows, counts, dt: str):
    """The stream and row_start, element by element."""
    out, row_start = bytearray(), [0]
    size = np.dtype(DTYPES[dt]).itemsize
    for i, c in enumerate(counts):
        for j in range(c):
            out += (int(rows[i, j]) % (1 << (8 * size))).to_bytes(
                size, "little")
        row_start.append(row_start[-1] + c)
    return bytes(out), row_start


@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
def test_narrow_rows_numpy_against_a_loop(pair):
    src, dt = pair
    rng = np.random.default_rng(3)
    n, T = 13, 9
    rows = _fitting(rng, src, dt, (n, T))
    counts = [0, 1, 2, 3, 7, 8, 9, 0, 0, 9, 5, 0, 4]
    stream, row_start = shardfmt.narrow_rows_numpy(rows, counts, dt)
    want, want_start = _loop(rows, counts, dt)
    assert stream == want
    assert row_start.dtype == np.int64 and row_start.tolist() == want_start
    # the stream read back as the type is the live values
    live = np.arange(T)[None, :] < np.asarray(counts)[:, None]
    assert (np.frombuffer(stream, dtype=DTYPES[dt]).astype(np.int64)
            == rows[live].astype(np.int64)).all()


@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
def test_narrow_rows_numpy_empty_shapes(pair):
    src, dt = pair
    for shape, counts in (((0, 5), []), ((4, 0), [0, 0, 0, 0]),
                          ((0, 0), []), ((3, 6), [0, 0, 0])):
        stream, row_start = shardfmt.narrow_rows_numpy(
            np.full(shape, -100, dtype=src), counts, dt)
        assert stream == b""
        assert row_start.dtype == np.int64
        assert row_start.tolist() == [0] * (shape[0] + 1)


# (source, type, values just inside, values just outside)
EDGES = [
    ("int32", "u1", (0, 255), (-1, 256)),
    ("int64", "u1", (0, 255), (-1, 256)),
    ("int32", "u2", (0, 65535), (65536, -1)),
    ("int64", "u2", (0, 65535), (65536, -1)),
    ("int32", "i2", (-32768, 32767), (-32769, 32768)),
    ("int64", "i2", (-32768, 32767), (-32769, 32768)),
    ("int32", "u4", (0, 2 ** 31 - 1), (-1,)),
    ("int64", "u4", (0, 2 ** 32 - 1), (2 ** 32, -1)),
    ("int32", "i4", (-2 ** 31, 2 ** 31 - 1), ()),
    ("int64", "i4", (-2 ** 31, 2 ** 31 - 1), (-2 ** 31 - 1, 2 ** 31)),
]


@pytest.mark.parametrize("edge", EDGES, ids=lambda e: f"{e[0]}-{e[1]}")
def test_limits_of_every_type(edge):
    src, dt, inside, outside = edge
    n, T = 4, 5
    counts = [5, 0, 3, 4]
    for v in inside:
        rows = np.zeros((n, T), dtype=src)
        rows[2, 2] = v
        stream, _ = shardfmt.narrow_rows_numpy(rows, counts, dt)
        assert int(np.frombuffer(stream, dtype=DTYPES[dt])[5 + 2]) == v
    for v in outside:
        rows = np.zeros((n, T), dtype=src)
        rows[2, 2] = v
        with pytest.raises(ValueError) as err:
            shardfmt.narrow_rows_numpy(rows, counts, dt)
        text = str(err.value)
        assert "row 2, column 2 " in text, text
        assert f"holds {v}," in text and dt in text, text


def test_padding_is_never_checked():
    rows = np.full((3, 6), -100, dtype=np.int64)
    counts = [2, 0, 5]
    rows[0, :2] = (1, 65535)
    rows[2, :5] = (5, 4, 3, 2, 1)
    stream, row_start = shardfmt.narrow_rows_numpy(rows, counts, "u2")
    assert np.frombuffer(stream, dtype="<u2").tolist() == \
        [1, 65535, 5, 4, 3, 2, 1]
    assert row_start.tolist() == [0, 2, 2, 7]


def test_first_misfit_in_stream_order_is_reported():
    rows = np.zeros((5, 4), dtype=np.int64)
    counts = [4, 0, 2, 4, 1]
    rows[3, 0] = 70000    # stream index 6
    rows[2, 1] = -7       # stream index 5: the first
    rows[4, 0] = 1 << 40  # stream index 10
    rows[2, 3] = 99999    # padding
    with pytest.raises(ValueError, match=r"row 2, column 1 holds -7, "
                                         r"which u2 \(0\.\.65535\)"):
        shardfmt.narrow_rows_numpy(rows, counts, "u2")
    # an empty row in front of the offender does not take its place
    rows[2, 1] = 0
    rows[2, 0] = 65536    # stream index 4 == row_start[1] == row_start[2]
    with pytest.raises(ValueError, match="row 2, column 0 holds 65536,"):
        shardfmt.narrow_rows_numpy(rows, counts, "u2")


FILTERS = [dict(), dict(shuffle_elem=2), dict(delta_elem=4,
                                               bitshuffle_elem=4)]


@pytest.mark.parametrize("filt", FILTERS, ids=["plain", "shuffle", "delta-bit"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_pack_rows_round_trip(dt, filt):
    rng = np.random.default_rng(11)
    n, T, pad = 37, 300, -100
    size = np.dtype(DTYPES[dt]).itemsize
    rows = _fitting(rng, "int64", dt, (n, T))
    counts = rng.integers(0, T + 1, n)
    counts[:4] = (T, 0, 1, T - 1)
    live = np.arange(T)[None, :] < counts[:, None]
    rows[~live] = pad
    block_raw = 1024  # rows of up to 300 * size bytes cross blocks
    shard, row_start = shardfmt.pack_rows(rows, counts, dt,
                                          block_raw=block_raw, **filt)
    assert int(row_start[-1]) * size % block_raw  # a ragged final block
    idx = shardfmt.read_index(shard)
    assert idx.raw_size == int(counts.sum()) * size
    got = shardfmt.read_rows_cpu(shard, row_start[:-1], np.diff(row_start),
                                 dt, "int64", T, pad)
    assert got.dtype == np.int64 and (got == rows).all()
    assert shardfmt.unpack_cpu(shard) == \
        shardfmt.narrow_rows_numpy(rows, counts, dt)[0]


def test_pack_rows_int32_batch_and_workers():
    rng = np.random.default_rng(12)
    rows = _fitting(rng, "int32", "u2", (20, 64))
    counts = rng.integers(0, 65, 20)
    shard, row_start = shardfmt.pack_rows(rows, counts, "u2", block_raw=512,
                                          shuffle_elem=2, workers=None)
    got = shardfmt.read_rows_cpu(shard, row_start[:-1], np.diff(row_start),
                                 "u2", "int32", 64, 0)
    live = np.arange(64)[None, :] < counts[:, None]
    assert (got == np.where(live, rows, 0)).all()


def test_offsets_sidecar_recipe():
    counts = np.random.default_rng(13).integers(0, 4097, 3000)
    row_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    side = shardfmt.pack(row_start.tobytes(), delta_elem=8,
                         bitshuffle_elem=8)
    back = np.frombuffer(shardfmt.unpack_cpu(side), dtype=np.int64)
    assert (back == row_start).all()
    assert (np.diff(back) == counts).all() and (back[:-1] >= 0).all()
    assert len(side) < row_start.nbytes  # the filters earn their keep


def test_row_start_of_pack_rows_round_trips_as_a_sidecar():
    rng = np.random.default_rng(14)
    rows = _fitting(rng, "int64", "i2", (50, 40))
    counts = rng.integers(0, 41, 50)
    shard, row_start = shardfmt.pack_rows(rows, counts, "i2", block_raw=256)
    side = shardfmt.pack(row_start.tobytes(), delta_elem=8,
                         bitshuffle_elem=8)
    back = np.frombuffer(shardfmt.unpack_cpu(side), dtype=np.int64)
    got = shardfmt.read_rows_cpu(shard, back[:-1], np.diff(back), "i2",
                                 "int64", 40, 7)
    live = np.arange(40)[None, :] < counts[:, None]
    assert (got == np.where(live, rows, 7)).all()


@pytest.mark.parametrize("counts, row", [
    ([1, 2], None), ([1, 2, 3, 4], None), ([1, -1, 9], 1), ([0, 5, 6], 2),
    ([6, 6, 0], 0)])
def test_count_errors(counts, row):
    rows = np.zeros((3, 5), dtype=np.int64)
    for fn in (shardfmt.narrow_rows_numpy, shardfmt.pack_rows):
        with pytest.raises(ValueError) as err:
            fn(rows, counts, "u2")
        if row is None:
            assert f"{len(counts)} counts for 3 rows" in str(err.value)
        else:
            assert f"row {row} has count {counts[row]}" in str(err.value)


def test_argument_errors():
    rows = np.zeros((3, 5), dtype=np.int64)
    counts = [1, 2, 3]
    for bad in ("u8", "i1", "f4", None, "int16"):
        with pytest.raises(ValueError, match="dst_dtype"):
            shardfmt.narrow_rows_numpy(rows, counts, bad)
        with pytest.raises(ValueError, match="dst_dtype"):
            shardfmt.pack_rows(rows, counts, bad)
    with pytest.raises(ValueError, match="exclude each other"):
        shardfmt.pack_rows(rows, counts, "u2", shuffle_elem=2,
                           bitshuffle_elem=2)
    with pytest.raises(ValueError, match="exclude each other"):
        shardfmt.pack_rows_auto(rows, counts, "u2", shuffle_elem=2,
                                bitshuffle_elem=2)
    with pytest.raises(ValueError, match="shuffle_elem=3"):
        shardfmt.pack_rows(rows, counts, "u2", shuffle_elem=3)
    for bad_rows in (np.zeros(5, dtype=np.int64),
                     np.zeros((3, 5), dtype=np.int16),
                     np.zeros((3, 5), dtype=np.float32),
                     np.zeros((1, 3, 5), dtype=np.int32)):
        with pytest.raises(ValueError, match="2-D int32 or int64"):
            shardfmt.narrow_rows_numpy(bad_rows, counts, "u2")


def test_pack_rows_auto_on_the_host_follows_pack_auto():
    rng = np.random.default_rng(15)
    rows = _fitting(rng, "int64", "u2", (8, 100))
    counts = rng.integers(0, 101, 8)
    want, want_start = shardfmt.pack_rows(rows, counts, "u2", block_raw=4096,
                                          shuffle_elem=2)
    # far below the threshold: the CPU writer, whatever the machine has
    got, row_start = shardfmt.pack_rows_auto(rows, counts, "u2",
                                             block_raw=4096, shuffle_elem=2)
    assert got == want and (row_start == want_start).all()
