"""GPU tests of typed row writes: the ops.compact_narrow kernel against
shardfmt.narrow_rows_numpy (every pair of types, row lengths and row
ends around the 16-byte slot, source rows at every alignment, runs of
empty rows, both ends of the work split, the status word), the
binding's argument rules, and the shardfmt writers on top of it against
the CPU path and the row readers.  Every comparison is exact."""
from unittest import mock

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from shipyard_amd import ops  # noqa: E402
from shipyard_amd.data import shardfmt  # noqa: E402
from shipyard_amd.data.stager import ShardStager  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLEAN = 2 ** 63 - 1
CANARY = 0xA5
MARGIN = 64  # canary bytes on either side of dst
NUMPY = {"u1": "<u1", "u2": "<u2", "i2": "<i2", "u4": "<u4", "i4": "<i4"}
LIMITS = {"u1": (0, 255), "u2": (0, 65535), "i2": (-32768, 32767),
          "u4": (0, 2 ** 32 - 1), "i4": (-2 ** 31, 2 ** 31 - 1)}
PAIRS = [(src, dt) for src in ("int32", "int64") for dt in NUMPY]
# what no destination type but i4-from-int32 (which takes everything)
# holds: around the source, and in its padding columns
POISON = {"int32": -2 ** 31, "int64": 2 ** 40 + 77}


def _pair_id(pair):
    return f"{pair[0]}-{pair[1]}"


def _fitting(rng, src: str, dt: str, shape):
    lo, hi = LIMITS[dt]
    hi = min(hi, np.iinfo(src).max)
    vals = rng.integers(lo, hi + 1, shape, dtype=np.int64)
    flat = vals.reshape(-1)
    if len(flat) >= 2:
        flat[0], flat[-1] = lo, hi
    return vals.astype(src)


def _batch(rng, src: str, dt: str, n: int, T: int, counts):
    """[n, T] rows whose live part fits ``dt`` and whose padding holds
    what ``dt`` cannot."""
    rows = _fitting(rng, src, dt, (n, T))
    live = np.arange(T)[None, :] < np.asarray(counts)[:, None]
    rows[~live] = POISON[src]
    return rows


def _src_view(rows):
    """The batch as a view one element into its allocation, with poison
    in front of it and behind it: a load that strays there changes the
    status word."""
    n, T = rows.shape
    big = torch.full((n * T + 2,), POISON[str(rows.dtype)],
                     dtype=getattr(torch, str(rows.dtype)), device=DEV)
    view = big[1:1 + n * T].view(n, T)
    view.copy_(torch.from_numpy(rows).to(DEV))
    return big, view


def _truncated(rows, counts, dt: str):
    """The stream with every live value cut to its low bytes, and the
    status word: the first stream index that does not fit."""
    n, T = rows.shape
    counts = np.asarray(counts, dtype=np.int64)
    live = np.arange(T)[None, :] < counts[:, None]
    vals = rows[live].astype(np.int64)
    lo, hi = LIMITS[dt]
    bad = np.flatnonzero((vals < lo) | (vals > hi))
    stream = vals.astype(NUMPY[dt]).tobytes()
    row_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    if not len(bad):  # then the reference takes it
        ref, ref_start = shardfmt.narrow_rows_numpy(rows, counts, dt)
        assert ref == stream and (ref_start == row_start).all()
    return stream, row_start, int(bad[0]) if len(bad) else CLEAN


def _narrow_in_canary(rows, counts, dt: str):
    """Run the kernel into a view of exactly total * S bytes inside a
    canary-filled buffer and compare the WHOLE buffer and the status
    word with numpy; the source and what surrounds it stay as they
    were."""
    stream, row_start, want_status = _truncated(rows, counts, dt)
    big_src, src = _src_view(rows)
    before = big_src.clone()
    big = torch.full((2 * MARGIN + len(stream),), CANARY, dtype=torch.uint8,
                     device=DEV)
    dst = big[MARGIN:MARGIN + len(stream)]
    assert dst.data_ptr() % 16 == 0
    status = torch.full((1,), CLEAN, dtype=torch.int64, device=DEV)
    ops.compact_narrow(src, torch.from_numpy(row_start).to(DEV), dst, dt,
                       status)
    torch.cuda.current_stream().synchronize()
    want = np.full(big.numel(), CANARY, dtype=np.uint8)
    want[MARGIN:MARGIN + len(stream)] = np.frombuffer(stream, dtype=np.uint8)
    got = big.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), bad[:8].tolist(), got[bad[:8]].tolist(),
                          want[bad[:8]].tolist())
    assert int(status.item()) == want_status
    assert torch.equal(big_src, before)
    return want_status


def _slot_counts(T: int, rng, repeat: int = 5):
    pool = sorted({c for c in (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, T - 1, T)
                   if 0 <= c <= T})
    return rng.permutation(np.repeat(pool, repeat))


@pytest.mark.parametrize("T", [1, 2, 3, 8, 9, 17, 128, 257])
@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
def test_compact_narrow_against_numpy(pair, T):
    src, dt = pair
    rng = np.random.default_rng(100 * T + len(src) + ord(dt[0]) + int(dt[1]))
    counts = _slot_counts(T, rng)
    rows = _batch(rng, src, dt, len(counts), T, counts)
    assert _narrow_in_canary(rows, counts, dt) == CLEAN


@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
def test_long_rows_at_every_alignment(pair):
    """Rows of 4099 elements: whole wave steps inside one row, an int32
    row only 4-byte aligned (odd T, the view at +1 element), an int64
    row 8-byte aligned, and row ends inside a step."""
    src, dt = pair
    rng = np.random.default_rng(7)
    T = 4099
    counts = np.array([T, T, T - 1, 0, T, 2500, T, 1])
    rows = _batch(rng, src, dt, len(counts), T, counts)
    assert _narrow_in_canary(rows, counts, dt) == CLEAN


@pytest.mark.parametrize("pair", [("int64", "u2"), ("int32", "u1"),
                                  ("int32", "i4"), ("int64", "u4")],
                         ids=_pair_id)
@pytest.mark.parametrize("T", [3, 17, 257])
def test_runs_of_empty_rows(pair, T):
    src, dt = pair
    rng = np.random.default_rng(T)
    for counts in (
            [T] + [0] * 300 + [min(T, 3)],           # longer than a step
            [0, 0, 0, T] + [0] * 300 + [T, T - 1, 0, 0],  # first and last
            [0] * 5 + [1] + [0] * 700 + [2] + [0] * 9):
        counts = np.minimum(counts, T)
        rows = _batch(rng, src, dt, len(counts), T, counts)
        assert _narrow_in_canary(rows, counts, dt) == CLEAN


@pytest.mark.parametrize("pair", [("int64", "u2"), ("int32", "i2")],
                         ids=_pair_id)
def test_all_rows_empty_touches_nothing(pair):
    src, dt = pair
    rows = np.full((40, 9), POISON[src], dtype=src)
    # dst of no bytes between the canaries, status as the caller set it
    assert _narrow_in_canary(rows, [0] * 40, dt) == CLEAN
    status = torch.full((1,), 12345, dtype=torch.int64, device=DEV)
    dst = torch.full((64,), CANARY, dtype=torch.uint8, device=DEV)
    ops.compact_narrow(torch.from_numpy(rows).to(DEV),
                       torch.zeros(41, dtype=torch.int64, device=DEV), dst,
                       dt, status)
    assert int(status.item()) == 12345
    assert (dst == CANARY).all().item()


@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
def test_totals_below_a_slot(pair):
    src, dt = pair
    rng = np.random.default_rng(9)
    rows = _batch(rng, src, dt, 1, 1, [1])  # n = 1, T = 1
    assert _narrow_in_canary(rows, [1], dt) == CLEAN
    counts = [1, 0, 2]  # three elements: no whole slot for any type
    rows = _batch(rng, src, dt, 3, 2, counts)
    assert _narrow_in_canary(rows, counts, dt) == CLEAN


@pytest.mark.parametrize("pair", [("int64", "u2"), ("int32", "u4"),
                                  ("int64", "u1")], ids=_pair_id)
def test_fewer_steps_than_waves(pair):
    """About 600 KiB of u2: some hundred steps for the 8192 waves of the
    fixed grid, most of which find nothing to do."""
    src, dt = pair
    rng = np.random.default_rng(10)
    n, T = 300, 1030
    counts = rng.integers(T - 40, T + 1, n)
    counts[::37] = 0
    rows = _batch(rng, src, dt, n, T, counts)
    assert _narrow_in_canary(rows, counts, dt) == CLEAN


def test_24_mib_stream_every_wave_takes_several_steps():
    """12.6 M int32 -> u2: 24 MiB of stream, 24 K steps, three for each
    wave, the last wave's run cut short by the end of the stream."""
    src, dt = "int32", "u2"
    rng = np.random.default_rng(11)
    n, T = 3150, 4099
    counts = rng.integers(T - 64, T + 1, n)
    counts[::101] = rng.integers(0, 17, len(counts[::101]))
    rows = _batch(rng, src, dt, n, T, counts)
    total = int(counts.sum())
    assert 24 << 20 <= total * 2 < 26 << 20 and total * 2 % 16
    assert _narrow_in_canary(rows, counts, dt) == CLEAN


def _status_batch(src="int64", dt="u2"):
    """64 full rows of 4096: 262144 elements, 512 steps of u2, each in
    a wave of its own."""
    rng = np.random.default_rng(12)
    n, T = 64, 4096
    counts = np.full(n, T)
    counts[5] = T - 3  # padding to hide a misfit in
    return _batch(rng, src, dt, n, T, counts), counts


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("pair", [("int64", "u2"), ("int32", "u2"),
                                  ("int64", "i4"), ("int32", "u4")],
                         ids=_pair_id)
def test_status_one_misfit(pair, where):
    src, dt = pair
    rows, counts = _status_batch(src, dt)
    r, c = {"first": (0, 0), "middle": (31, 1234),
            "last": (63, 4095)}[where]
    rows[r, c] = -1 if src == "int32" else LIMITS[dt][1] + 1
    row_start = np.concatenate(([0], np.cumsum(counts)))
    assert _narrow_in_canary(rows, counts, dt) == int(row_start[r]) + c


def test_status_two_misfits_in_different_waves_report_the_smaller():
    rows, counts = _status_batch()
    rows[50, 7] = 65536
    rows[9, 4000] = -1
    row_start = np.concatenate(([0], np.cumsum(counts)))
    assert _narrow_in_canary(rows, counts, "u2") == int(row_start[9]) + 4000
    rows[9, 4000] = 5
    assert _narrow_in_canary(rows, counts, "u2") == int(row_start[50]) + 7


def test_status_ignores_the_padding():
    rows, counts = _status_batch()
    assert (rows[5, -3:] == POISON["int64"]).all()
    assert _narrow_in_canary(rows, counts, "u2") == CLEAN
    rows[5, -3:] = (-100, 65536, -1)
    assert _narrow_in_canary(rows, counts, "u2") == CLEAN


def test_binding_rejections():
    n, T = 6, 10
    src = torch.zeros((n, T), dtype=torch.int64, device=DEV)
    row_start = torch.arange(n + 1, dtype=torch.int64, device=DEV) * T
    big = torch.full((1024 + 16,), CANARY, dtype=torch.uint8, device=DEV)
    dst = big[:1024]
    status = torch.full((1,), CLEAN, dtype=torch.int64, device=DEV)
    good = dict(src=src, row_start=row_start, dst=dst, dst_dtype="u2",
                status=status)
    cpu = torch.device("cpu")
    bad = [
        dict(src=src.to(torch.int16)), dict(src=src.to(torch.float32)),
        dict(src=src.view(-1)), dict(src=src[:, ::2]), dict(src=src.t()),
        dict(src=src.to(cpu)),
        dict(dst_dtype="u8"), dict(dst_dtype="i1"), dict(dst_dtype=None),
        dict(row_start=row_start.to(torch.int32)),
        dict(row_start=row_start.view(1, -1)),
        dict(row_start=torch.arange(2 * (n + 1), dtype=torch.int64,
                                    device=DEV)[::2]),
        dict(row_start=row_start[:-1]),
        dict(row_start=torch.cat([row_start, row_start[-1:]])),
        dict(row_start=row_start.to(cpu)),
        dict(dst=dst.view(torch.int8)), dict(dst=big[::2][:512]),
        dict(dst=dst.to(cpu)), dict(dst=big[1:1025]), dict(dst=big[8:1032]),
        dict(status=status.to(torch.int32)),
        dict(status=torch.full((2,), CLEAN, dtype=torch.int64, device=DEV)),
        dict(status=status.to(cpu)),
    ]
    for change in bad:
        with pytest.raises(ValueError):
            ops.compact_narrow(**{**good, **change})
    # the row length limit, without a row that long
    with mock.patch.object(ops, "WIDEN_MAX_ROW_ELEMS", T - 1):
        with pytest.raises(ValueError, match=f"at most {T - 1} elements"):
            ops.compact_narrow(**good)
    torch.cuda.synchronize()
    assert int(status.item()) == CLEAN
    assert (big == CANARY).all().item()
    # no rows, or rows of no elements: a no-op without a launch
    with mock.patch("shipyard_amd.ops._call",
                    side_effect=AssertionError("launched")):
        ops.compact_narrow(src[:0], row_start[:1], dst, "u2", status)
        ops.compact_narrow(src[:, :0].contiguous(), row_start, dst, "u2",
                           status)
    assert (big == CANARY).all().item()


# ------------------------------------------------------------ shardfmt
def _tokens(n=40, T=333, dt="u2", src="int64", pad=-100, seed=20):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, T + 1, n)
    counts[:4] = (T, 0, 1, T - 1)
    rows = _fitting(rng, src, dt, (n, T))
    rows[np.arange(T)[None, :] >= counts[:, None]] = pad
    return rows, counts


@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
def test_narrow_rows_device_equals_numpy(pair):
    src, dt = pair
    rows, counts = _tokens(dt=dt, src=src)
    want, want_start = shardfmt.narrow_rows_numpy(rows, counts, dt)
    d_rows = torch.from_numpy(rows).to(DEV)
    for c in (counts.tolist(), counts, torch.from_numpy(counts).to(DEV)):
        got, row_start = shardfmt.narrow_rows_device(d_rows, c, dt)
        assert got.dtype == torch.uint8 and got.is_cuda
        assert got.cpu().numpy().tobytes() == want
        assert isinstance(row_start, np.ndarray)
        assert row_start.dtype == np.int64
        assert (row_start == want_start).all()


def test_narrow_rows_device_empty_and_errors():
    rows = torch.full((3, 5), -100, dtype=torch.int64, device=DEV)
    got, row_start = shardfmt.narrow_rows_device(rows, [0, 0, 0], "u2")
    assert got.numel() == 0 and row_start.tolist() == [0, 0, 0, 0]
    got, row_start = shardfmt.narrow_rows_device(rows[:0], [], "u2")
    assert got.numel() == 0 and row_start.tolist() == [0]
    with pytest.raises(ValueError, match="2 counts for 3 rows"):
        shardfmt.narrow_rows_device(rows, [1, 1], "u2")
    with pytest.raises(ValueError, match="row 1 has count 6"):
        shardfmt.narrow_rows_device(rows, [1, 6, 0], "u2")
    with pytest.raises(ValueError, match="row 2 has count -1"):
        shardfmt.narrow_rows_device(
            rows, torch.tensor([1, 5, -1], device=DEV), "u2")
    with pytest.raises(ValueError, match="dst_dtype"):
        shardfmt.narrow_rows_device(rows, [0, 0, 0], "u3")
    with pytest.raises(ValueError, match="not on a GPU"):
        shardfmt.narrow_rows_device(rows.cpu(), [0, 0, 0], "u2")


@pytest.mark.parametrize("pair", [("int64", "u2"), ("int32", "u4"),
                                  ("int64", "i4"), ("int32", "u1")],
                         ids=_pair_id)
def test_misfit_message_is_the_cpu_path_s(pair):
    src, dt = pair
    rows, counts = _tokens(dt=dt, src=src)
    rows[7, :3] = 0  # live below
    rows[7, 2] = -1 if src == "int32" else LIMITS[dt][0] - 1
    rows[20, 0] = -1 if src == "int32" else LIMITS[dt][1] + 1
    counts[7], counts[20] = max(counts[7], 3), max(counts[20], 1)
    with pytest.raises(ValueError) as cpu:
        shardfmt.narrow_rows_numpy(rows, counts, dt)
    assert "row 7, column 2 holds" in str(cpu.value)
    with pytest.raises(ValueError) as gpu:
        shardfmt.narrow_rows_device(torch.from_numpy(rows).to(DEV), counts,
                                    dt)
    assert str(gpu.value) == str(cpu.value)
    with pytest.raises(ValueError) as packed:
        shardfmt.pack_rows_gpu(torch.from_numpy(rows).to(DEV), counts, dt)
    assert str(packed.value) == str(cpu.value)


FILTERS = [dict(), dict(shuffle_elem=2), dict(delta_elem=4,
                                               bitshuffle_elem=4)]


@pytest.mark.parametrize("filt", FILTERS,
                         ids=["plain", "shuffle", "delta-bit"])
def test_pack_rows_gpu_round_trip(filt, tmp_path):
    T, pad, dt = 333, -100, "u2"
    rows, counts = _tokens(n=80, T=T, dt=dt, pad=pad)
    d_rows = torch.from_numpy(rows).to(DEV)
    shard, row_start = shardfmt.pack_rows_gpu(d_rows, counts, dt,
                                              block_raw=4096, **filt)
    stream, want_start = shardfmt.narrow_rows_numpy(rows, counts, dt)
    assert (row_start == want_start).all()
    assert shard == shardfmt.pack_gpu(stream, block_raw=4096, **filt)
    assert len(stream) > 4 * 4096 and len(stream) % 4096
    starts, lens = row_start[:-1], np.diff(row_start)
    # the row readers give the batch back
    idx = shardfmt.read_index(shard)
    d_comp = torch.frombuffer(bytearray(shard[idx.payload_off:]),
                              dtype=torch.uint8).to(DEV)
    got = shardfmt.decode_rows_device(d_comp, idx, starts, lens, DEV, dt,
                                      torch.int64, T, pad)
    assert torch.equal(got, d_rows)
    path = tmp_path / "tokens.syshard"
    path.write_bytes(shard)
    got, res = ShardStager(staging_mb=1, verify=True).stage_rows(
        path, starts, lens, dt, torch.int64, T, pad)
    assert torch.equal(got, d_rows)
    assert res.raw_bytes == len(stream)
    assert (shardfmt.read_rows_cpu(shard, starts, lens, dt, "int64", T, pad)
            == rows).all()


def test_pack_rows_gpu_int32_batch_and_bad_block_raw():
    rows, counts = _tokens(n=30, T=200, dt="i2", src="int32", pad=0)
    d_rows = torch.from_numpy(rows).to(DEV)
    shard, row_start = shardfmt.pack_rows_gpu(d_rows, counts, "i2",
                                              block_raw=4096, shuffle_elem=2)
    idx = shardfmt.read_index(shard)
    d_comp = torch.frombuffer(bytearray(shard[idx.payload_off:]),
                              dtype=torch.uint8).to(DEV)
    got = shardfmt.decode_rows_device(d_comp, idx, row_start[:-1],
                                      np.diff(row_start), DEV, "i2",
                                      torch.int32, 200, 0)
    assert torch.equal(got, d_rows)
    with mock.patch("shipyard_amd.ops._call",
                    side_effect=AssertionError("launched")):
        with pytest.raises(ValueError, match="block_raw=1000"):
            shardfmt.pack_rows_gpu(d_rows, counts, "i2", block_raw=1000)
        with pytest.raises(ValueError, match="exclude each other"):
            shardfmt.pack_rows_gpu(d_rows, counts, "i2", shuffle_elem=2,
                                   bitshuffle_elem=2)


def test_pack_rows_auto_picks_its_writer():
    rows, counts = _tokens(n=30, T=200)
    d_rows = torch.from_numpy(rows).to(DEV)
    want_gpu = shardfmt.pack_rows_gpu(d_rows, counts, "u2", block_raw=4096,
                                      shuffle_elem=2)[0]
    want_cpu = shardfmt.pack_rows(rows, counts, "u2", block_raw=4096,
                                  shuffle_elem=2)[0]
    real_gpu, real_cpu = shardfmt.pack_gpu, shardfmt.pack
    with mock.patch.object(shardfmt, "pack_gpu", side_effect=real_gpu) as g, \
            mock.patch.object(shardfmt, "pack", side_effect=real_cpu) as c:
        # a CUDA tensor: the GPU, however small
        got, _ = shardfmt.pack_rows_auto(d_rows, counts, "u2",
                                         block_raw=4096, shuffle_elem=2)
        assert got == want_gpu and g.call_count == 1 and c.call_count == 0
        # a host batch below the threshold: the CPU
        got, _ = shardfmt.pack_rows_auto(rows, counts, "u2", block_raw=4096,
                                         shuffle_elem=2)
        assert got == want_cpu and g.call_count == 1 and c.call_count == 1
        # a host batch whose stream reaches it: the GPU writer
        got, _ = shardfmt.pack_rows_auto(rows, counts, "u2", block_raw=4096,
                                         shuffle_elem=2, gpu_threshold=1024)
        assert got == want_gpu and g.call_count == 2 and c.call_count == 1
        # a CUDA tensor and a block size the GPU writer does not take
        got, row_start = shardfmt.pack_rows_auto(d_rows, counts, "u2",
                                                 block_raw=1000)
        assert g.call_count == 2 and c.call_count == 2
    assert got == shardfmt.pack_rows(rows, counts, "u2", block_raw=1000)[0]
