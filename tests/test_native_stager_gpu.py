"""GPU test: native C++ staging pipeline (sy_stage_file)."""
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from shipyard_amd import ops  # noqa: E402


@pytest.mark.parametrize("direct", [True, False], ids=["odirect", "buffered"])
def test_stage_file_native_roundtrip(tmp_path, direct):
    data = random.Random(31).randbytes(7 * (1 << 20) + 12345)
    src = tmp_path / "blob.bin"
    src.write_bytes(data)
    dst = torch.zeros(len(data), dtype=torch.uint8, device="cuda:0")
    secs = ops.stage_file_native(src, dst, staging_mb=2, use_direct=direct)
    torch.cuda.synchronize()
    assert secs > 0
    assert bytes(dst.cpu().numpy().tobytes()) == data


def test_stage_file_native_offset(tmp_path):
    data = random.Random(32).randbytes(1 << 20)
    src = tmp_path / "blob.bin"
    src.write_bytes(data)
    n = 300_000
    off = 4096
    dst = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    ops.stage_file_native(src, dst, file_off=off, n_bytes=n, staging_mb=1)
    torch.cuda.synchronize()
    assert bytes(dst.cpu().numpy().tobytes()) == data[off:off + n]


def test_stage_file_native_missing_file(tmp_path):
    dst = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError):
        ops.stage_file_native(tmp_path / "nope.bin", dst, n_bytes=16)


# ------------------------------------------------- staging-window edges
MIB = 1 << 20
GUARD = 0xA5
SLACK = 8192   # guard bytes behind n_bytes: two 4 KiB O_DIRECT round-ups


@pytest.fixture(scope="module")
def blob():
    return random.Random(33).randbytes(4 * MIB + 12345)


def _stage_guarded(path, n, **kw):
    """Stage into a GUARD-filled tensor of n + SLACK bytes; returns the
    staged payload after asserting every byte behind it is untouched
    (the pipeline may over-read the FILE into its pinned ring, but only
    n bytes may reach the device)."""
    dst = torch.full((n + SLACK,), GUARD, dtype=torch.uint8,
                     device="cuda:0")
    ops.stage_file_native(path, dst, n_bytes=n, **kw)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    bad = np.nonzero(host[n:] != GUARD)[0]
    assert bad.size == 0, "guard byte %d behind n_bytes overwritten" % bad[0]
    return bytes(host[:n].tobytes())


@pytest.mark.parametrize("direct", [True, False], ids=["odirect", "buffered"])
@pytest.mark.parametrize("n", [1, 4095, 4096, MIB - 1, MIB, MIB + 1,
                               2 * MIB, 3 * MIB + 12345])
def test_stage_file_native_window_edges(tmp_path, blob, n, direct):
    """File lengths around the 1 MiB staging window and the 4 KiB
    O_DIRECT granule; the file ends where the request ends."""
    src = tmp_path / "edge.bin"
    src.write_bytes(blob[:n])
    got = _stage_guarded(src, n, staging_mb=1, use_direct=direct)
    assert got == blob[:n]


@pytest.mark.parametrize("direct", [True, False], ids=["odirect", "buffered"])
@pytest.mark.parametrize("n", [5000, MIB + 5000, 2 * MIB - 1])
def test_stage_file_native_subrange_inside_longer_file(tmp_path, blob, n,
                                                       direct):
    """file_off=4096 keeps O_DIRECT on; n is no 4 KiB multiple and the
    file goes on behind the range, so the rounded-up reads really bring
    bytes past n_bytes into the ring."""
    src = tmp_path / "long.bin"
    src.write_bytes(blob)
    got = _stage_guarded(src, n, file_off=4096, staging_mb=1,
                         use_direct=direct)
    assert got == blob[4096:4096 + n]


@pytest.mark.parametrize("off", [1, 4097, MIB + 511])
def test_stage_file_native_unaligned_offset(tmp_path, blob, off):
    src = tmp_path / "long.bin"
    src.write_bytes(blob)
    n = MIB + 300_001
    got = _stage_guarded(src, n, file_off=off, staging_mb=1,
                         use_direct=True)
    assert got == blob[off:off + n]


@pytest.mark.parametrize("direct", [True, False], ids=["odirect", "buffered"])
def test_stage_file_native_short_file_then_good_call(tmp_path, blob,
                                                     direct):
    """The file ends inside the second window: the first window's copy
    is already queued when the short read is found.  The call raises,
    and the pinned ring is safe to reuse by the next call."""
    have = MIB + 100
    src = tmp_path / "short.bin"
    src.write_bytes(blob[:have])
    want = 2 * MIB + 5
    dst = torch.full((want,), GUARD, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError):
        ops.stage_file_native(src, dst, n_bytes=want, staging_mb=1,
                              use_direct=direct)
    with pytest.raises(RuntimeError):  # range starts behind EOF
        ops.stage_file_native(src, dst, file_off=2 * MIB, n_bytes=4096,
                              staging_mb=1, use_direct=direct)
    torch.cuda.synchronize()
    # the failed call drained its stream before returning: the first
    # window is in place, nothing behind it was written
    host = dst.cpu().numpy()
    assert bytes(host[:MIB].tobytes()) == blob[:MIB]
    assert (host[MIB:] == GUARD).all()
    good = tmp_path / "good.bin"
    good.write_bytes(blob[MIB:3 * MIB + 7])
    got = _stage_guarded(good, 2 * MIB + 7, staging_mb=1,
                         use_direct=direct)
    assert got == blob[MIB:3 * MIB + 7]


@pytest.mark.parametrize("direct", [True, False], ids=["odirect", "buffered"])
def test_stage_file_native_ring_grows_then_is_reused(tmp_path, blob,
                                                     direct):
    src = tmp_path / "ring.bin"
    src.write_bytes(blob)
    n = 3 * MIB + 12345
    for staging_mb in (1, 4, 1):
        got = _stage_guarded(src, n, staging_mb=staging_mb,
                             use_direct=direct)
        assert got == blob[:n], staging_mb
