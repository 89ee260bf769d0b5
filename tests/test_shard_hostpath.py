"""CPU coverage of the vectorized shard-decode host path: the batching
logic of decode_device (numpy index columns, gather/LZ4 split, offsets,
CRC compare) exercised against stub ops that emulate the kernels on
CPU.  The GPU numerics themselves are covered by tests/test_shard_gpu
(-m gpu); this pins the host-side orchestration on every CPU run."""
import os
import random
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from shard_stub_ops import CpuOps, decode as _decode  # noqa: E402

from shipyard_amd.data import shardfmt  # noqa: E402


def test_mixed_stored_and_lz4_blocks():
    random.seed(3)
    data = (b"compressible text " * 4000 + os.urandom(70_000)
            + bytes(random.choices(b"xyz01", k=30_000)))
    packed = shardfmt.pack(data, block_raw=8192)
    idx = shardfmt.read_index(packed)
    stored = int((idx.table["comp_len"] == idx.table["raw_len"]).sum())
    assert 0 < stored < idx.n_blocks  # genuinely mixed
    fake = CpuOps()
    assert _decode(packed, fake) == data
    kinds = dict(fake.calls)
    assert kinds["gather"] == stored
    assert kinds["lz4"] == idx.n_blocks - stored


def test_corruption_detected_via_vector_compare():
    data = b"all work and no play " * 8000
    packed = bytearray(shardfmt.pack(data, block_raw=8192))
    idx = shardfmt.read_index(bytes(packed))
    packed[idx.payload_off + 5] ^= 0x7F
    with pytest.raises(ValueError, match="CRC mismatch"):
        _decode(bytes(packed), CpuOps())


def test_single_block_and_empty():
    fake = CpuOps()
    assert _decode(shardfmt.pack(b""), fake) == b""
    small = b"tiny payload " * 10
    assert _decode(shardfmt.pack(small), fake) == small


def test_index_parse_scales():
    """131k-block index parses in milliseconds (was a python loop)."""
    import time

    import numpy as np

    n = 131072
    table = np.zeros(n, dtype=shardfmt._entry_dt())
    table["comp_len"] = 4096
    table["raw_len"] = 4096
    table["comp_off"] = np.arange(n, dtype=np.uint64) * 4096
    buf = shardfmt.HEADER.pack(shardfmt.MAGIC, 1, 4096, n * 4096, n) + \
        table.tobytes()
    t0 = time.perf_counter()
    idx = shardfmt.read_index(buf)
    idx.raw_offs()
    assert shardfmt._stored_contiguous(idx)
    assert (time.perf_counter() - t0) < 0.25
    assert idx.n_blocks == n


def test_pack_auto_cpu_fallback_roundtrip():
    """pack_auto on a no-GPU host routes to the CPU writer and the
    result round-trips (the GPU path is covered by gpu-marked
    tests)."""
    import torch

    from shipyard_amd.data import shardfmt

    data = (b"roundtrip payload " * 9000) + bytes(range(256)) * 16
    blob = shardfmt.pack_auto(data, gpu_threshold=1 << 20)
    assert shardfmt.unpack_cpu(blob) == data
    if not torch.cuda.is_available():
        # small payloads and CPU hosts take the identical CPU path
        assert blob == shardfmt.pack(data)
