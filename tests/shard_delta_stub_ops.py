"""CpuOps (tests/shard_stub_ops) plus strict CPU stand-ins for the two
filter kernels that decode_device drives, ops.byte_shuffle and
ops.delta_filter (a plain helper module, not a conftest).

Like the base class the stand-ins assert what the kernels trust: uint8,
equal sizes, 16-byte-aligned bases, 4 KiB block geometry, the element
sizes, and the aliasing rules (byte_shuffle never in place; delta_filter
either exactly in place or disjoint)."""
from unittest import mock

import torch

from shard_stub_ops import CpuOps

from shipyard_amd.data import shardfmt


def _check_pair(src, dst, block_raw, elem_size):
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8
    assert src.is_contiguous() and dst.is_contiguous()
    assert src.numel() == dst.numel()
    assert src.data_ptr() % 16 == 0, "src base not 16-byte aligned"
    assert dst.data_ptr() % 16 == 0, "dst base not 16-byte aligned"
    assert 0 < block_raw < (1 << 32) and block_raw % 4096 == 0, block_raw
    assert elem_size in (2, 4, 8), elem_size


def _disjoint(src, dst) -> bool:
    s0, d0, n = src.data_ptr(), dst.data_ptr(), src.numel()
    return s0 + n <= d0 or d0 + n <= s0


class FilterOps(CpuOps):
    def byte_shuffle(self, src, dst, block_raw, elem_size, inverse=False):
        _check_pair(src, dst, block_raw, elem_size)
        assert _disjoint(src, dst), "byte_shuffle cannot alias"
        self.calls.append(("shuffle", src.numel()))
        out = shardfmt.shuffle_blocks_numpy(
            bytes(src.numpy().tobytes()), block_raw, elem_size, inverse)
        dst.copy_(torch.frombuffer(bytearray(out), dtype=torch.uint8))

    def delta_filter(self, src, dst, block_raw, elem_size, inverse=False):
        _check_pair(src, dst, block_raw, elem_size)
        in_place = src.data_ptr() == dst.data_ptr()
        assert in_place or _disjoint(src, dst), "partial overlap"
        self.calls.append(("delta-inplace" if in_place else "delta",
                           src.numel()))
        out = shardfmt.delta_blocks_numpy(
            bytes(src.numpy().tobytes()), block_raw, elem_size, inverse)
        dst.copy_(torch.frombuffer(bytearray(out), dtype=torch.uint8))


def aligned_tensor(payload: bytes):
    """uint8 CPU tensor of ``payload`` whose base is 16-byte aligned
    (what a device allocation guarantees)."""
    n = len(payload)
    buf = torch.empty(n + 16, dtype=torch.uint8)
    lo = (-buf.data_ptr()) % 16
    t = buf[lo:lo + n]
    if n:
        t.copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
    return t


def decode_packed(packed: bytes, fake: FilterOps, verify: bool = True):
    """read_index + decode_device on an aligned CPU tensor with every
    kernel replaced by ``fake``.  Returns (output tensor, payload
    tensor)."""
    idx = shardfmt.read_index(packed)
    return decode_index(idx, packed[idx.payload_off:], fake, verify)


def decode_index(idx, payload: bytes, fake: FilterOps, verify: bool = True):
    d_comp = aligned_tensor(payload)
    with mock.patch("shipyard_amd.ops.gather_copy", fake.gather_copy), \
         mock.patch("shipyard_amd.ops.lz4_decode_blocks",
                    fake.lz4_decode_blocks), \
         mock.patch("shipyard_amd.ops.lz4_all_ok", fake.lz4_all_ok), \
         mock.patch("shipyard_amd.ops.crc32c_chunks", fake.crc32c_chunks), \
         mock.patch("shipyard_amd.ops.byte_shuffle", fake.byte_shuffle), \
         mock.patch("shipyard_amd.ops.delta_filter", fake.delta_filter):
        out = shardfmt.decode_device(d_comp, idx, torch.device("cpu"),
                                     verify=verify)
    return out, d_comp
