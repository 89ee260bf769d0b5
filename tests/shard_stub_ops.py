"""CPU stand-ins for the shipyard_amd.ops kernels that decode_device
drives, with the exact tensor contracts of ops.* (a plain helper
module, not a conftest).

The stub is strict where the kernels are trusting: every offset it is
handed must lie inside its tensor and meet the 16-byte rules of the
uint4 paths, so a host-side indexing mistake fails here instead of
reading or writing out of bounds on a device.  ``launches`` counts every
emulated kernel launch; the rejection tests assert it stays 0.
``FilterOps`` adds the two filter kernels, ops.byte_shuffle and
ops.delta_filter, to ``CpuOps``."""
import contextlib
from unittest import mock

import torch

from shipyard_amd.data import lz4py, shardfmt
from shipyard_amd.ops import gf2


class CpuOps:
    """Kernel emulation with the exact tensor contracts of ops.*"""

    def __init__(self):
        self.calls = []

    @property
    def launches(self) -> int:
        return len(self.calls)

    def gather_copy(self, src, soff, dst, doff, lens):
        assert soff.dtype == torch.int64 and doff.dtype == torch.int64
        assert lens.dtype == torch.uint32
        self.calls.append(("gather", soff.numel()))
        for s, d, l in zip(soff.tolist(), doff.tolist(),
                           lens.view(torch.int32).tolist()):
            assert s % 16 == 0 and d % 16 == 0, (s, d)
            assert 0 <= s and 0 < l and s + l <= src.numel(), (s, l)
            assert 0 <= d and d + l <= dst.numel(), (d, l)
            dst[d:d + l] = src[s:s + l]

    def lz4_decode_blocks(self, comp, ioff, ilen, out, ooff, olen,
                          raw_cap):
        assert ioff.dtype == torch.int64 and ooff.dtype == torch.int64
        assert ilen.dtype == torch.uint32 and olen.dtype == torch.uint32
        assert raw_cap <= 65536
        self.calls.append(("lz4", ioff.numel()))
        cb = bytes(comp.numpy().tobytes())
        for io_, il, oo, ol in zip(
                ioff.tolist(), ilen.view(torch.int32).tolist(),
                ooff.tolist(), olen.view(torch.int32).tolist()):
            assert oo % 16 == 0, oo
            assert 0 <= io_ and 0 < il and io_ + il <= len(cb), (io_, il)
            assert 0 <= oo and 0 < ol <= raw_cap, (oo, ol)
            assert oo + ol <= out.numel(), (oo, ol)
            raw = lz4py.decompress_block(cb[io_:io_ + il], ol)
            out[oo:oo + ol] = torch.frombuffer(bytearray(raw),
                                               dtype=torch.uint8)
        return torch.zeros(ioff.numel(), dtype=torch.uint32)

    @staticmethod
    def lz4_all_ok(status):
        return True

    def crc32c_chunks(self, t, chunk_size, n_chains=None):
        assert chunk_size % 4096 == 0, chunk_size
        self.calls.append(("crc", t.numel()))
        b = bytes(t.numpy().tobytes())
        return torch.tensor(
            [gf2.crc32c(b[i:i + chunk_size])
             for i in range(0, len(b), chunk_size)],
            dtype=torch.int64).to(torch.uint32)


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
    """CpuOps plus strict stand-ins for the two filter kernels: uint8,
    equal sizes, 16-byte-aligned bases, 4 KiB block geometry, the
    element sizes, and the aliasing rules (byte_shuffle never in place;
    delta_filter either exactly in place or disjoint)."""

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


def patched_ops(fake: CpuOps):
    """Context manager: every shipyard_amd.ops kernel that ``fake``
    emulates is replaced by its emulation."""
    stack = contextlib.ExitStack()
    for name in ("gather_copy", "lz4_decode_blocks", "lz4_all_ok",
                 "crc32c_chunks", "byte_shuffle", "delta_filter"):
        if hasattr(fake, name):
            stack.enter_context(mock.patch(f"shipyard_amd.ops.{name}",
                                           getattr(fake, name)))
    return stack


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


def decode_index_aligned(idx, payload: bytes, fake: FilterOps,
                         verify: bool = True):
    """decode_device on an aligned CPU tensor of ``payload`` with every
    kernel replaced by ``fake``.  Returns (output tensor, payload
    tensor)."""
    d_comp = aligned_tensor(payload)
    with patched_ops(fake):
        out = shardfmt.decode_device(d_comp, idx, torch.device("cpu"),
                                     verify=verify)
    return out, d_comp


def decode_packed(packed: bytes, fake: FilterOps, verify: bool = True):
    """read_index + decode_index_aligned."""
    idx = shardfmt.read_index(packed)
    return decode_index_aligned(idx, packed[idx.payload_off:], fake, verify)


def decode_index(idx, payload: bytes, fake: CpuOps, verify: bool = True):
    """decode_device on a CPU tensor of ``payload`` with the kernels
    replaced by ``fake``.  Returns the decoded tensor."""
    d_comp = torch.frombuffer(bytearray(payload) or bytearray(1),
                              dtype=torch.uint8)
    if not payload:
        d_comp = d_comp[:0]
    with patched_ops(fake):
        return shardfmt.decode_device(d_comp, idx, torch.device("cpu"),
                                      verify=verify)


def decode(packed: bytes, fake: CpuOps, verify: bool = True) -> bytes:
    """read_index + decode_device through the stub ops."""
    idx = shardfmt.read_index(packed)
    out = decode_index(idx, packed[idx.payload_off:], fake, verify=verify)
    return bytes(out.numpy().tobytes())
