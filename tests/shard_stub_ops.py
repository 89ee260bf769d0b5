"""CPU stand-ins for the shipyard_amd.ops kernels that decode_device
drives, with the exact tensor contracts of ops.* (a plain helper
module, not a conftest).

The stub is strict where the kernels are trusting: every offset it is
handed must lie inside its tensor and meet the 16-byte rules of the
uint4 paths, so a host-side indexing mistake fails here instead of
reading or writing out of bounds on a device.  ``launches`` counts every
emulated kernel launch; the rejection tests assert it stays 0."""
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


def decode_index(idx, payload: bytes, fake: CpuOps, verify: bool = True):
    """decode_device on a CPU tensor of ``payload`` with the kernels
    replaced by ``fake``.  Returns the decoded tensor."""
    d_comp = torch.frombuffer(bytearray(payload) or bytearray(1),
                              dtype=torch.uint8)
    if not payload:
        d_comp = d_comp[:0]
    with mock.patch("shipyard_amd.ops.gather_copy", fake.gather_copy), \
         mock.patch("shipyard_amd.ops.lz4_decode_blocks",
                    fake.lz4_decode_blocks), \
         mock.patch("shipyard_amd.ops.lz4_all_ok", fake.lz4_all_ok), \
         mock.patch("shipyard_amd.ops.crc32c_chunks", fake.crc32c_chunks):
        return shardfmt.decode_device(d_comp, idx, torch.device("cpu"),
                                      verify=verify)


def decode(packed: bytes, fake: CpuOps, verify: bool = True) -> bytes:
    """read_index + decode_device through the stub ops."""
    idx = shardfmt.read_index(packed)
    out = decode_index(idx, packed[idx.payload_off:], fake, verify=verify)
    return bytes(out.numpy().tobytes())
