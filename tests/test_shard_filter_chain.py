"""The SYSHARD filter chains on the device side, through strict CPU stub
ops: the writer chain (pack_gpu's) applies delta then shuffle, each
into a new tensor, and leaves its input alone; the reader chain
(decode_device's) undoes them in reverse, in place only where the
filter allows it and the source is not the caller's payload."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from shard_stub_ops import (FilterOps, aligned_tensor,  # noqa: E402
                            patched_ops)

from shipyard_amd.data import shardfmt  # noqa: E402

B = 4096
N = 2 * B + 1001  # two full blocks and a ragged one


def _bytes(t) -> bytes:
    return bytes(t.numpy().tobytes())


def _apart(a, b) -> bool:
    return a.data_ptr() + a.numel() <= b.data_ptr() or \
        b.data_ptr() + b.numel() <= a.data_ptr()


# (delta, shuffle), the writer's launches, the reader's launches from a
# tensor of its own, the reader's launches from a borrowed payload
CASES = [
    (8, 0, ["delta"], ["delta-inplace"], ["delta"]),
    (0, 4, ["shuffle"], ["shuffle"], ["shuffle"]),
    (8, 2, ["delta", "shuffle"], ["shuffle", "delta-inplace"],
     ["shuffle", "delta-inplace"]),
]


@pytest.mark.parametrize("D,S,wrote,unwound,unwound_borrowed", CASES,
                         ids=["delta8", "shuffle4", "delta8+shuffle2"])
def test_device_chains(D, S, wrote, unwound, unwound_borrowed):
    x = np.random.default_rng(16 * D + S).integers(
        0, 256, N, dtype=np.uint8).tobytes()
    elems = {"delta_elem": D, "shuffle_elem": S}
    t = aligned_tensor(x)

    fake = FilterOps()
    with patched_ops(fake):
        flt = shardfmt.filter_chain_device(t, B, elems)
    # delta first, then shuffle; "delta-inplace" would be an in-place call
    assert [k for k, _ in fake.calls] == wrote
    assert all(n == N for _, n in fake.calls)
    assert _bytes(t) == x and _apart(t, flt)  # the input is left alone
    want = shardfmt.filter_chain_numpy(x, B, elems)
    assert want != x and _bytes(flt) == want

    # reader, source borrowed: the first step must not write to it
    fake = FilterOps()
    with patched_ops(fake):
        out = shardfmt.unfilter_chain_device(flt, B, elems, borrowed=True)
    assert [k for k, _ in fake.calls] == unwound_borrowed
    assert _bytes(out) == x
    assert _bytes(flt) == want and _apart(flt, out)

    # reader, source its own (the decode target): in place where allowed
    fake = FilterOps()
    with patched_ops(fake):
        out = shardfmt.unfilter_chain_device(flt, B, elems, borrowed=False)
    assert [k for k, _ in fake.calls] == unwound
    assert _bytes(out) == x
    assert (out.data_ptr() == flt.data_ptr()) == (unwound == ["delta-inplace"])
