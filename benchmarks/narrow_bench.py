#!/usr/bin/env python3
"""Typed row writes on the MI355X: the compact_narrow kernel.

ops.compact_narrow in four cases, the row reader's mirrored.  GB/s
counts the source bytes of the live elements plus the stream bytes
written; each figure is the median, after a warm-up, of device-event
timings of windows of 10 back-to-back calls.  The content is random
values that fit the destination type.
(a) 32768 rows of 4096 int64 -> u2, full rows;
(b) the same with counts uniform in 0..4096;
(c) 131072 rows of T = 128 int32 -> u2, counts uniform in 0..128;
(d) 32768 rows of 4096 int32 -> i4, full rows: a plain compaction.
Next to each case, the same stream made by the composed torch path: a
mask built from the counts, boolean indexing (which synchronises with
the host to learn the size of its result) and a narrowing ``.to`` whose
bytes equal the unsigned type's.  Its bytes are counted like the
kernel's (what the result needs, not what the passes move), and its
result is compared with the kernel's.  ``dst.copy_(src)`` with the total
traffic of (a), 1.25 GiB, and of (d), 1 GiB, is timed before and after
the kernels.

Prints one line per measurement and a final JSON line with all of them.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
from shipyard_amd import ops  # noqa: E402

INNER = 10  # launches per timed window: a lone 0.1 ms launch shows its
#             enqueue gap in the event interval
CLEAN = (1 << 63) - 1
# the torch type whose low bytes are the destination type's
TORCH_NARROW = {"u2": torch.int16, "i4": torch.int32}
SIZE = {"u2": 2, "i4": 4}
LIMIT = {"u2": 1 << 16, "i4": (1 << 31) - 1}


def _median_ms(fn, warmup: int, reps: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(INNER):
            fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) / INNER)
    return statistics.median(times)


def _composed(src, counts, dst_dtype):
    cols = torch.arange(src.shape[1], device=src.device)
    live = cols[None, :] < counts[:, None]
    return src[live].to(TORCH_NARROW[dst_dtype]).view(torch.uint8)


def kernel_rates(scale: int, warmup: int, reps: int) -> list:
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    rng = np.random.default_rng(1)
    rows = []

    def row(name, ms, moved, **kw):
        r = dict(name=name, ms=round(ms, 4), bytes=moved,
                 gbps=round(moved / ms / 1e6, 1), **kw)
        rows.append(r)
        print(f"{name:50s} {r['ms']:8.4f} ms  {r['gbps']:8.1f} GB/s "
              "(read+write)")

    def copies(tag):
        for mib in (640, 512):  # half the traffic of (a) and of (d)
            n = (mib << 20) // scale
            a = torch.empty(n, dtype=torch.uint8, device="cuda")
            b = torch.empty(n, dtype=torch.uint8, device="cuda")
            ms = _median_ms(lambda: b.copy_(a), warmup, reps)
            row(f"copy_ {mib // scale} MiB{tag}", ms, 2 * n)
            del a, b

    copies("")
    cases = (
        ("(a) int64->u2, 4096 full", torch.int64, "u2", 32768, 4096, True),
        ("(b) int64->u2, 4096 ragged", torch.int64, "u2", 32768, 4096,
         False),
        ("(c) int32->u2, 128 ragged", torch.int32, "u2", 131072, 128, False),
        ("(d) int32->i4, 4096 full", torch.int32, "i4", 32768, 4096, True),
    )
    for name, sd, dd, n, T, full in cases:
        n //= scale
        S = SIZE[dd]
        src = torch.randint(0, LIMIT[dd], (n, T), dtype=sd, device="cuda",
                            generator=gen)
        counts = np.full(n, T) if full else rng.integers(0, T + 1, n)
        total = int(counts.sum())
        row_start = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=row_start[1:])
        d_start = torch.from_numpy(row_start).to("cuda")
        d_counts = torch.from_numpy(counts.astype(np.int64)).to("cuda")
        dst = torch.empty(total * S, dtype=torch.uint8, device="cuda")
        status = torch.full((1,), CLEAN, dtype=torch.int64, device="cuda")
        moved = total * (src.element_size() + S)
        ms = _median_ms(
            lambda: ops.compact_narrow(src, d_start, dst, dd, status),
            warmup, reps)
        assert int(status.item()) == CLEAN, name
        row(f"{name}: compact_narrow", ms, moved, rows=n, T=T)
        ref = _composed(src, d_counts, dd)
        assert torch.equal(ref, dst), name
        del ref
        ms = _median_ms(lambda: _composed(src, d_counts, dd), warmup, reps)
        row(f"{name}: composed", ms, moved, rows=n, T=T)
        del src, dst
    copies(" (again)")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=int, default=1,
                    help="divide every case's row count by this (a quick "
                         "run; the figures then say little)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("narrow_bench needs a GPU: a CPU timing says nothing "
                 "about the MI355X")
    ops.require_native()
    result = {"bench": "narrow", "device": torch.cuda.get_device_name(0),
              "kernel": kernel_rates(a.scale, a.warmup, a.reps)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
