#!/usr/bin/env python3
"""Packed row reads on the MI355X: the gather_pack kernel.

ops.gather_pack in four cases.  GB/s counts the source bytes of the
segments plus all bytes of the three outputs (tokens, segment_ids,
positions); each figure is the median, after a warm-up, of device-event
timings of windows of 10 back-to-back calls.  The content is random
bytes.
(a) 32768 rows of 4096, u2 -> int64, samples with counts uniform in
    1..4096 packed by shardfmt.plan_packed_rows (as many samples as fill
    the rows);
(b) the first 32768 of those samples one per row, the shape of
    rows_bench's case (b) for gather_widen;
(c) 131072 rows of 128, u2 -> int32, counts uniform in 1..32, packed,
    random starts in a 256 MiB source: many segments per wave step;
(d) 32768 rows of 4096, i4 -> int32, every row one full segment.
Next to each case, the same three tensors made by the composed path:
ops.gather_widen into an [m, max count] batch, a boolean-mask gather of
its live elements scattered into a torch.full of pad, and
repeat_interleave + arange for the other two tensors.  Its bytes are
counted like the kernel's (what the result needs, not what the passes
move), and its result is compared with the kernel's before timing.
``dst.copy_(src)`` of the same total traffic (half of it read, half
written) is timed in the same process before and after each kernel.

Also computed on the CPU: the batch fill, live elements / (n_rows * T),
of case (a)'s samples packed and one per row.

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
from shipyard_amd.data import shardfmt  # noqa: E402

INNER = 10  # launches per timed window: a lone 0.1 ms launch shows its
#             enqueue gap in the event interval
SIZE = {"u2": 2, "i4": 4}


def _median_ms(fn, warmup: int, reps: int, inner: int = INNER) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(inner):
            fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) / inner)
    return statistics.median(times)


def _dev(arr, dtype=np.int64):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype)).to("cuda")


def samples_for_rows(rng, n_rows: int, T: int, max_count: int):
    """Counts uniform in 1..max_count, as many as next-fit puts into
    n_rows rows of T, and their plan."""
    counts = rng.integers(1, max_count + 1,
                          4 * n_rows * T // (max_count + 1) + 16)
    row, col, _ = shardfmt.plan_packed_rows(counts, T)
    keep = row < n_rows
    assert not keep[-1], "drew too few samples to fill the rows"
    return counts[keep], row[keep], col[keep]


def fill_figures(scale: int = 1) -> dict:
    """Case (a)'s samples, packed and one per row: live / (rows * T)."""
    n_rows, T = 32768 // scale, 4096
    counts, _, _ = samples_for_rows(np.random.default_rng(1), n_rows, T, T)
    live = int(counts.sum())
    return dict(samples=len(counts), live=live, T=T, packed_rows=n_rows,
                fill_packed=round(live / (n_rows * T), 4),
                fill_one_per_row=round(live / (len(counts) * T), 4))


def _composed(src, soff, counts, dstart, labels, total: int, max_count: int,
              shape, src_dtype, out_dtype, pad):
    m = counts.numel()
    batch = torch.empty((m, max_count), dtype=out_dtype, device="cuda")
    ops.gather_widen(src, soff, counts, batch, src_dtype, pad)
    live = torch.arange(max_count, device="cuda")[None, :] < counts[:, None]
    seg_of = torch.repeat_interleave(torch.arange(m, device="cuda"), counts,
                                     output_size=total)
    within = torch.arange(total, device="cuda") - \
        (torch.cumsum(counts, 0) - counts)[seg_of]
    at = dstart[seg_of] + within
    tokens = torch.full(shape, pad, dtype=out_dtype, device="cuda")
    tokens.view(-1)[at] = batch[live]
    segment_ids = torch.zeros(shape, dtype=torch.int32, device="cuda")
    segment_ids.view(-1)[at] = labels[seg_of]
    positions = torch.zeros(shape, dtype=torch.int32, device="cuda")
    positions.view(-1)[at] = within.to(torch.int32)
    return tokens, segment_ids, positions


def kernel_rates(scale: int, warmup: int, reps: int) -> list:
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    n_src = (512 << 20) // scale
    src = torch.randint(0, 256, (n_src,), dtype=torch.uint8, device="cuda",
                        generator=gen)
    rng = np.random.default_rng(1)
    rows = []

    def row(name, ms, moved, **kw):
        r = dict(name=name, ms=round(ms, 4), bytes=moved,
                 gbps=round(moved / ms / 1e6, 1), **kw)
        rows.append(r)
        print(f"{name:46s} {r['ms']:9.4f} ms  {r['gbps']:8.1f} GB/s "
              "(read+write)")
        return r

    n_a, T_a = 32768 // scale, 4096
    counts_a, row_a, col_a = samples_for_rows(rng, n_a, T_a, T_a)
    n_c, T_c = 131072 // scale, 128
    counts_c, row_c, col_c = samples_for_rows(rng, n_c, T_c, 32)
    n_b = min(n_a, len(counts_a))
    cases = (
        ("(a) u2->int64, 4096 packed", "u2", torch.int64, n_a, T_a,
         counts_a, row_a, col_a, "slots"),
        ("(b) u2->int64, 4096 one per row", "u2", torch.int64, n_b, T_a,
         counts_a[:n_b], np.arange(n_b), np.zeros(n_b, dtype=np.int64),
         "slots"),
        ("(c) u2->int32, 128 packed, random starts", "u2", torch.int32, n_c,
         T_c, counts_c, row_c, col_c, "random"),
        ("(d) i4->int32, 4096 full", "i4", torch.int32, n_a, T_a,
         np.full(n_a, T_a), np.arange(n_a), np.zeros(n_a, dtype=np.int64),
         "slots"),
    )
    for name, sd, od, n, T, counts, prow, pcol, kind in cases:
        S = SIZE[sd]
        n_el = n_src // S
        m = len(counts)
        if kind == "random":
            starts = rng.integers(0, n_el // 2 - T, m)  # a 256 MiB source
        else:  # every sample in a slot of T elements of its own, shuffled
            assert m * T <= n_el, (name, m)
            starts = rng.permutation(m) * T
        order, dstart, labels = shardfmt._packed_lists(counts, prow, pcol, T)
        lists = (_dev(starts[order] * S), _dev(counts[order]), _dev(dstart),
                 _dev(labels, np.int32))
        out = (torch.empty((n, T), dtype=od, device="cuda"),
               torch.empty((n, T), dtype=torch.int32, device="cuda"),
               torch.empty((n, T), dtype=torch.int32, device="cuda"))
        total = int(counts.sum())
        moved = total * S + n * T * (out[0].element_size() + 8)
        pad = 50256

        def kernel():
            ops.gather_pack(src, *lists, *out, sd, pad)

        half = moved // 2
        c_src = torch.empty(half, dtype=torch.uint8, device="cuda")
        c_dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        c_src.random_(0, 256, generator=gen)

        def copy():
            c_dst.copy_(c_src)

        before = _median_ms(copy, warmup, reps)
        ms = _median_ms(kernel, warmup, reps)
        after = _median_ms(copy, warmup, reps)
        del c_src, c_dst
        row(f"{name}: copy_ before", before, 2 * half)
        row(f"{name}: copy_ after", after, 2 * half)
        k = row(f"{name}: gather_pack", ms, moved, rows=n, T=T, segments=m,
                fill=round(total / (n * T), 4))
        k["vs_copy"] = round(min(before, after) / ms * moved / (2 * half), 3)

        max_count = int(counts.max())

        def composed():
            return _composed(src, lists[0], lists[1], lists[2], lists[3],
                             total, max_count, (n, T), sd, od, pad)

        ref = composed()
        for r, o, which in zip(ref, out, ("tokens", "segment_ids",
                                          "positions")):
            assert torch.equal(r, o), (name, which)
        del ref, r
        cms = _median_ms(composed, 2, max(3, reps // 5), inner=2)
        row(f"{name}: composed", cms, moved, rows=n, T=T)
        k["kernel_over_composed"] = round(ms / cms, 4)
        print(f"{'':46s} {k['vs_copy']:.3f} of the copy's rate, "
              f"{cms / ms:.1f}x the composed path's speed")
        del out, lists
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=int, default=1,
                    help="divide every case's row count by this (a quick "
                         "run; the figures then say little)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--fill-only", action="store_true",
                    help="print the batch fill figures (CPU) and leave")
    a = ap.parse_args()
    fill = fill_figures(a.scale)
    print("fill", json.dumps(fill))
    if a.fill_only:
        return
    if not torch.cuda.is_available():
        sys.exit("packed_bench needs a GPU: a CPU timing says nothing "
                 "about the MI355X")
    ops.require_native()
    print(json.dumps({"bench": "packed",
                      "device": torch.cuda.get_device_name(0), "fill": fill,
                      "kernel": kernel_rates(a.scale, a.warmup, a.reps)}))


if __name__ == "__main__":
    main()
