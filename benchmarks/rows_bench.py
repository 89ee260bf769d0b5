#!/usr/bin/env python3
"""Typed row reads on the MI355X: the gather_widen kernel and row staging.

1. Kernel: ops.gather_widen in four cases.  GB/s counts the source bytes
   of the rows read plus all n * T * D bytes of the output written; each
   figure is the median, after a warm-up, of device-event timings of
   windows of 10 back-to-back calls.  The content is random bytes.
   (a) 32768 rows of 4096 u2 -> int64, full rows, shuffled row order;
   (b) the same with counts uniform in 0..4096;
   (c) 131072 rows of T = 128 u2 -> int32, counts uniform in 0..128,
       random starts in a 256 MiB source;
   (d) 32768 rows of 4096 i4 -> int32, full rows: a copy with padding.
   Next to each case, the same tensor made by the composed path that
   the byte range read offers: torch.full of the byte rows,
   ops.gather_ranges (three launches), a view and ``.to`` to widen, and
   a pad mask built from the counts and applied with ``masked_fill_``.
   Its bytes are counted like the kernel's (what the result needs, not
   what the passes move), and its result is compared with the kernel's.
   ``dst.copy_(src)`` of 256 MiB and of 512 MiB is timed before and
   after the kernels.
2. Staging: ShardStager.stage_rows for 1024 random 8 KiB samples as the
   int64 rows of a batch, against stage_ranges plus the torch tail
   (view, widen, masked pad), on two 256 MiB token shards (Zipf(1.3)
   ids capped at 50000, 8 KiB blocks): int32 ids with shuffle_elem=4
   and uint16 ids with shuffle_elem=2.  Host clock around the call,
   which ends in a device synchronise; page-cached file, median of the
   repetitions.

Prints one line per measurement and a final JSON line with all of them.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
from shipyard_amd import ops  # noqa: E402
from shipyard_amd.data import shardfmt  # noqa: E402
from shipyard_amd.data.stager import ShardStager  # noqa: E402


INNER = 10  # launches per timed window: a lone 0.1 ms launch shows its
#             enqueue gap in the event interval

# how torch reads the source elements for the composed path: a dtype it
# can view and widen, and the mask that undoes a sign extension
TORCH_SRC = {"u2": (torch.int16, 0xFFFF), "i4": (torch.int32, None)}
SIZE = {"u2": 2, "i4": 4}


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


def _dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64)).to(
        "cuda")


def _widen_tail(rows, counts, src_dtype, out_dtype, pad):
    """Byte rows -> typed rows with torch: the passes a caller of the
    byte range read runs today."""
    view, mask = TORCH_SRC[src_dtype]
    vals = rows.view(view).to(out_dtype)
    if mask is not None:
        vals &= mask
    cols = torch.arange(vals.shape[1], device=vals.device)
    return vals.masked_fill_(cols[None, :] >= counts[:, None], pad)


def _composed(src, soff, lens, doff, counts, n, T, src_dtype, out_dtype,
              pad):
    rows = torch.full((n, T * SIZE[src_dtype]), 0, dtype=torch.uint8,
                      device="cuda")
    ops.gather_ranges(src, soff, lens, rows.view(-1), doff)
    return _widen_tail(rows, counts, src_dtype, out_dtype, pad)


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
        print(f"{name:50s} {r['ms']:8.4f} ms  {r['gbps']:8.1f} GB/s "
              "(read+write)")

    def copies(tag):
        for mib in (256, 512):
            n = (mib << 20) // scale
            dst = torch.empty(n, dtype=torch.uint8, device="cuda")
            ms = _median_ms(lambda: dst.copy_(src[:n]), warmup, reps)
            row(f"copy_ {mib // scale} MiB{tag}", ms, 2 * n)
            del dst

    copies("")
    cases = (
        ("(a) u2->int64, 4096 full", "u2", torch.int64, 32768, 4096, "full"),
        ("(b) u2->int64, 4096 ragged", "u2", torch.int64, 32768, 4096,
         "ragged"),
        ("(c) u2->int32, 128 ragged, random starts", "u2", torch.int32,
         131072, 128, "random"),
        ("(d) i4->int32, 4096 full", "i4", torch.int32, 32768, 4096, "full"),
    )
    for name, sd, od, n, T, kind in cases:
        n //= scale
        S = SIZE[sd]
        n_el = n_src // S
        if kind == "random":
            starts = rng.integers(0, n_el // 2 - T, n)  # a 256 MiB source
        else:
            starts = rng.permutation(n) * T
        assert int(starts.max()) + T <= n_el
        counts = np.full(n, T) if kind == "full" else \
            rng.integers(0, T + 1, n)
        pad = 50256
        a = (_dev(starts * S), _dev(counts))
        out = torch.empty((n, T), dtype=od, device="cuda")
        moved = int(counts.sum()) * S + out.numel() * out.element_size()
        ms = _median_ms(
            lambda: ops.gather_widen(src, a[0], a[1], out, sd, pad),
            warmup, reps)
        row(f"{name}: gather_widen", ms, moved, rows=n, T=T)
        b = (_dev(counts * S), _dev(np.arange(n) * T * S))
        ref = _composed(src, a[0], b[0], b[1], a[1], n, T, sd, od, pad)
        assert torch.equal(ref, out), name
        del ref
        ms = _median_ms(
            lambda: _composed(src, a[0], b[0], b[1], a[1], n, T, sd, od, pad),
            warmup, reps)
        row(f"{name}: composed", ms, moved, rows=n, T=T)
        del out
    copies(" (again)")
    return rows


def staging_rates(mib: int, samples: int, reps: int) -> list:
    rng = np.random.default_rng(2)
    sample = 8192
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for sd, npdt, S in (("i4", "<i4", 4), ("u2", "<u2", 2)):
            n_tok = (mib << 20) // S
            # skewed token ids below a 50k vocabulary
            tokens = np.minimum(rng.zipf(1.3, n_tok), 50000).astype(npdt)
            T = sample // S
            starts = rng.integers(0, n_tok - T, samples).astype(np.int64)
            counts = np.full(samples, T, dtype=np.int64)
            d_counts = _dev(counts)
            path = os.path.join(tmp, f"tokens_{sd}.syshard")
            with open(path, "wb") as f:
                f.write(shardfmt.pack_gpu(tokens.tobytes(), block_raw=8192,
                                          shuffle_elem=S))
            st = ShardStager(verify=True)

            def typed():
                out, res = st.stage_rows(path, starts, counts, sd,
                                         torch.int64, T, 50256)
                return out, res

            def composed():
                raw, res = st.stage_ranges(path, starts * S, counts * S,
                                           row_stride=sample)
                out = _widen_tail(raw, d_counts, sd, torch.int64, 50256)
                torch.cuda.synchronize()
                return out, res

            want = torch.from_numpy(
                tokens[starts[:, None] + np.arange(T)[None, :]].astype(
                    np.int64)).to("cuda")
            for call in (typed, composed):  # warm-up and check
                out, _ = call()
                assert torch.equal(out, want), (sd, call.__name__)
                del out
            del want
            for name, call in (("stage_rows", typed),
                               ("stage_ranges + torch tail", composed)):
                secs, res = [], None
                for _ in range(reps):
                    t0 = time.perf_counter()
                    out, res = call()
                    secs.append(time.perf_counter() - t0)
                    del out
                r = dict(name=f"{name}, {sd} -> int64 ({samples} x 8 KiB "
                         f"of {mib} MiB)", file_bytes=res.file_bytes,
                         out_bytes=samples * T * 8,
                         seconds=round(statistics.median(secs), 5))
                rows.append(r)
                print(f"{r['name']:62s} file {r['file_bytes']:>10d} B  "
                      f"out {r['out_bytes']:>10d} B  {r['seconds']:9.5f} s")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=int, default=1,
                    help="divide every kernel case's row count by this "
                         "(a quick run; the figures then say little)")
    ap.add_argument("--stage-mib", type=int, default=256,
                    help="raw size of each staged token shard in MiB")
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--skip-stage", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rows_bench needs a GPU: a CPU timing says nothing "
                 "about the MI355X")
    ops.require_native()
    result = {"bench": "rows", "device": torch.cuda.get_device_name(0),
              "kernel": kernel_rates(a.scale, a.warmup, a.reps)}
    if not a.skip_stage:
        result["staging"] = staging_rates(a.stage_mib, a.samples,
                                          a.stage_reps)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
