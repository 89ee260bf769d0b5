#!/usr/bin/env python3
"""Delta filter on the MI355X: kernel rate and staging rate.

1. Kernel: ops.delta_filter forward and inverse, out of place and in
   place, at E in {2, 4, 8} and block_raw in {8 KiB, 64 KiB}, next to
   ``dst.copy_(src)`` of the same size in the same process.  The filter
   reads and writes every byte once, so the device copy is the
   yardstick.  GB/s counts read + write bytes; each figure is the
   median, after a warm-up, of device-event timings of windows of 10
   back-to-back launches.  The content is random bytes: the kernel's
   work does not depend on the values, and repeated in-place launches
   just keep transforming the buffer.
2. Staging: ShardStager.stage_file on an int64 cumulative-offset shard
   (Poisson(40) steps), unfiltered, shuffle 8, delta 8 and delta 8 +
   shuffle 8: file bytes and raw GB/s (host clock around stage_file,
   which ends in a stream synchronise; page-cached file, median of the
   repetitions).

Prints one line per measurement and a final JSON line with all of them.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
from shipyard_amd import ops  # noqa: E402
from shipyard_amd.data import shardfmt  # noqa: E402
from shipyard_amd.data.stager import ShardStager  # noqa: E402


INNER = 10  # launches per timed window: a lone 0.1 ms launch shows its
#             enqueue gap in the event interval


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


def kernel_rates(mib: int, warmup: int, reps: int) -> list:
    n = mib << 20
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda",
                        generator=gen)
    dst = torch.empty_like(src)
    rows = []

    def row(name, ms, **kw):
        r = dict(name=name, mib=mib, ms=round(ms, 4),
                 gbps=round(2 * n / ms / 1e6, 1), **kw)
        rows.append(r)
        print(f"{name:34s} {r['ms']:8.4f} ms  {r['gbps']:8.1f} GB/s "
              "(read+write)")

    row("copy_", _median_ms(lambda: dst.copy_(src), warmup, reps))
    for block_raw in (8192, 65536):
        for E in (2, 4, 8):
            for inverse in (False, True):
                for in_place in (False, True):
                    out = src if in_place else dst
                    ms = _median_ms(
                        lambda: ops.delta_filter(src, out, block_raw, E,
                                                 inverse=inverse),
                        warmup, reps)
                    row(f"{'undelta' if inverse else 'delta'} E={E} "
                        f"B={block_raw >> 10}K "
                        f"{'in place' if in_place else 'out of place'}",
                        ms, elem=E, block_raw=block_raw, inverse=inverse,
                        in_place=in_place)
    # the yardstick again, after the kernels: shows the drift of the run
    row("copy_ (again)", _median_ms(lambda: dst.copy_(src), warmup, reps))
    return rows


def staging_rates(mib: int, reps: int) -> list:
    n_el = (mib << 20) // 8
    offsets = np.cumsum(np.random.default_rng(1).poisson(40, n_el)).astype(
        "<i8").tobytes()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, D, S in (("unfiltered", 0, 0), ("shuffle 8", 0, 8),
                           ("delta 8", 8, 0),
                           ("delta 8 + shuffle 8", 8, 8)):
            path = os.path.join(tmp, f"offsets_{D}_{S}.syshard")
            blob = shardfmt.pack_gpu(offsets, delta_elem=D, shuffle_elem=S)
            with open(path, "wb") as f:
                f.write(blob)
            st = ShardStager(verify=True)
            out, _ = st.stage_file(path)  # warm-up: page cache, code objects
            assert bytes(out.cpu().numpy().tobytes()) == offsets
            del out
            rates = []
            for _ in range(reps):
                out, res = st.stage_file(path)
                rates.append(res.gbps)
                del out
            r = dict(name=f"stage_file {name}", raw_bytes=len(offsets),
                     file_bytes=len(blob),
                     file_over_raw=round(len(blob) / len(offsets), 4),
                     raw_gbps=round(statistics.median(rates), 2))
            rows.append(r)
            print(f"{r['name']:34s} file {r['file_bytes']:>11d} B "
                  f"({r['file_over_raw']:.3f} of raw)  "
                  f"{r['raw_gbps']:6.2f} GB/s raw")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mib", type=int, default=256,
                    help="kernel buffer size in MiB")
    ap.add_argument("--stage-mib", type=int, default=256,
                    help="raw size of the staged offset shard in MiB")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--skip-stage", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("delta_bench needs a GPU: a CPU timing says nothing "
                 "about the MI355X")
    ops.require_native()
    result = {"bench": "delta", "device": torch.cuda.get_device_name(0),
              "kernel": kernel_rates(a.mib, a.warmup, a.reps)}
    if not a.skip_stage:
        result["staging"] = staging_rates(a.stage_mib, a.stage_reps)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
