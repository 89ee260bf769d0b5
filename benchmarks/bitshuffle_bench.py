#!/usr/bin/env python3
"""Bit-shuffle filter on the MI355X: kernel rate and staging rate.

1. Kernel: ops.bit_shuffle forward and inverse at B in {2, 4, 8} and
   block_raw in {8 KiB, 64 KiB}, next to ``dst.copy_(src)`` of the same
   size in the same process.  The kernel is a copy with a transpose, so
   the device copy is the yardstick.  GB/s counts read + write bytes;
   each figure is the median, after a warm-up, of device-event timings
   of windows of 10 back-to-back launches.
2. Staging: ShardStager.stage_file on a bf16 N(0, 0.02) weight shard,
   bitshuffle_elem=2 against unfiltered and against shuffle_elem=2:
   file bytes and raw GB/s (host clock around stage_file, which ends in
   a stream synchronise; page-cached file, median of the repetitions).

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
        print(f"{name:28s} {r['ms']:8.4f} ms  {r['gbps']:8.1f} GB/s "
              "(read+write)")
        return r

    copy = row("copy_", _median_ms(lambda: dst.copy_(src), warmup, reps))
    for block_raw in (8192, 65536):
        for B in (2, 4, 8):
            for inverse in (False, True):
                ms = _median_ms(
                    lambda: ops.bit_shuffle(src, dst, block_raw, B,
                                            inverse=inverse),
                    warmup, reps)
                r = row(f"{'unbitshuffle' if inverse else 'bitshuffle'} "
                        f"B={B} blk={block_raw >> 10}K", ms, elem=B,
                        block_raw=block_raw, inverse=inverse)
                r["of_copy"] = round(r["gbps"] / copy["gbps"], 3)
    # the yardstick again, after the kernels: shows the drift of the run
    row("copy_ (again)", _median_ms(lambda: dst.copy_(src), warmup, reps))
    return rows


def staging_rates(mib: int, reps: int) -> list:
    n_el = (mib << 20) // 2
    w = np.random.default_rng(0).normal(0, 0.02, n_el).astype(np.float32)
    weights = (w.view(np.uint32) >> 16).astype("<u2").tobytes()  # bf16
    del w
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, kw in (("unfiltered", {}),
                         ("shuffle 2", {"shuffle_elem": 2}),
                         ("bitshuffle 2", {"bitshuffle_elem": 2})):
            path = os.path.join(tmp, f"w_{name.replace(' ', '')}.syshard")
            blob = shardfmt.pack_gpu(weights, **kw)
            with open(path, "wb") as f:
                f.write(blob)
            st = ShardStager(verify=True)
            out, _ = st.stage_file(path)  # warm-up: page cache, code objects
            assert bytes(out.cpu().numpy().tobytes()) == weights
            del out
            rates = []
            for _ in range(reps):
                out, res = st.stage_file(path)
                rates.append(res.gbps)
                del out
            r = dict(name=f"stage_file {name}", raw_bytes=len(weights),
                     file_bytes=len(blob),
                     file_over_raw=round(len(blob) / len(weights), 4),
                     raw_gbps=round(statistics.median(rates), 2))
            rows.append(r)
            print(f"{r['name']:28s} file {r['file_bytes']:>11d} B "
                  f"({r['file_over_raw']:.3f} of raw)  "
                  f"{r['raw_gbps']:6.2f} GB/s raw")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mib", type=int, default=256,
                    help="kernel buffer size in MiB")
    ap.add_argument("--stage-mib", type=int, default=256,
                    help="raw size of the staged bf16 weight shard in MiB")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--skip-stage", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bitshuffle_bench needs a GPU: a CPU timing says nothing "
                 "about the MI355X")
    ops.require_native()
    result = {"bench": "bitshuffle",
              "device": torch.cuda.get_device_name(0),
              "kernel": kernel_rates(a.mib, a.warmup, a.reps)}
    if not a.skip_stage:
        result["staging"] = staging_rates(a.stage_mib, a.stage_reps)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
