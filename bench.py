#!/usr/bin/env python3
"""Flagship benchmark: RCCL all-reduce bus bandwidth via the gang path.

This measures BASELINE.json's headline metric — "RCCL all-reduce bus
GB/s (multi-instance task) 1/2/4/8 GPU; submit->launch p50" — the
MI355X-native analogue of the reference's mpiBench multi-instance-task
recipe (reference recipes/mpiBench-OpenMPI/config/docker/jobs.yaml).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`.
For N>1 the driver launches this under torch.distributed.run with one
rank per GPU; ranks read RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from env.
W untimed warmup steps, then EXACTLY K timed steps bracketed by a
barrier + torch.cuda.synchronize() on both sides; time is the MAX over
ranks; rank 0 prints ONE JSON line.

One "step" = R back-to-back in-place all-reduces of a fixed per-rank
payload (default 256 MiB bf16, R = --reps-per-step, default 16 on GPU
so the timed region is long enough for utilization sampling) through
the framework's GangComm — the same code path a multi-instance gang
task uses.  Value = per-op bus GB/s
(nccl-tests convention, busbw = algbw * 2*(N-1)/N).  At N=1 an
all-reduce is a no-op, so the degenerate gang-of-1 step is a local
in-place reduction y += x of the same payload and the reported value is
2*S/t (bytes of the two operands over time); this N=1 semantics is
recorded in config.n1_semantics.

A plain run sets up, warms up, times the K steps and prints the result
line.  `--full` additionally reports submit->launch p50 latency (ms)
through the local executor (single process task path), mirroring
BASELINE.md's second metric.  `--dump-outputs DIR` writes what the last
timed step left in the reduced buffer to DIR/<name>.npy (float32); the
inputs are seeded, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

# multi-process GPU runs need dmabuf IPC (the host driver rejects
# legacy IPC); harmless for single-rank runs
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def measure_submit_launch_p50(samples: int = 10):
    """Submit tiny process tasks through the executor; p50 of
    submit->launch latency in ms.  Returns None if the executor is not
    available (early bootstrap)."""
    try:
        from shipyard_amd.executor.latency import measure_submit_launch
    except Exception:
        return None
    try:
        return measure_submit_launch(samples=samples)
    except Exception:
        return None


SEED = 20240611
DUMP_MAX_ELEMS = 4 << 20  # 16 MiB of float32 per dumped array


def dump_outputs(dirname: str, arrays: dict) -> None:
    """Write each 1-D tensor as DIR/<name>.npy in float32.  An array
    longer than DUMP_MAX_ELEMS is reduced to a fixed, seeded sample of
    its elements (sorted indices, so the sample keeps buffer order).

    The step accumulates in place, so the dump is the buffer after all
    (warmup + steps) * ops_per_step operations.  At N=1 a bf16
    accumulator stops changing once x falls below half an ulp of y
    (a few hundred adds); runs with few steps and --reps-per-step 1
    give the most sensitive comparison."""
    import numpy as np
    import torch

    os.makedirs(dirname, exist_ok=True)
    for name, t in arrays.items():
        n = t.numel()
        if n > DUMP_MAX_ELEMS:
            idx = np.sort(np.random.default_rng(SEED).integers(
                0, n, size=DUMP_MAX_ELEMS))
            t = t[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(dirname, name + ".npy"),
                t.to(torch.float32).cpu().numpy())


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--payload-mb", type=int, default=256,
                   help="per-rank all-reduce payload in MiB")
    p.add_argument("--reps-per-step", type=int, default=0,
                   help="collective ops per timed step (0 = auto: "
                        "sized so a step is ~tens of ms and the smi "
                        "sampler can observe the timed region)")
    p.add_argument("--latency-samples", type=int, default=10)
    p.add_argument("--full", action="store_true",
                   help="also measure what the headline figure does not "
                        "need (submit->launch p50 through the executor)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the buffer the last "
                        "step produced to DIR/<name>.npy (float32)")
    args = p.parse_args()

    import torch

    from shipyard_amd.comm import (GangComm, apply_rccl_tuning,
                                   bus_bandwidth_gbps)

    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    # committed xGMI tuning profile (comm/rccl_tuning.yaml); must be in
    # the env before the RCCL communicator initializes
    tuning = apply_rccl_tuning(world_env)

    comm = GangComm()
    world = comm.world
    dev = comm.device
    on_gpu = dev.type == "cuda"

    payload_mb = args.payload_mb
    if not on_gpu:
        payload_mb = min(payload_mb, 8)  # CPU smoke only
    numel = payload_mb * (1 << 20) // 2  # bf16 = 2 bytes
    payload_bytes = numel * 2

    # seeded inputs (per rank): identical from run to run
    torch.manual_seed(SEED + comm.rank)
    x = torch.randn(numel, dtype=torch.float32, device=dev).to(torch.bfloat16)
    y = None
    if world == 1:
        y = torch.randn(numel, dtype=torch.float32, device=dev).to(
            torch.bfloat16)

    # inner reps: one timed "step" is R back-to-back collective ops so
    # the timed region lasts long enough for the driver's smi sampler
    # to observe gpu utilization (round-1 weak point: a 2.8 ms region
    # was never sampled).  Bandwidth stays honest: R*payload over the
    # step time.
    reps = args.reps_per_step
    if reps <= 0:
        # N=1's local add is ~0.14 ms/op: 128 reps make a ~18 ms step
        # (20 steps -> ~0.36 s timed region).  N>1 all-reduce ops are
        # ~2 ms already, so 16 reps suffice.
        reps = (128 if world == 1 else 16) if on_gpu else 1

    # a GPU run is only meaningful on a built tree: like smoke(), fail
    # loudly when the HIP ops library is missing instead of timing a
    # half-built checkout
    if on_gpu:
        from shipyard_amd import ops

        ops.require_native()

    def step() -> None:
        if world > 1:
            for _ in range(reps):
                comm.all_reduce_(x)
        else:
            for _ in range(reps):
                y.add_(x)

    # submit->launch p50 (--full, rank 0 only, before the timed region)
    p50_ms = None
    if args.full and comm.rank == 0:
        p50_ms = measure_submit_launch_p50(args.latency_samples)

    for _ in range(args.warmup):
        step()

    comm.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    if on_gpu:
        torch.cuda.synchronize()
    t1 = time.perf_counter()
    comm.barrier()

    elapsed = comm.max_scalar(t1 - t0)
    ms_per_step = elapsed / args.steps * 1e3

    per_op = elapsed / (args.steps * reps)
    if world > 1:
        value = bus_bandwidth_gbps(payload_bytes, per_op, world)
    else:
        value = 2.0 * payload_bytes / per_op / 1e9

    if args.dump_outputs and comm.rank == 0:
        # the buffer a caller of the step holds afterwards: the reduced
        # payload (identical on every rank) or, at N=1, the accumulator
        dump_outputs(args.dump_outputs,
                     {"allreduce_out": x} if world > 1 else {"reduce_out": y})

    if comm.rank == 0:
        out = {
            "metric": "rccl_allreduce_bus_GBps",
            "value": round(value, 3),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "model": "mpibench-rccl-allreduce",
                "global_batch": world,
                "seq_len": numel,
                "parallelism": f"gang{world}",
                "payload_mb_per_rank": payload_mb,
                "ops_per_step": reps,
                "n1_semantics": "local in-place add (2S bytes moved); "
                                "busbw undefined at N=1",
                "submit_launch_p50_ms": p50_ms,
                "rccl_tuning_applied": tuning,
                "device": dev.type,
            },
        }
        print(json.dumps(out), flush=True)

    comm.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
