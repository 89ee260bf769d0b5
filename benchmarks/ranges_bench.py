#!/usr/bin/env python3
"""Range reads on the MI355X: the gather_ranges kernel and range staging.

1. Kernel: ops.gather_ranges in four cases, next to its yardstick in
   the same process.  GB/s counts read + write bytes of the ranges;
   each figure is the median, after a warm-up, of device-event timings
   of windows of 10 back-to-back calls.  A call is everything
   ops.gather_ranges launches: the piece count, torch.cumsum and the
   gather.  The content is random bytes.
   (a) one 256 MiB range, both sides 16 B aligned: the work split,
       against ``dst.copy_(src)``;
   (b) the same range at source +3 / destination +5 bytes: what the
       re-alignment costs, against ``dst.copy_(src)``;
   (c) 32768 ranges of 8 KiB, all 16 B aligned: the aligned case on
       many ranges, against ops.gather_copy on the same lists;
   (d) 131072 ranges of 1..4096 bytes (uniform) at random byte offsets,
       packed output: ragged small ranges, reported on its own.
   ``dst.copy_(src)`` is timed before and after the kernels.
2. Staging: ShardStager.stage_ranges for 1024 random 8 KiB samples of a
   256 MiB int32 token shard (shuffle_elem=4, 8 KiB blocks) against
   stage_file of the whole shard: file bytes and seconds of both (host
   clock around the call, which ends in a stream synchronise;
   page-cached file, median of the repetitions).

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


def _dev(arr, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(arr)).to("cuda").view(dtype)


def kernel_rates(mib: int, warmup: int, reps: int) -> list:
    n = mib << 20
    slack = 4096
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    src = torch.randint(0, 256, (n + slack,), dtype=torch.uint8,
                        device="cuda", generator=gen)
    # (d) packs 131072 ranges of 2 KiB on average: a little room on top
    dst = torch.empty(n + n // 64 + slack, dtype=torch.uint8, device="cuda")
    rows = []

    def row(name, ms, moved, **kw):
        r = dict(name=name, ms=round(ms, 4), bytes=moved,
                 gbps=round(2 * moved / ms / 1e6, 1), **kw)
        rows.append(r)
        print(f"{name:44s} {r['ms']:8.4f} ms  {r['gbps']:8.1f} GB/s "
              "(read+write)")

    def copy():
        dst[:n].copy_(src[:n])

    row("copy_", _median_ms(copy, warmup, reps), n)

    # (a) and (b): one range
    for name, so, do in (("(a) one range, aligned", 0, 0),
                         ("(b) one range, src+3 / dst+5", 3, 5)):
        a = (_dev(np.array([so], dtype=np.int64)),
             _dev(np.array([n], dtype=np.int64)),
             _dev(np.array([do], dtype=np.int64)))
        ms = _median_ms(
            lambda: ops.gather_ranges(src, a[0], a[1], dst, a[2]),
            warmup, reps)
        row(name, ms, n, ranges=1)

    # (c) 8 KiB ranges, aligned, shuffled order; gather_copy beside it
    rng = np.random.default_rng(1)
    k = n // 8192
    soff = rng.permutation(k).astype(np.int64) * 8192
    doff = np.arange(k, dtype=np.int64) * 8192
    lens = np.full(k, 8192, dtype=np.int64)
    c = (_dev(soff), _dev(lens), _dev(doff),
         _dev(lens.astype(np.uint32).view(np.int32), torch.uint32))
    ms = _median_ms(
        lambda: ops.gather_copy(src, c[0], dst, c[2], c[3]), warmup, reps)
    row(f"(c) gather_copy, {k} x 8 KiB aligned", ms, n, ranges=k)
    ms = _median_ms(
        lambda: ops.gather_ranges(src, c[0], c[1], dst, c[2]), warmup, reps)
    row(f"(c) gather_ranges, {k} x 8 KiB aligned", ms, n, ranges=k)

    # (d) ragged: lengths 1..4096, random source offsets, packed output
    k = (n // 2048) if mib < 256 else 131072
    lens = rng.integers(1, 4097, k).astype(np.int64)
    soff = rng.integers(0, n - 4096, k).astype(np.int64)
    doff = np.zeros(k, dtype=np.int64)
    np.cumsum(lens[:-1], out=doff[1:])
    moved = int(lens.sum())
    assert moved <= dst.numel()
    d = (_dev(soff), _dev(lens), _dev(doff))
    ms = _median_ms(
        lambda: ops.gather_ranges(src, d[0], d[1], dst, d[2]), warmup, reps)
    row(f"(d) gather_ranges, {k} ragged 1..4096 B", ms, moved, ranges=k)
    # what the kernel wrote, once, against numpy on a sample of ranges
    host_src = src.cpu().numpy()
    for i in rng.integers(0, k, 64).tolist():
        got = dst[doff[i]:doff[i] + lens[i]].cpu().numpy()
        assert (got == host_src[soff[i]:soff[i] + lens[i]]).all(), i

    # the yardstick again, after the kernels: shows the drift of the run
    row("copy_ (again)", _median_ms(copy, warmup, reps), n)
    return rows


def staging_rates(mib: int, samples: int, reps: int) -> list:
    rng = np.random.default_rng(2)
    n_tok = (mib << 20) // 4
    # skewed token ids below a 50k vocabulary: the high bytes compress
    tokens = np.minimum(rng.zipf(1.3, n_tok), 50000).astype("<i4").tobytes()
    sample = 8192
    offs = rng.integers(0, len(tokens) - sample, samples).astype(np.int64)
    lens = np.full(samples, sample, dtype=np.int64)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tokens.syshard")
        blob = shardfmt.pack_gpu(tokens, block_raw=8192, shuffle_elem=4)
        with open(path, "wb") as f:
            f.write(blob)
        idx = shardfmt.read_index(blob)
        touched = len(idx.select_blocks(offs, lens))
        st = ShardStager(verify=True)
        out, _ = st.stage_file(path)  # warm-up: page cache, code objects
        whole = out.cpu().numpy()
        assert whole.tobytes() == tokens
        del out
        out, _ = st.stage_ranges(path, offs, lens, row_stride=sample)
        got = out.cpu().numpy()
        for i in range(samples):
            assert (got[i] == whole[offs[i]:offs[i] + sample]).all(), i
        del out, got, whole
        for name, call in (
                ("stage_file", lambda: st.stage_file(path)),
                ("stage_ranges", lambda: st.stage_ranges(
                    path, offs, lens, row_stride=sample))):
            secs, res = [], None
            for _ in range(reps):
                out, res = call()
                secs.append(res.seconds)
                del out
            r = dict(name=f"{name} ({samples} x 8 KiB of {mib} MiB)"
                     if name == "stage_ranges" else f"{name} ({mib} MiB)",
                     file_bytes=res.file_bytes, raw_bytes=res.raw_bytes,
                     seconds=round(statistics.median(secs), 5))
            if name == "stage_ranges":
                r["blocks_touched"] = touched
                r["blocks"] = idx.n_blocks
            rows.append(r)
            print(f"{r['name']:44s} file {r['file_bytes']:>11d} B  "
                  f"raw {r['raw_bytes']:>11d} B  {r['seconds']:9.5f} s")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mib", type=int, default=256,
                    help="bytes moved by each kernel case, in MiB")
    ap.add_argument("--stage-mib", type=int, default=256,
                    help="raw size of the staged token shard in MiB")
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--skip-stage", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ranges_bench needs a GPU: a CPU timing says nothing "
                 "about the MI355X")
    ops.require_native()
    result = {"bench": "ranges", "device": torch.cuda.get_device_name(0),
              "kernel": kernel_rates(a.mib, a.warmup, a.reps)}
    if not a.skip_stage:
        result["staging"] = staging_rates(a.stage_mib, a.samples,
                                          a.stage_reps)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
