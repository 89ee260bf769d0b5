"""A/B: v2 strided CRC kernel vs v3 coalesced-tile kernel.
Correctness vs CPU reference first, then DVFS-warmed throughput at
several chunk sizes and grid caps."""
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from shipyard_amd import ops  # noqa: E402
from shipyard_amd.ops import gf2  # noqa: E402


def check_correct():
    for chunk in (32768, 65536, 262144):
        n = chunk * 7
        data = torch.randint(0, 256, (n,), dtype=torch.uint8,
                             device="cuda")
        raw_v3 = ops.crc32c_chunks_coal_raw(data, chunk_size=chunk)
        raw_v2 = ops.crc32c_chunks(data, chunk_size=chunk, finish=False)
        assert torch.equal(raw_v3, raw_v2), (chunk, raw_v3[:4],
                                             raw_v2[:4])
        # and against the CPU reference on a sample
        host = bytes(data[:chunk].cpu().numpy().tobytes())
        ref = gf2.crc32c_raw(host)
        assert int(raw_v3[0].item()) == ref, (chunk, ref)
    print(json.dumps({"correct": True}), flush=True)


def bench(fn, size, iters=10, warm_s=0.8):
    data = torch.randint(0, 256, (size,), dtype=torch.uint8,
                         device="cuda")
    fn(data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        fn(data)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn(data)
    torch.cuda.synchronize()
    return size / ((time.perf_counter() - t0) / iters) / 1e9


def main():
    assert torch.cuda.is_available()
    check_correct()
    size = 1 << 30

    def run_v2(data, chunk):
        n_chains = gf2.pick_crc_chains(chunk)
        mats = torch.tensor(gf2.level_matrices(chunk, 256 * n_chains),
                            dtype=torch.int64).to(torch.uint32).cuda()
        out = torch.empty(size // chunk, dtype=torch.uint32,
                          device="cuda")

        def f(d):
            ops._call("sy_crc32c_chunks", d, size, chunk, mats, out,
                      size // chunk, n_chains)
        return f

    def run_v3(data, chunk):
        mats = torch.tensor(gf2.coalesced_matrices(),
                            dtype=torch.int64).to(torch.uint32).cuda()
        out = torch.empty(size // chunk, dtype=torch.uint32,
                          device="cuda")

        def f(d):
            ops._call("sy_crc32c_chunks_coal", d, size, chunk, mats, out,
                      size // chunk)
        return f

    for chunk in (65536, 262144, 1048576):
        data = torch.randint(0, 256, (size,), dtype=torch.uint8,
                             device="cuda")
        for name, mk in (("v2", run_v2), ("v3_coal", run_v3)):
            f = mk(data, chunk)
            f(data)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.8:
                f(data)
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                f(data)
            torch.cuda.synchronize()
            gbps = size / ((time.perf_counter() - t0) / 10) / 1e9
            print(json.dumps({"kernel": name, "chunk": chunk,
                              "GBps": round(gbps, 1),
                              "grid_env": os.environ.get(
                                  "SY_CRC_COAL_GRID", "default")}),
                  flush=True)
        del data


if __name__ == "__main__":
    main()
