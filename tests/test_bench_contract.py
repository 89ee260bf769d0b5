"""Driver-contract guard: `python bench.py` emits exactly one JSON line
with every field the round harness depends on."""
import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).parents[1]

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"}


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--steps", "2",
         "--warmup", "1", "--payload-mb", "4", "--full"],
        capture_output=True, text=True, timeout=300, cwd=str(REPO))
    assert out.returncode == 0, out.stderr[-500:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    doc = json.loads(lines[0])
    assert REQUIRED <= set(doc)
    assert doc["metric"] == "rccl_allreduce_bus_GBps"
    assert doc["n_gpus"] == 1 and doc["steps"] == 2 and doc["warmup"] == 1
    assert doc["higher_is_better"] is True
    assert doc["scaling"] == "weak"
    assert doc["dtype"] == "bf16" and doc["data"] == "synthetic"
    assert isinstance(doc["value"], (int, float)) and doc["value"] > 0
    cfg = doc["config"]
    for key in ("model", "global_batch", "seq_len", "parallelism"):
        assert key in cfg
    # p50 measured through the executor
    assert cfg["submit_launch_p50_ms"] is None or \
        cfg["submit_launch_p50_ms"] > 0


def test_bench_plain_run_dumps_reproducible_outputs(tmp_path):
    """A plain run (no --full) skips the executor latency measurement,
    and --dump-outputs writes the last step's buffer as float32 .npy,
    identical from run to run (seeded inputs)."""
    import numpy as np

    arrays = []
    for name in ("a", "b"):
        d = tmp_path / name
        out = subprocess.run(
            [sys.executable, str(REPO / "bench.py"), "--gpus", "1",
             "--steps", "3", "--warmup", "1", "--payload-mb", "1",
             "--dump-outputs", str(d)],
            capture_output=True, text=True, timeout=300, cwd=str(REPO))
        assert out.returncode == 0, out.stderr[-500:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout
        doc = json.loads(lines[0])
        assert REQUIRED <= set(doc)
        assert doc["steps"] == 3 and doc["ms_per_step"] > 0
        assert doc["config"]["submit_launch_p50_ms"] is None
        files = sorted(p.name for p in d.iterdir())
        assert files == ["reduce_out.npy"]
        arr = np.load(d / "reduce_out.npy")
        assert arr.dtype == np.float32 and arr.ndim == 1
        assert 0 < arr.nbytes <= 64 << 20
        assert np.isfinite(arr).all() and arr.std() > 0
        arrays.append(arr)
    assert np.array_equal(arrays[0], arrays[1])


def test_bench_world2_gloo_contract():
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29533", str(REPO / "bench.py"),
         "--gpus", "2", "--steps", "2", "--warmup", "1",
         "--payload-mb", "2"],
        capture_output=True, text=True, timeout=300, cwd=str(REPO))
    assert out.returncode == 0, out.stderr[-800:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout  # rank 0 only
    doc = json.loads(lines[0])
    assert doc["n_gpus"] == 2
    assert doc["config"]["parallelism"] == "gang2"


def test_bench_world2_torchrun_contract(tmp_path):
    """The driver's exact launch shape (torch.distributed.run, one
    rank per GPU) at world 2 on CPU/gloo: rank 0 prints ONE valid JSON
    line with whole-job semantics (n_gpus=2, MAX-over-ranks timing,
    tuning profile applied)."""
    import json
    import socket
    import subprocess
    import sys
    from pathlib import Path

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    repo = Path(__file__).parents[1]
    res = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(port), str(repo / "bench.py"),
         "--gpus", "2", "--steps", "2", "--warmup", "1",
         "--payload-mb", "2", "--latency-samples", "2"],
        capture_output=True, text=True, timeout=300, cwd=str(repo))
    assert res.returncode == 0, res.stderr[-800:]
    lines = [ln for ln in res.stdout.splitlines()
             if ln.startswith("{")]
    assert len(lines) == 1, res.stdout  # exactly one JSON line (rank 0)
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert out["metric"] == "rccl_allreduce_bus_GBps"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"]["parallelism"] == "gang2"
    # the committed tuning profile reached the env before init
    assert out["config"]["rccl_tuning_applied"].get(
        "NCCL_MIN_NCHANNELS") == "16"


def test_bench_world4_torchrun_contract(tmp_path):
    """SCALE's N=4 shape on CPU/gloo: aggregate semantics hold at
    more than two ranks (busbw factor 2*(N-1)/N, single JSON line)."""
    import json
    import socket
    import subprocess
    import sys
    from pathlib import Path

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    repo = Path(__file__).parents[1]
    res = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
         "--master-port", str(port), str(repo / "bench.py"),
         "--gpus", "4", "--steps", "2", "--warmup", "1",
         "--payload-mb", "1", "--latency-samples", "1"],
        capture_output=True, text=True, timeout=300, cwd=str(repo))
    assert res.returncode == 0, res.stderr[-800:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4
    assert out["config"]["parallelism"] == "gang4"
    assert out["config"]["rccl_tuning_applied"].get(
        "NCCL_MIN_NCHANNELS") == "24"
