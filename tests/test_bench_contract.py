"""bench.py driver contract on the CPU (gloo): one JSON line from rank 0 with
the whole-job value, launched exactly as the driver launches N > 1."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(*extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "bench.py"), "--cpu", "--gpus", "2",
           *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "transport", "rccl_ranks", "migrations_timed",
              "migrations_expected", "degraded", "failures"):
        assert k in out
    # migration health: every exchange of the timed window happened
    assert out["degraded"] is False and out["failures"] == 0
    assert out["migrations_timed"] == out["migrations_expected"] >= 1
    assert out["transport"] == "torch" and out["rccl_ranks"] == 0  # gloo: no RCCL involved
    return out


def test_expected_migrations():
    sys.path.insert(0, ROOT)
    import bench

    # IslandModel.run starts an exchange at every generation g > 0 with g % every == 0
    assert bench.expected_migrations(0, 10, 10) == 0
    assert bench.expected_migrations(2, 12, 10) == 1
    assert bench.expected_migrations(10, 20, 10) == 2
    assert bench.expected_migrations(5, 500, 10) == 50
    assert bench.expected_migrations(5, 500, 0) == 0


def _dump(tmp, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--cpu", "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs writes the population the last timed step left: every
    score, a fixed sample of decoded genomes whose scores the torch oracle
    reproduces, the best fitness; the same arguments give the same arrays,
    and --full is accepted."""
    import numpy as np
    import torch

    import libpga_amd as pga

    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    # 40000 rows of 1024 bits exceed the genome budget: 8192 rows are sampled
    out = _dump(a, "--pop", "40000")
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    _dump(b, "--pop", "40000", "--full")
    names = sorted(p.name for p in a.iterdir())
    assert names == ["best_fitness.npy", "genomes.npy", "genomes_index.npy", "scores.npy"]
    arr = {n[:-4]: np.load(a / n) for n in names}
    assert sum(v.nbytes for v in arr.values()) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) for v in arr.values())
    assert arr["scores"].shape == (40000,) and arr["genomes"].shape == (8192, 1024)
    idx = arr["genomes_index"].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < 40000
    ref = pga.models.OneMax(1024).reference_fitness(torch.from_numpy(arr["genomes"]).to(torch.uint8))
    assert np.array_equal(ref.numpy().astype(np.float32), arr["scores"][idx])
    assert arr["best_fitness"][0] == arr["scores"].max() == out["best_fitness"]
    for n in names:
        assert np.array_equal(np.load(a / n), np.load(b / n)), n


def test_bench_tsp256_two_ranks_gloo():
    """BASELINE config 5 through the driver's launcher (reduced population)."""
    out = _run("--steps", "12", "--warmup", "2", "--problem", "tsp256", "--crossover", "pmx", "--pop", "1024")
    assert out["config"]["model"] == "TSP-256" and out["config"]["crossover"] == "pmx"
    assert out["config"]["global_batch"] == 2048 and out["dtype"] == "u16-permutation"
    assert out["vs_baseline"] is None  # no reference-semantics run for TSP
    assert abs(out["value"] - out["gens_per_sec"] * 1024 * 2) < 1e-6 * out["value"]


def test_bench_two_ranks_gloo():
    out = _run("--steps", "12", "--warmup", "2", "--pop", "4096", "--length", "128")
    assert out["n_gpus"] == 2 and out["steps"] == 12 and out["warmup"] == 2 and out["scaling"] == "weak"
    # whole-job aggregate: evals/s over both islands
    assert abs(out["value"] - out["gens_per_sec"] * 4096 * 2) < 1e-6 * out["value"]
    assert abs(out["ms_per_step"] - 1e3 / out["gens_per_sec"]) < 1e-6 * out["ms_per_step"]
    assert out["config"]["global_batch"] == 8192 and out["config"]["parallelism"] == "island2"
    assert out["migrations"] >= 1
