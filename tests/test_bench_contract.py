"""bench.py driver-contract test: one JSON line with the required fields."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu",
         "--n", "1024", "--nb", "256", "--steps", "1", "--warmup", "0"],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["metric"] == "cholesky_fp64_gflops"
    assert j["unit"] == "GFlop/s"
    assert j["higher_is_better"] is True
    assert j["scaling"] == "strong"
    assert j["dtype"] == "fp64"
    assert j["n_gpus"] == 1 and j["steps"] == 1 and j["warmup"] == 0
    assert j["value"] > 0 and j["ms_per_step"] > 0
    for k in ("model", "n", "nb", "parallelism"):
        assert k in j["config"]
    assert "synthetic" in j["data"]


def test_bench_dist_cpu_2rank():
    """2-rank gloo run of bench.py (exercises the RCCL-order dry-run guard
    and the distributed POTRF path through the driver entry point)."""
    env = dict(os.environ)
    env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29571",
                "DLAF_BENCH_N": "1024", "DLAF_BENCH_NB": "256"})
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29572", os.path.join(ROOT, "bench.py"),
         "--device", "cpu", "--steps", "1", "--warmup", "0", "--gpus", "2"],
        capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2
    assert j["config"]["parallelism"] == "grid1x2"


def _run_bench_cpu(extra):
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu",
         "--n", "384", "--nb", "128", "--steps", "2", "--warmup", "1"] + extra,
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the factor of the last timed step (float64 .npy,
    identical from run to run, reconstructs the seeded input); --full keeps
    the result line's contract and a plain run carries no extra configs."""
    import numpy as np
    import torch

    from dlaf_amd import Matrix
    from dlaf_amd.matrix import util as mutil

    d1, d2 = tmp_path / "a", tmp_path / "b"
    j1 = _run_bench_cpu(["--dump-outputs", str(d1)])
    j2 = _run_bench_cpu(["--dump-outputs", str(d2), "--full"])
    for j in (j1, j2):
        assert j["metric"] == "cholesky_fp64_gflops" and j["steps"] == 2
        assert j["ms_per_step"] > 0
    assert j1["config"]["extra_configs"] == {}
    assert sorted(p.name for p in d1.iterdir()) == ["L.npy"]
    L1, L2 = np.load(d1 / "L.npy"), np.load(d2 / "L.npy")
    assert L1.dtype == np.float64 and L1.shape == (384, 384)
    assert np.array_equal(L1, L2)
    assert np.array_equal(L1, np.tril(L1))
    a = Matrix.create(384, 384, 128, 128, dtype=torch.float64)
    mutil.set_random_hermitian_positive_definite(a, seed=42)
    A = a.to_global().numpy()
    assert np.abs(L1 @ L1.T - A).max() <= 1e-12 * np.abs(A).max()


def test_bench_dump_sampled_path(tmp_path, monkeypatch):
    """Beyond the whole-factor size limit the dump is the diagonal, the last
    rows and a fixed seeded sample of the lower triangle, read through the
    tile layout (uneven last tile included)."""
    import importlib.util

    import numpy as np
    import torch

    from dlaf_amd import Matrix

    spec = importlib.util.spec_from_file_location(
        "_bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "_DUMP_FULL_MAX_BYTES", 0)
    monkeypatch.setattr(bench, "_DUMP_SAMPLES", 5000)

    n, nb = 200, 64
    g = torch.arange(n * n, dtype=torch.float64).reshape(n, n)
    m = Matrix.create(n, n, nb, nb, dtype=torch.float64)
    m.set_from_global(g)
    outs = []
    for d in (tmp_path / "a", tmp_path / "b"):
        bench._dump_outputs(str(d), m, 0)
        outs.append({p.stem: np.load(p) for p in d.iterdir()})
    o = outs[0]
    assert sorted(o) == ["L_diag", "L_sample", "L_tail_rows"]
    assert all(np.array_equal(o[k], outs[1][k]) for k in o)
    assert all(v.dtype == np.float64 for v in o.values())
    G = g.numpy()
    assert np.array_equal(o["L_diag"], np.diag(G))
    assert np.array_equal(o["L_tail_rows"], np.tril(G)[n - 64:])
    s = o["L_sample"]
    assert s.shape == (5000,)
    r, c = (s // n).astype(int), (s % n).astype(int)  # entries encode (r, c)
    assert (r >= c).all() and len(np.unique(s)) > 2000
