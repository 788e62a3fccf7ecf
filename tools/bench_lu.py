"""Time lu_factorization next to torch.linalg.lu_factor on the same device.

usage: bench_lu.py [--n N ...] [--nb NB] [--types dz] [--reps R]
Defaults: n = 8192 16384 32768, nb = 512, float64 and complex128. For each
(n, dtype), on a matrix uniform in +-0.5 restored before every call (the copy
not timed):
  lu_factorization   warmed, median of R calls, each bracketed by a device
                     synchronize (the call ends in its one host read, info)
  panel / interchanges / row solve / trailing update
                     one more factorization with device events around each
                     step of each tile column; the four sums, and the rate of
                     the trailing update over its 2 nb^3 flops per tile triple
                     (8 nb^3 complex)
  torch lu_factor    torch.linalg.lu_factor on a copy, same protocol
  residual           ||P A - L U||_1 / ||A||_1 of both (n <= 16384 only: the
                     check multiplies the factors)
Prints a table and repeats every row as one JSON line. A GPU is required:
there is nothing to measure on the host."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[8192, 16384, 32768])
ap.add_argument("--nb", type=int, default=512)
ap.add_argument("--types", default="dz")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-torch", action="store_true")
args = ap.parse_args()
import torch
from dlaf_amd import Matrix, lu_factorization
from dlaf_amd.algs import lu as lu_mod
from dlaf_amd.ops._ext import get_ext

assert torch.cuda.is_available(), "bench_lu.py needs a GPU"
dev = "cuda"
sync = torch.cuda.synchronize
DTYPES = {"d": torch.float64, "z": torch.complex128,
          "s": torch.float32, "c": torch.complex64}


def timed(fn, before, reps, warm=1):
    for _ in range(warm):
        before()
        fn()
    ts = []
    for _ in range(reps):
        before()
        sync(); t0 = time.perf_counter(); fn(); sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def residual(a, lu, piv0):
    """||P A - L U||_1 / ||A||_1 on the device; piv0 0-based interchanges."""
    n = a.shape[0]
    perm = torch.arange(n, device=a.device)
    for j, p in enumerate(piv0.tolist()):
        if p != j:
            perm[[j, p]] = perm[[p, j]]
    eye = torch.eye(n, dtype=a.dtype, device=a.device)
    r = a[perm] - (torch.tril(lu, -1) + eye) @ torch.triu(lu)
    return float(r.abs().sum(0).max() / a.abs().sum(0).max())


def phases(A, keep):
    """Device time of each step, summed over the tile columns."""
    A.storage.copy_(keep)
    n, nt = A.dist.m, A.dist.nr_tiles[0]
    ipiv = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    rowbuf = lu_mod._row_buffer(A)
    marks = []
    for k in range(nt):
        row = [torch.cuda.Event(enable_timing=True)]
        row[0].record()
        for step in lu_mod.STEPS:
            step(A, k, ipiv, info, rowbuf)
            row.append(torch.cuda.Event(enable_timing=True))
            row[-1].record()
        marks.append(row)
    sync()
    return [sum(r[i].elapsed_time(r[i + 1]) for r in marks) * 1e-3
            for i in range(len(lu_mod.STEPS))]


for n in args.n:
    for t in args.types:
        dtype = DTYPES[t]
        nb = args.nb
        A = Matrix.create(n, n, nb, nb, dtype=dtype, device=dev)
        torch.manual_seed(n)
        A.storage.copy_(torch.rand(A.storage.shape, dtype=dtype, device=dev))
        if dtype.is_complex:
            A.storage.sub_(0.5 + 0.5j)
        else:
            A.storage.sub_(0.5)
        A._set_identity_pad()
        keep = A.storage.clone()
        restore = lambda: A.storage.copy_(keep)  # noqa: E731
        med, mn = timed(lambda: lu_factorization(A), restore, args.reps)
        restore()
        ipiv, info = lu_factorization(A)
        dist = A.dist
        nt = dist.nr_tiles[0]
        flops_tri = (8 if dtype.is_complex else 2) * nb ** 3
        trail_flops = flops_tri * sum((nt - k - 1) ** 2 for k in range(nt))
        total_flops = (4 if dtype.is_complex else 1) * 2 / 3 * n ** 3
        out = {"n": n, "nb": nb, "dtype": str(dtype),
               "w": get_ext().LU_W, "info": info,
               "lu_ms": med * 1e3, "lu_min_ms": mn * 1e3,
               "lu_tflops": total_flops / med / 1e12}
        small = n <= 16384
        if small:
            a0 = Matrix(A.dist, dtype, A.device, None,
                        _storage=keep).to_global()
            out["residual"] = residual(a0, A.to_global(), ipiv)
        ph = phases(A, keep)
        for name, v in zip(("panel", "interchanges", "row_solve", "trailing"),
                           ph):
            out[f"{name}_ms"] = v * 1e3
        out["trailing_tflops"] = trail_flops / ph[3] / 1e12 if ph[3] else 0.0
        del A
        if not args.no_torch:
            g = Matrix(dist, dtype, dev, None, _storage=keep).to_global()
            del keep
            work = torch.empty_like(g)
            tmed, tmn = timed(lambda: torch.linalg.lu_factor(work),
                              lambda: work.copy_(g), args.reps)
            out["torch_ms"] = tmed * 1e3
            out["torch_min_ms"] = tmn * 1e3
            if small:
                lu, piv = torch.linalg.lu_factor(g)
                out["torch_residual"] = residual(g, lu, piv - 1)
                del lu
            del g, work
        torch.cuda.empty_cache()
        print(f"n={n} nb={nb} {dtype}: lu {out['lu_ms']:9.1f} ms "
              f"({out['lu_tflops']:.1f} TF/s)  panel {out['panel_ms']:8.1f}  "
              f"swaps {out['interchanges_ms']:7.1f}  row solve "
              f"{out['row_solve_ms']:7.1f}  trailing {out['trailing_ms']:8.1f}"
              f" ms ({out['trailing_tflops']:.1f} TF/s)  torch "
              f"{out.get('torch_ms', float('nan')):9.1f} ms")
        print(json.dumps(out))
