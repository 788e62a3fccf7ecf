"""Time cholesky_rcond with the vector-solve kernel against the "blocked"
method, with the Cholesky factorization of the same matrix as the yardstick.

usage: bench_rcond.py [n [nb [d|z|s|c]]] [--reps R] [--no-blocked]
Warmed, median of R calls, each bracketed by a device synchronize (the
estimate ends in host reads anyway). Prints, and repeats as one JSON line:
  potrf            cholesky_factorization of the matrix (restored before each
                   call, the copy not timed)
  rcond kernel     cholesky_rcond(method="kernel"), diagonal inverses included
  rcond blocked    cholesky_rcond(method="blocked")
  solves           vector solves per estimate (two per estimator step)
  diag inverses    tri_inverse_full_many over the nt diagonal tiles alone, and
                   its share of the kernel-method estimate
  one solve N / C  a single kernel solve, against the floor of reading the
                   triangle once: n^2 / 2 * itemsize / 6.3 TB/s
A GPU is required: there is nothing to measure on the host."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=32768)
ap.add_argument("nb", nargs="?", type=int, default=512)
ap.add_argument("type", nargs="?", choices="dzsc", default="d")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-blocked", action="store_true")
args = ap.parse_args()
import torch
from dlaf_amd import (Matrix, UpLo, Op, Diag, matrix_norm,
                      cholesky_factorization, cholesky_rcond,
                      TriangularVectorSolver)
from dlaf_amd.matrix import util as mutil
from dlaf_amd.ops import tile_ops as ops

assert torch.cuda.is_available(), "bench_rcond.py needs a GPU"
HBM = 6.3e12  # bytes/s
n, nb = args.n, args.nb
dtype = {"d": torch.float64, "z": torch.complex128,
         "s": torch.float32, "c": torch.complex64}[args.type]
dev = "cuda"
mat = Matrix.create(n, n, nb, nb, dtype=dtype, device=dev)
mutil.set_random_hermitian_positive_definite(mat, seed=1)
anorm = matrix_norm("one", mat, uplo=UpLo.Lower, structure="hermitian")
keep = mat.storage.clone()
sync = torch.cuda.synchronize


def timed(fn, reps=args.reps, before=None, warm=2):
    for _ in range(warm):
        if before:
            before()
        fn()
    ts = []
    for _ in range(reps):
        if before:
            before()
        sync(); t0 = time.perf_counter(); fn(); sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


out = {"n": n, "nb": nb, "dtype": str(dtype)}
print(f"n={n} nb={nb} {dtype} matrix {keep.numel() * keep.element_size() / 2**30:.2f} GiB")
potrf, _ = timed(lambda: cholesky_factorization(UpLo.Lower, mat), reps=3,
                 before=lambda: mat.storage.copy_(keep), warm=1)
del keep
out["potrf_ms"] = potrf * 1e3
print(f"{'potrf':22s} median {potrf * 1e3:10.3f} ms")

# vector solves per estimate
count = [0]
_solve = TriangularVectorSolver.solve


def _counting(self, op, x):
    count[0] += 1
    return _solve(self, op, x)


results = {}
for method in ("kernel",) + (() if args.no_blocked else ("blocked",)):
    TriangularVectorSolver.solve = _counting
    count[0] = 0
    results[method] = cholesky_rcond(UpLo.Lower, mat, anorm, method=method)
    TriangularVectorSolver.solve = _solve
    solves = count[0]
    med, mn = timed(lambda: cholesky_rcond(UpLo.Lower, mat, anorm,
                                           method=method),
                    reps=args.reps if method == "kernel" else 3, warm=1)
    out[f"rcond_{method}_ms"] = med * 1e3
    out[f"solves_{method}"] = solves
    print(f"{'rcond ' + method:22s} median {med * 1e3:10.3f} ms  min "
          f"{mn * 1e3:10.3f} ms  {solves} solves  rcond={results[method]:.6e}"
          f"  {med / potrf * 100:6.1f} % of potrf")
out["rcond"] = results["kernel"]

nt = mat.dist.nr_tiles[0]
dinv, _ = timed(lambda: ops.tri_inverse_full_many(
    (mat.tile((k, k)) for k in range(nt)), lower=True, unit=False))
out["diag_inverses_ms"] = dinv * 1e3
print(f"{'diag inverses':22s} median {dinv * 1e3:10.3f} ms  "
      f"{dinv * 1e3 / out['rcond_kernel_ms'] * 100:6.1f} % of rcond kernel")

sv = TriangularVectorSolver(UpLo.Lower, Diag.NonUnit, mat, method="kernel")
x = torch.ones(n, dtype=dtype, device=dev)
floor = n * n / 2 * mat.storage.element_size() / HBM
out["solve_floor_ms"] = floor * 1e3
for op in (Op.NoTrans, Op.ConjTrans):
    med, mn = timed(lambda: sv.solve(op, x.fill_(1.0)), reps=max(args.reps, 9))
    out[f"solve_{op.value}_ms"] = med * 1e3
    print(f"{'one solve ' + op.value:22s} median {med * 1e3:10.3f} ms  min "
          f"{mn * 1e3:10.3f} ms  floor {floor * 1e3:8.3f} ms  "
          f"{med / floor:6.2f} x floor")
print(json.dumps(out))
