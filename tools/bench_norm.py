"""Time matrix_norm against the per-tile max_norm loop and a torch reduction.

usage: bench_norm.py [n [nb [d|z|s|c]]] [--reps R] [--structure S]
Warmed, median of R calls (each bracketed by a device synchronize; every
call ends in a host read of the result anyway). Prints seconds and the
achieved read rate n*n*itemsize / t for: matrix_norm max / one / inf / fro,
the norm kernel alone (no host read-back), max_norm, storage.abs().amax()
(the yardstick of the issue: a full pass, plus the abs temporary) and
storage.aminmax() (one read pass, no temporary)."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=32768)
ap.add_argument("nb", nargs="?", type=int, default=512)
ap.add_argument("type", nargs="?", choices="dzsc", default="d")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--structure", default="general",
                choices=["general", "hermitian", "triangular"])
args = ap.parse_args()
import torch
from dlaf_amd import Matrix, UpLo, matrix_norm, max_norm
from dlaf_amd.matrix import util as mutil
from dlaf_amd.algs.norm import _local_partials

n, nb = args.n, args.nb
dtype = {"d": torch.float64, "z": torch.complex128,
         "s": torch.float32, "c": torch.complex64}[args.type]
dev = "cuda" if torch.cuda.is_available() else "cpu"
mat = Matrix.create(n, n, nb, nb, dtype=dtype, device=dev)
mutil.set_random_hermitian(mat, seed=1)
uplo = None if args.structure == "general" else UpLo.Lower
code = {"general": 0, "hermitian": 1, "triangular": 2}[args.structure]
nbytes = n * n * mat.storage.element_size()


def sync():
    if dev == "cuda":
        torch.cuda.synchronize()


def timed(name, fn):
    fn(); fn(); sync()
    ts = []
    for _ in range(args.reps):
        sync(); t0 = time.perf_counter(); fn(); sync()
        ts.append(time.perf_counter() - t0)
    med = statistics.median(ts)
    print(f"{name:28s} median {med * 1e3:10.3f} ms  min {min(ts) * 1e3:10.3f} ms"
          f"  {nbytes / med / 1e12:6.3f} TB/s of matrix bytes")
    return med


print(f"n={n} nb={nb} {dtype} structure={args.structure} dev={dev} "
      f"matrix {nbytes / 2**30:.2f} GiB")
for k in ("max", "one", "inf", "fro"):
    timed(f"matrix_norm {k}", lambda: matrix_norm(
        k, mat, uplo=uplo, structure=args.structure))
timed("norm kernel, both passes", lambda: _local_partials(mat, code, False,
                                                          False))
timed("max_norm (per-tile loop)", lambda: max_norm(mat, uplo))
timed("storage.abs().amax()", lambda: mat.storage.abs().amax().item())
if not dtype.is_complex:
    timed("storage.aminmax()", lambda: [float(v) for v in mat.storage.aminmax()])
