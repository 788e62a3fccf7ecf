"""Timing breakdown of the eigensolver pipeline on GPU (SYEV config 4 shape).

usage: time_eigensolver.py [n [nb [band [d|z|s|c]]]] [--eigenvalues-only]
           [--tridiag-solver {dc,bisect}] [--eigenvalues-index-begin I]
           [--eigenvalues-index-end I] [--reps R]
``--eigenvalues-only`` times the values-only pipeline instead: red2band,
band2tridiag, Sturm bisection (no D&C, no back-transforms).
``--tridiag-solver bisect`` replaces the D&C stage by ``tridiag_bisect`` +
``tridiag_invit`` (only the selected eigenpairs). ``--reps R`` runs the whole
pipeline R times on the same input and prints every run: the first one pays
for code-object loads and library set-up. The first stage, ``norm+scale``, is
the drivers' safe-scaling step (one norm pass; the matrix here is in range,
so nothing is scaled)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=4096)
ap.add_argument("nb", nargs="?", type=int, default=512)
ap.add_argument("band", nargs="?", type=int, default=None)
ap.add_argument("type", nargs="?", choices="dzsc", default="d")
ap.add_argument("--eigenvalues-only", action="store_true")
ap.add_argument("--tridiag-solver", choices=["dc", "bisect"], default="dc")
ap.add_argument("--eigenvalues-index-begin", type=int, default=0)
ap.add_argument("--eigenvalues-index-end", type=int, default=None)
ap.add_argument("--reps", type=int, default=1)
args = ap.parse_args()
import torch
from dlaf_amd import Matrix, UpLo
from dlaf_amd.matrix import util as mutil
from dlaf_amd.algs.red2band import reduction_to_band, bt_reduction_to_band
from dlaf_amd.algs.band2tridiag import band_to_tridiagonal, bt_band_to_tridiagonal
from dlaf_amd.algs.tridiag_dc import tridiagonal_eigensolver
from dlaf_amd.algs.tridiag_invit import tridiagonal_eigenvectors
from dlaf_amd.algs.eigensolver import get_band_size
from dlaf_amd.algs import _scaling

n, nb = args.n, args.nb
band = args.band if args.band is not None else get_band_size(nb)
dtype = {"d": torch.float64, "z": torch.complex128,
         "s": torch.float32, "c": torch.complex64}[args.type]
ib = args.eigenvalues_index_begin
ie = n if args.eigenvalues_index_end is None else args.eigenvalues_index_end
dev = "cuda" if torch.cuda.is_available() else "cpu"

def sync():
    if dev == "cuda":
        torch.cuda.synchronize()

def report(title, stamps, fmt):
    tot = stamps[-1][1] - stamps[0][1]
    print(f"{title} n={n} nb={nb} band={band} dev={dev}: total {tot:.2f}s")
    for (nm, t1), (_, t0) in zip(stamps[1:], stamps[:-1]):
        print(f"  {nm:16s} {format(t1 - t0, fmt)}s")

for rep in range(args.reps):
    mat = Matrix.create(n, n, nb, nb, dtype=dtype, device=dev)
    mutil.set_random_hermitian(mat, seed=1)
    a0 = None
    if n <= 4096:
        a0 = mat.to_global()
        a0 = torch.tril(a0) + torch.tril(a0, -1).mH
    sync()
    stamps = [("start", time.perf_counter())]
    _scaling.scale_hermitian(mat, None); sync(); stamps.append(("norm+scale", time.perf_counter()))
    refl = reduction_to_band(mat, band); sync(); stamps.append(("red2band", time.perf_counter()))
    tri = band_to_tridiagonal(UpLo.Lower, band, mat); sync(); stamps.append(("band2tridiag", time.perf_counter()))
    if args.eigenvalues_only:
        from dlaf_amd import tridiagonal_eigenvalues
        w = tridiagonal_eigenvalues(tri.d, tri.e, ib, ie, device=mat.device); sync(); stamps.append(("tridiag_bisect", time.perf_counter()))
        report(f"HEEV-values[{mat.dtype}]", stamps, "8.3f")
        if a0 is not None:
            werr = (w - torch.linalg.eigvalsh(a0)[ib:ie].to(w.dtype)).abs().max().item()
            print(f"  werr={werr:.2e}")
        continue
    if args.tridiag_solver == "bisect":
        from dlaf_amd import tridiagonal_eigenvalues
        w = tridiagonal_eigenvalues(tri.d, tri.e, ib, ie, device=mat.device); sync(); stamps.append(("tridiag_bisect", time.perf_counter()))
        info = {}
        E_real = tridiagonal_eigenvectors(tri.d, tri.e, w, device=mat.device, _timings=info); sync(); stamps.append(("tridiag_invit", time.perf_counter()))
        E = E_real.to(mat.dtype)
    else:
        w, E_real = tridiagonal_eigensolver(tri.d, tri.e, device=mat.device); sync(); stamps.append(("tridiag_dc", time.perf_counter()))
        w = w[ib:ie].clone()
        E = E_real[:, ib:ie].to(mat.dtype).contiguous()
    del E_real
    bt_band_to_tridiagonal(E, tri); sync(); stamps.append(("bt_band2tridiag", time.perf_counter()))
    bt_reduction_to_band(E, mat, refl); sync(); stamps.append(("bt_red2band", time.perf_counter()))
    report(f"HEEV[{mat.dtype}] tridiag_solver={args.tridiag_solver} "
           f"range=[{ib},{ie})", stamps, "8.2f")
    if args.tridiag_solver == "bisect":
        print("  invit: " + ", ".join(
            f"{k}={v:.3f}s" if isinstance(v, float) else f"{k}={v}"
            for k, v in info.items()))
    if a0 is not None:
        res = (a0 @ E - E @ torch.diag(w.to(E.dtype))).abs().max().item()
        orth = (E.mH @ E - torch.eye(ie - ib, dtype=E.dtype, device=E.device)).abs().max().item()
        print(f"  res={res:.2e} orth={orth:.2e}")
    del E, mat, refl, tri
