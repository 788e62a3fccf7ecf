#!/usr/bin/env python3
"""SYEV/HEEV miniapp (reference ``miniapp/miniapp_eigensolver.cpp``):
time-to-solution of the full two-stage eigensolver, or with
``--eigenvalues-only`` of the values-only driver (no eigenvectors)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from _harness import run_miniapp, random_herm
from dlaf_amd import UpLo, hermitian_eigensolver, hermitian_eigenvalues


def extra(p):
    p.add_argument("--band-size", type=int, default=0)
    p.add_argument("--eigenvalues-only", action="store_true",
                   help="hermitian_eigenvalues: Sturm bisection, no eigenvectors")
    p.add_argument("--tridiag-solver", choices=["dc", "bisect"], default="dc",
                   help="tridiagonal stage: divide and conquer, or bisection "
                        "+ inverse iteration (local grids only)")


def setup(ctx):
    a = random_herm(ctx)
    return {"a": a, "ref": a.clone()}


def run(ctx, st):
    band = ctx.opts.band_size or None
    if ctx.opts.eigenvalues_only:
        return hermitian_eigenvalues(UpLo.Lower, st["a"], ctx.comm_grid, band=band)
    w, e = hermitian_eigensolver(UpLo.Lower, st["a"], ctx.comm_grid, band=band,
                                 tridiag_solver=ctx.opts.tridiag_solver)
    return (w, e)


def check(ctx, st, result):
    a = st["ref"].to_global()
    a = torch.tril(a) + torch.tril(a, -1).mH
    if ctx.opts.eigenvalues_only:
        import numpy as np
        wref = np.linalg.eigvalsh(a.cpu().numpy())
        err = np.abs(result.cpu().numpy() - wref).max()
        return float(err / max(1.0, np.abs(wref).max()))
    w, evecs = result
    E = evecs.to_global()
    r = (a @ E - E @ torch.diag(w.to(E.dtype))).abs().max()
    return (r / max(1.0, w.abs().max())).item()


if __name__ == "__main__":
    run_miniapp("miniapp_eigensolver", setup, run, lambda ctx: None, check, extra=extra)
