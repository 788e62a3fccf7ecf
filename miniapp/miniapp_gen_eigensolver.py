#!/usr/bin/env python3
"""SYGV/HEGV miniapp (reference ``miniapp/miniapp_gen_eigensolver.cpp``);
``--eigenvalues-only`` times the values-only driver (no eigenvectors)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from _harness import run_miniapp, random_herm, random_spd
from dlaf_amd import (UpLo, hermitian_generalized_eigensolver,
                      hermitian_generalized_eigenvalues)


def extra(p):
    p.add_argument("--eigenvalues-only", action="store_true",
                   help="hermitian_generalized_eigenvalues: no eigenvectors")
    p.add_argument("--tridiag-solver", choices=["dc", "bisect"], default="dc",
                   help="tridiagonal stage: divide and conquer, or bisection "
                        "+ inverse iteration (local grids only)")


def setup(ctx):
    st = {"a": random_herm(ctx), "b": random_spd(ctx)}
    if ctx.opts.check_result != "none":
        st["a0"], st["b0"] = st["a"].clone(), st["b"].clone()
    return st


def run(ctx, st):
    if ctx.opts.eigenvalues_only:
        return hermitian_generalized_eigenvalues(UpLo.Lower, st["a"], st["b"],
                                                 ctx.comm_grid)
    return hermitian_generalized_eigensolver(
        UpLo.Lower, st["a"], st["b"], ctx.comm_grid,
        tridiag_solver=ctx.opts.tridiag_solver)


def check(ctx, st, result):
    """max |A E - B E diag(w)| / (|w|_max |B|_max)."""
    import torch
    a = st["a0"].to_global()
    a = torch.tril(a) + torch.tril(a, -1).mH
    b = st["b0"].to_global()
    b = torch.tril(b) + torch.tril(b, -1).mH
    if ctx.opts.eigenvalues_only:
        # max |w - eigvalsh(L^-1 A L^-H)| / |w|_max
        import numpy as np
        li = np.linalg.inv(np.linalg.cholesky(b.cpu().numpy()))
        c = li @ a.cpu().numpy() @ li.conj().T
        wref = np.linalg.eigvalsh(0.5 * (c + c.conj().T))
        err = np.abs(result.cpu().numpy() - wref).max()
        return float(err / max(1.0, np.abs(wref).max()))
    w, evecs = result
    E = evecs.to_global()
    r = (a @ E - b @ (E * w.to(E.dtype))).abs().max()
    return (r / max(1.0, w.abs().max().item()) / b.abs().max()).item()


if __name__ == "__main__":
    run_miniapp("miniapp_gen_eigensolver", setup, run, lambda ctx: None, check,
                extra=extra)
