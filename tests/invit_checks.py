"""Checks shared by the inverse-iteration tests (CPU host twin and GPU
kernel): the eigenvector bounds of ``tests/test_tridiag.py`` and the column
backward error of one shifted solve.
"""

import numpy as np
import torch

import tridiag_cases as tc
from dlaf_amd import tridiagonal_eigenvalues, tridiagonal_eigenvectors
from dlaf_amd.ops._ext import get_ext

SIZES = [1, 2, 3, 63, 64, 65, 257]
RANGES_257 = [(0, 1), (256, 257), (5, 5), (17, 93)]
CHUNK_CASES = ["random", "glued_wilkinson", "graded"]   # n = 1025, [400, 520)
SOLVE_SIZES = [2, 3, 65, 1025]
SOLVE_FAMILIES = ["toeplitz", "random"]
SOLVE_BOUND = 64.0


def _t(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def check_eigenvectors(family, n, ib=0, ie=None, device="cpu", **kw):
    """Eigenvectors of the index range on ``device`` against the D&C bounds
    max|T Z - Z w| < 1e-12 n scale and max|Z^T Z - I| < 1e-12 n."""
    ie = n if ie is None else ie
    d, e = tc.make_case(family, n)
    w = tridiagonal_eigenvalues(_t(d), _t(e), ib, ie)
    Z = tridiagonal_eigenvectors(_t(d, device), _t(e, device), w.to(device),
                                 **kw)
    k = ie - ib
    assert Z.shape == (n, k) and Z.dtype == torch.float64
    assert Z.device.type == torch.device(device).type
    if k == 0:
        return Z
    Zn, wn = Z.cpu().numpy(), w.numpy()
    TZ = d[:, None] * Zn
    if n > 1:
        TZ[:-1] += e[:, None] * Zn[1:]
        TZ[1:] += e[:, None] * Zn[:-1]
    scale = max(1.0, np.abs(d).max(), np.abs(e).max() if n > 1 else 0.0)
    res = np.abs(TZ - Zn * wn).max()
    orth = np.abs(Zn.T @ Zn - np.eye(k)).max()
    G = tc.gershgorin(d, e)[2] or 1.0
    print(f"{family} n={n} [{ib},{ie}): res = {res / (n * tc.EPS * G):.3f}, "
          f"orth = {orth / (n * tc.EPS):.3f} n*eps*G "
          f"(bound {1e-12 / tc.EPS:.0f})")
    assert res < 1e-12 * n * scale, f"res={res}"
    assert orth < 1e-12 * n, f"orth={orth}"
    return Z


def solve_case(family, n, at_eigenvalues):
    """Scaled (d, e), shifts, tol and a random X for one direct solve."""
    d, e = tc.make_case(family, n)
    nrm = max(np.abs(d).max(), np.abs(e).max())
    ds, es = d / nrm, e / nrm
    r = np.abs(ds).copy()
    r[:-1] += np.abs(es)
    r[1:] += np.abs(es)
    t1 = float(r.max())
    w = tridiagonal_eigenvalues(_t(ds), _t(es)).numpy()
    lam = w if at_eigenvalues else 0.5 * (w[:-1] + w[1:])
    g = torch.Generator().manual_seed(3)
    X = torch.rand((n, len(lam)), generator=g, dtype=torch.float64) * 2 - 1
    return ds, es, np.ascontiguousarray(lam), t1, X


def run_solve(ds, es, lam, t1, X, device):
    n, k = X.shape
    Y = X.clone().to(device)
    work = torch.empty((3, n, k), dtype=torch.float64, device=device)
    get_ext().tridiag_shifted_solve(_t(ds, device), _t(es, device),
                                    _t(lam, device), tc.EPS * t1, Y, work)
    return Y.cpu()


def check_solve(family, n, at_eigenvalues, device="cpu"):
    """Column backward error |(T - lam) y - x|_inf / (eps (|T|_1 + |lam|)
    |y|_inf) <= 64 for every column."""
    ds, es, lam, t1, X = solve_case(family, n, at_eigenvalues)
    Y = run_solve(ds, es, lam, t1, X, device).numpy()
    assert np.isfinite(Y).all()
    R = ds[:, None] * Y - lam * Y
    R[:-1] += es[:, None] * Y[1:]
    R[1:] += es[:, None] * Y[:-1]
    R -= X.numpy()
    be = (np.abs(R).max(0)
          / (tc.EPS * (t1 + np.abs(lam)) * np.abs(Y).max(0))).max()
    where = "eigenvalues" if at_eigenvalues else "midpoints"
    print(f"{family} n={n} at {where}: backward error = {be:.3f} "
          f"(bound {SOLVE_BOUND:.0f})")
    assert be <= SOLVE_BOUND
    return Y
