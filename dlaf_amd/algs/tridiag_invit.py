"""Tridiagonal eigenvectors by inverse iteration (LAPACK ``stebz`` +
``stein``): the k eigenvectors that belong to k bisection eigenvalues, in
O(n*k) memory.

``tridiagonal_eigenvectors`` runs simultaneous inverse iteration on all
selected columns: every sweep solves ``(T - lam_j I) y_j = x_j`` for each
column with the pivoted LU of ``csrc/tridiag_lu.h`` (HIP kernel
``csrc/invit.hip``, one thread per column; the host twin for CPU tensors),
normalises, and re-orthogonalises every cluster of close eigenvalues with a
QR. The rules are ``dstein``'s: coincident shifts are spread by
``10 eps ||T||_1``, eigenvalues closer than ``1e-3 ||T||_1`` form a cluster,
at most 5 sweeps. The start vectors come from a seeded CPU generator, so the
host and the device start from the same bits and repeated calls agree
bitwise.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..core.asserts import dlaf_assert
from ..ops._ext import get_ext
from .tridiag_bisect import _resolve_device, tridiagonal_eigenvalues

__all__ = ["tridiagonal_eigenvectors", "tridiagonal_eigensolver_bisect"]

EPS = 2.0 ** -52
MIN_ITS = 2
MAX_ITS = 5                 # dstein MAXITS
ORTOL = 1e-3                # dstein: cluster when the gap is below ORTOL*|T|_1
PERTOL = 10.0               # dstein: spread coincident shifts by PERTOL*eps*|T|_1
RES_TOL = 1e-12             # stop at ||T z - w z||_inf <= RES_TOL * n * scale
WORK_BYTES = 1 << 30        # budget of the [3, n, cols] U workspace
_SEED = 7


def _cluster_starts(ws: torch.Tensor, t1: float) -> list:
    """Start indices (plus k) of the maximal runs of eigenvalues whose
    consecutive gaps are below ORTOL*t1. ``ws`` host float64, ascending."""
    k = ws.shape[0]
    brk = torch.nonzero(ws[1:] - ws[:-1] >= ORTOL * t1).reshape(-1) + 1
    return [0] + brk.tolist() + [k]


def _orthogonalise(X: torch.Tensor, groups) -> None:
    """Replace the columns of every cluster by the Q of their QR; clusters of
    one size go through one batched call."""
    n = X.shape[0]
    for size, starts in groups:
        if len(starts) == 1:
            a = starts[0]
            q, _ = torch.linalg.qr(X[:, a:a + size])
            X[:, a:a + size] = q
            continue
        idx = (torch.tensor(starts, device=X.device).unsqueeze(1)
               + torch.arange(size, device=X.device)).reshape(-1)
        blk = X[:, idx].reshape(n, len(starts), size).permute(1, 0, 2)
        q, _ = torch.linalg.qr(blk.contiguous())
        X[:, idx] = q.permute(1, 0, 2).reshape(n, -1)


def _residuals(ds, es, ws, Z) -> torch.Tensor:
    """Column residuals ||T z - w z||_inf, O(n k)."""
    R = ds.unsqueeze(1) * Z - Z * ws
    R[:-1] += es.unsqueeze(1) * Z[1:]
    R[1:] += es.unsqueeze(1) * Z[:-1]
    return R.abs().amax(dim=0)


def tridiagonal_eigenvectors(d: torch.Tensor, e: torch.Tensor, w: torch.Tensor,
                             device=None, *, _work_cols: Optional[int] = None,
                             _timings: Optional[dict] = None) -> torch.Tensor:
    """Orthonormal eigenvectors ``Z`` [n, len(w)] (float64, on ``device``,
    default where ``d`` lives) of the real symmetric tridiagonal matrix with
    diagonal ``d`` [n] and off-diagonal ``e`` [n-1], for the eigenvalues ``w``
    (ascending, as ``tridiagonal_eigenvalues`` returns them).

    Raises ``RuntimeError`` when a column has not reached the residual
    ``1e-12 * n * max(1, |d|_max, |e|_max)`` after 5 sweeps.
    """
    device = _resolve_device(d, device)
    dh = d.detach().to("cpu", torch.float64).contiguous()
    eh = e.detach().to("cpu", torch.float64).contiguous()
    wh = w.detach().to("cpu", torch.float64).reshape(-1).contiguous()
    n, k = dh.shape[0], wh.shape[0]
    dlaf_assert(dh.dim() == 1 and eh.dim() == 1
                and eh.shape[0] == max(n - 1, 0),
                "tridiagonal: d [n] and e [n-1] required", tuple(d.shape),
                tuple(e.shape))
    dlaf_assert(k <= n, "more eigenvalues than rows", k, n)
    if n == 0 or k == 0:
        return torch.zeros((n, 0), dtype=torch.float64, device=device)
    if n == 1:
        return torch.ones((1, 1), dtype=torch.float64, device=device)
    dlaf_assert(bool((wh[1:] >= wh[:-1]).all()), "w must be ascending")
    nrm = max(float(dh.abs().max()), float(eh.abs().max()))
    if nrm == 0.0:
        return torch.eye(n, k, dtype=torch.float64, device=device)

    # scaled problem: max(|d|, |e|) = 1
    ds, es, ws = dh / nrm, eh / nrm, wh / nrm
    r = ds.abs()
    r[:-1] += es.abs()
    r[1:] += es.abs()
    t1 = float(r.max())
    lam = ws.clone()
    if k > 1 and bool((ws[1:] - ws[:-1] < PERTOL * EPS * t1).any()):
        # sequential by nature (each shift is compared with the perturbed
        # one before it); runs on the host only when some shifts coincide
        ll, step = lam.tolist(), PERTOL * EPS * t1
        for j in range(1, k):
            if ll[j] - ll[j - 1] < step:
                ll[j] = ll[j - 1] + step
        lam = torch.tensor(ll, dtype=torch.float64)
    starts = _cluster_starts(ws, t1)
    by_size = {}
    for a, b in zip(starts[:-1], starts[1:]):
        if b - a > 1:
            by_size.setdefault(b - a, []).append(a)
    groups = sorted(by_size.items())

    gen = torch.Generator(device="cpu").manual_seed(_SEED)
    X = torch.rand((n, k), generator=gen, dtype=torch.float64) * 2.0 - 1.0
    X = X.to(device)
    ds, es, ws, lam = ds.to(device), es.to(device), ws.to(device), lam.to(device)

    if _work_cols is None:
        cols = max(64, (WORK_BYTES // (3 * 8 * n)) // 64 * 64)
    else:
        cols = int(_work_cols)
        dlaf_assert(cols > 0, "_work_cols must be positive", cols)
    cols = min(cols, k)
    work = torch.empty((3, n, cols), dtype=torch.float64, device=device)
    ext = get_ext()
    tol = EPS * t1
    # test bound 1e-12 * n * max(1, nrm) in the units of the scaled problem
    bound = RES_TOL * n * max(1.0, nrm) / nrm
    timer = _StageTimer(device, _timings)
    bad = k
    for it in range(MAX_ITS):
        with timer("solve"):
            for c0 in range(0, k, cols):
                c1 = min(c0 + cols, k)
                ext.tridiag_shifted_solve(ds, es, lam[c0:c1], tol,
                                          X[:, c0:c1], work)
        with timer("orth"):
            X /= torch.linalg.vector_norm(X, dim=0)
            _orthogonalise(X, groups)
        if it + 1 >= MIN_ITS:
            with timer("residual"):
                bad = int((~(_residuals(ds, es, ws, X) <= bound)).sum())
            if bad == 0:
                break
    if _timings is not None:
        _timings["iterations"] = it + 1
        _timings["clusters"] = len(starts) - 1
        _timings["max_cluster"] = max(b - a for a, b in
                                      zip(starts[:-1], starts[1:]))
    if bad:
        raise RuntimeError(
            f"tridiagonal_eigenvectors: {bad} of {k} eigenvectors above the "
            f"residual bound after {MAX_ITS} inverse iterations")
    return X


class _StageTimer:
    """Accumulates synchronised wall time per stage into a dict; a no-op
    (no synchronisation) without one."""

    def __init__(self, device, sink):
        self.device, self.sink = device, sink

    def __call__(self, name):
        self.name = name
        return self

    def __enter__(self):
        if self.sink is not None:
            import time
            self._sync()
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if self.sink is not None:
            import time
            self._sync()
            self.sink[self.name] = (self.sink.get(self.name, 0.0)
                                    + time.perf_counter() - self.t0)
        return False

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)


def tridiagonal_eigensolver_bisect(
        d: torch.Tensor, e: torch.Tensor, index_begin: int = 0,
        index_end: Optional[int] = None, device=None, *,
        _work_cols: Optional[int] = None,
        _timings: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eigenpairs ``index_begin <= k < index_end`` (0-based, ascending) of
    tridiag(d, e): Sturm bisection for the eigenvalues, inverse iteration for
    the eigenvectors. Returns (w [m], Z [n, m]) float64 on ``device``; ``w``
    is bitwise what ``tridiagonal_eigenvalues`` returns for the range.
    """
    device = _resolve_device(d, device)
    timer = _StageTimer(device, _timings)
    with timer("tridiag_bisect"):
        w = tridiagonal_eigenvalues(d, e, index_begin, index_end,
                                    device=device)
    sub = {} if _timings is not None else None
    with timer("tridiag_invit"):
        Z = tridiagonal_eigenvectors(d, e, w, device=device,
                                     _work_cols=_work_cols, _timings=sub)
    if _timings is not None:
        _timings["invit"] = sub
    return w, Z
