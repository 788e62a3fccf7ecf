"""Iterative refinement, error bounds and the mixed-precision solve for
Hermitian positive definite systems.

``cholesky_refine`` (``?porfs``) improves a computed solution of ``A X = B``
and returns, per right-hand side, the componentwise backward error ``berr``
and a bound ``ferr`` on the relative forward error. ``cholesky_solve_expert``
(``?posvx`` with ``fact='N'``) is norm, factorization, ``cholesky_rcond``,
``cholesky_solve`` and ``cholesky_refine`` in one call.
``cholesky_solve_mixed`` (``dsposv`` / ``zcposv``) factors in single
precision, where the matrix rate is twice the double one, and refines the
solution to double precision accuracy.

All three rest on ``HermitianVectorProduct``: ``y = A x`` and, from the same
pass over the stored triangle, ``|A| |x|``. On a local device matrix it is
the memory-bound HIP kernel of ``csrc/hemv.hip`` (method ``"kernel"``), which
reads the triangle once; everywhere else (CPU, distributed grids) it is
``hermitian_multiplication`` on an ``n x 1`` matrix (method ``"blocked"``).
``|.|`` of a complex number is LAPACK's ``CABS1``, ``|re| + |im|``.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from ..types import Side, UpLo, Op, Diag, is_complex, real_dtype
from ..core.asserts import dlaf_assert
from ..ops._ext import get_ext
from ..matrix.matrix import Matrix
from ..comm.grid import CommGrid
from .norm import matrix_norm
from .cholesky import cholesky_factorization
from .multiplication import hermitian_multiplication
from .condition import (_METHODS, _grid_of, _check_square,
                        TriangularVectorSolver, inverse_norm_estimate,
                        cholesky_rcond, cholesky_solve)

_ITMAX = 5  # ?porfs' refinement limit
# cholesky_solve_mixed works column by column on the vector kernels up to this
# many right-hand sides, on hermitian_multiplication and triangular_solver
# above. Measured (docs/DESIGN.md): the product kernel stays ahead of
# hermitian_multiplication up to about 40 columns at n = 16384 .. 32768.
MIXED_KERNEL_MAX_NRHS = 32

_DEMOTED = {torch.float64: torch.float32, torch.complex128: torch.complex64}
_PROMOTED = {low: high for high, low in _DEMOTED.items()}


def _lapack_eps(dtype: torch.dtype) -> float:
    """LAPACK's ``?lamch('Epsilon')``: half of the spacing at 1."""
    return 0.5 * torch.finfo(real_dtype(dtype)).eps


def _cabs1(x: torch.Tensor) -> torch.Tensor:
    return x.real.abs() + x.imag.abs() if x.is_complex() else x.abs()


def cholesky_info(mat: Matrix, grid: Optional[CommGrid] = None) -> int:
    """``info`` of a Cholesky factorization left in ``mat``: 0, or the order
    of the first leading minor that was not positive definite (its pivot's
    square root left a NaN on the diagonal). An O(n) scan of the diagonal.

    On a grid each rank scans the diagonal tiles it owns and the smallest
    positive info is all-reduced, so every rank returns the same value."""
    info = 0
    nt = mat.dist.nr_tiles[0]
    for k in range(nt):
        if mat.dist.rank_of_tile((k, k)) != (mat.dist.rank_row, mat.dist.rank_col):
            continue
        d = mat.tile((k, k)).diagonal()
        bad = torch.isnan(d.real if d.is_complex() else d)
        if bool(bad.any()):
            info = k * mat.dist.mb + int(bad.int().argmax()) + 1
            break
    if grid is not None and grid.distributed:
        import torch.distributed as tdist
        # min over positive infos == first failing pivot; encode 0 as +inf
        t = torch.tensor([float(info) if info > 0 else float("inf")],
                         dtype=torch.float64)
        tdist.all_reduce(t, op=tdist.ReduceOp.MIN, group=grid.full_group)
        v = float(t.item())
        info = 0 if v == float("inf") else int(v)
    return info


class HermitianVectorProduct:
    """``y = A x`` for single vectors, A the Hermitian matrix whose ``uplo``
    triangle is stored in ``A``; with ``want_abs`` also ``|A| |x|``.

    ``method``: ``"kernel"`` (HIP kernel; local device matrix only),
    ``"blocked"`` (``hermitian_multiplication`` on an ``n x 1`` matrix;
    anywhere) or ``"auto"`` (the kernel where it can run). The kernel reads
    the stored triangle once per call, never the other triangle, the
    imaginary part of the diagonal or the padding, and accumulates single
    precision in double. The blocked method keeps that precision contract
    with copies it builds on first use and keeps: a double precision copy of
    a single precision ``A`` for ``A x``, and a real ``CABS1`` copy for
    ``|A| |x|``. That multiplies the memory of the matrix on this fallback
    path, which is accepted; the copies hold ``A`` as it was when they were
    built. The kernel reads ``A``'s storage at each call.
    """

    def __init__(self, uplo: UpLo, A: Matrix, grid: Optional[CommGrid] = None,
                 method: str = "auto"):
        dlaf_assert(method in _METHODS, "method must be one of", _METHODS,
                    method)
        dlaf_assert(uplo in (UpLo.Lower, UpLo.Upper), "bad uplo", uplo)
        _check_square(A)
        self.uplo, self.A = uplo, A
        self.grid = _grid_of(A, grid)
        d = A.dist
        can_kernel = self.can_run_kernel(A, grid)
        if method == "auto":
            method = "kernel" if can_kernel else "blocked"
        dlaf_assert(method != "kernel" or can_kernel,
                    "method='kernel' needs a local matrix on the device",
                    A.device, (d.grid_rows, d.grid_cols))
        self.method = method
        self.n = d.m
        self._wide: Optional[Matrix] = None
        self._abs: Optional[Matrix] = None
        if method == "kernel" and self.n > 0:
            pad = d.nr_tiles[0] * d.nb
            self._storage = A.storage.contiguous()
            self._xpad = torch.zeros(pad, dtype=A.dtype, device=A.device)
            self._ypad = torch.zeros(pad, dtype=A.dtype, device=A.device)
            self._apad = torch.zeros(pad, dtype=real_dtype(A.dtype),
                                     device=A.device)
            self._none = torch.empty(0, dtype=real_dtype(A.dtype),
                                     device=A.device)

    @staticmethod
    def can_run_kernel(A: Matrix, grid: Optional[CommGrid] = None) -> bool:
        d = A.dist
        return (_grid_of(A, grid) is None and d.grid_rows == 1
                and d.grid_cols == 1 and A.device.type == "cuda")

    def _wide_matrix(self) -> Matrix:
        if self._wide is None:
            A = self.A
            self._wide = A if A.dtype in _DEMOTED else A.astype(_PROMOTED[A.dtype])
        return self._wide

    def _abs_matrix(self) -> Matrix:
        if self._abs is None:
            A = self._wide_matrix()
            d = A.dist
            m = Matrix(d, real_dtype(A.dtype), A.device, A.grid,
                       _storage=_cabs1(A.storage))
            if is_complex(A.dtype):  # the diagonal counts as |Re a_ii|
                for k in range(d.nr_tiles[0]):
                    if d.rank_of_tile((k, k)) == (d.rank_row, d.rank_col):
                        m.tile((k, k)).diagonal().copy_(
                            A.tile((k, k)).diagonal().real.abs())
            self._abs = m
        return self._abs

    def _blocked(self, A: Matrix, x: torch.Tensor) -> torch.Tensor:
        nb = A.dist.nb
        X = Matrix.create(self.n, 1, nb, nb, dtype=A.dtype, device=A.device,
                          grid=self.grid)
        Y = X.like()
        X.set_from_global(x[:, None])
        hermitian_multiplication(Side.Left, self.uplo, 1.0, A, X, 0.0, Y,
                                 self.grid)
        return Y.to_global()[:, 0]  # all-reduced on a grid

    def apply(self, x: torch.Tensor, want_abs: bool = False):
        """``A x`` for the 1-D tensor ``x`` (length n, the same on every
        rank), or ``(A x, |A| |x|)`` with ``want_abs``; new tensors."""
        dlaf_assert(x.dim() == 1 and x.shape[0] == self.n
                    and x.dtype == self.A.dtype, "x must be a vector of "
                    "length n of the matrix's dtype", tuple(x.shape), x.dtype)
        rdt = real_dtype(self.A.dtype)
        if self.n == 0:
            y = torch.zeros_like(x)
            return (y, torch.zeros(0, dtype=rdt, device=x.device)) \
                if want_abs else y
        if self.method == "kernel":
            dlaf_assert(x.device == self._xpad.device, "x must be on the "
                        "matrix's device", x.device, self._xpad.device)
            self._xpad[: self.n] = x
            # a missing kernel is an error: get_ext() raises
            get_ext().hemv_tiles(self._storage, self._xpad, self._ypad,
                                 self._apad if want_abs else self._none,
                                 self.n, int(self.uplo == UpLo.Upper))
            y = self._ypad[: self.n].clone()
            return (y, self._apad[: self.n].clone()) if want_abs else y
        wide = self._wide_matrix()
        xw = x.to(wide.dtype)
        y = self._blocked(wide, xw).to(x.dtype)
        if not want_abs:
            return y
        return y, self._blocked(self._abs_matrix(), _cabs1(xw)).to(rdt)


def _potrs_ops(uplo: UpLo):
    return ((Op.NoTrans, Op.ConjTrans) if uplo == UpLo.Lower
            else (Op.ConjTrans, Op.NoTrans))


def cholesky_refine(uplo: UpLo, A: Matrix, L: Matrix, B: Matrix, X: Matrix,
                    grid: Optional[CommGrid] = None,
                    method: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """Improve the solution ``X`` (n x nrhs, in place) of ``A X = B`` by
    iterative refinement and return ``(ferr, berr)``, as ``?porfs``.

    ``A`` is the Hermitian positive definite matrix (its ``uplo`` triangle),
    ``L`` its Cholesky factor as ``cholesky_factorization`` leaves it; both
    and ``B`` are only read. ``berr[j]`` is the componentwise relative
    backward error of column j, ``ferr[j]`` an estimated bound on
    ``||x_j - x_true||_inf / ||x_j||_inf``; float64 CPU tensors of length
    nrhs, the same on every rank.

    The loop is ``dporfs`` / ``zporfs``: at most five corrections per column,
    continued while ``berr > eps`` and ``berr`` at least halves; the forward
    bound is the one-norm estimate (``inverse_norm_estimate``) of
    ``diag(w) inv(A)``, ``w = |r| + (n + 1) eps (|A| |x| + |b|)``, over
    ``||x||_inf``. Each step reads A once (``HermitianVectorProduct``) and
    solves with the factor twice (``TriangularVectorSolver``).
    """
    _check_square(A)
    _check_square(L)
    n, nrhs = A.dist.m, B.dist.n
    dlaf_assert(L.dist.m == n and B.dist.m == n and X.dist.size == B.dist.size,
                "shapes of A, L, B, X do not match", A.dist.size, L.dist.size,
                B.dist.size, X.dist.size)
    ferr = torch.zeros(nrhs, dtype=torch.float64)
    berr = torch.zeros(nrhs, dtype=torch.float64)
    if n == 0 or nrhs == 0:
        return ferr, berr
    g = _grid_of(A, grid)
    hv = HermitianVectorProduct(uplo, A, g, method)
    sv = TriangularVectorSolver(uplo, Diag.NonUnit, L, g, method)
    first, second = _potrs_ops(uplo)

    def potrs(v):
        sv.solve(first, v)
        sv.solve(second, v)

    eps = _lapack_eps(A.dtype)
    safmin = torch.finfo(real_dtype(A.dtype)).tiny
    nz = n + 1
    safe1 = nz * safmin
    safe2 = safe1 / eps
    Bg, Xg = B.to_global(), X.to_global()
    for j in range(nrhs):
        b, x = Bg[:, j], Xg[:, j].clone()
        absb = _cabs1(b)
        count, lstres = 1, 3.0
        while True:
            ax, aabs = hv.apply(x, want_abs=True)
            r = b - ax
            w = aabs + absb
            absr = _cabs1(r)
            big = w > safe2
            s = float(torch.where(big, absr / torch.where(big, w, 1.0),
                                  (absr + safe1) / (w + safe1)).max().item())
            berr[j] = s
            if s > eps and 2.0 * s <= lstres and count <= _ITMAX:
                potrs(r)
                x += r
                lstres = s
                count += 1
                continue
            break
        w = absr + nz * eps * w
        w[~big] += safe1
        wv = w.to(A.dtype)

        def op(v):  # diag(w) inv(A) v
            potrs(v)
            v.mul_(wv)

        def op_h(v):  # its conjugate transpose, inv(A) diag(w) v
            v.mul_(wv)
            potrs(v)

        f = inverse_norm_estimate(n, op, op_h, A.dtype, A.device)
        xmax = float(_cabs1(x).max().item())
        ferr[j] = f / xmax if xmax != 0.0 else f
        Xg[:, j] = x
    X.set_from_global(Xg)
    return ferr, berr


def cholesky_solve_expert(uplo: UpLo, A: Matrix, B: Matrix,
                          grid: Optional[CommGrid] = None,
                          method: str = "auto"):
    """Solve ``A X = B`` for Hermitian positive definite ``A`` with condition
    estimate and error bounds, as ``?posvx`` with ``fact='N'`` (no
    equilibration). Returns ``(X, L, rcond, ferr, berr, info)``: the refined
    solution, the Cholesky factor, the estimated reciprocal one-norm
    condition number and ``cholesky_refine``'s bounds. ``info > 0``: the
    leading minor of that order is not positive definite (``X`` is None,
    ``rcond`` 0); ``info = n + 1``: ``rcond`` is below the machine epsilon,
    the solution and bounds are returned all the same. ``A`` and ``B`` are
    only read."""
    _check_square(A)
    n, nrhs = A.dist.m, B.dist.n
    g = _grid_of(A, grid)
    anorm = matrix_norm("one", A, structure="hermitian", uplo=uplo, grid=g)
    L = A.clone()
    cholesky_factorization(uplo, L, g)
    info = cholesky_info(L, g)
    if info > 0:
        zeros = torch.zeros(nrhs, dtype=torch.float64)
        return None, L, 0.0, zeros, zeros.clone(), info
    rcond = cholesky_rcond(uplo, L, anorm, g, method)
    X = B.clone()
    cholesky_solve(uplo, L, X, g)
    ferr, berr = cholesky_refine(uplo, A, L, B, X, g, method)
    if rcond < _lapack_eps(A.dtype):
        info = n + 1
    return X, L, rcond, ferr, berr, info


def cholesky_solve_mixed(uplo: UpLo, A: Matrix, B: Matrix,
                         grid: Optional[CommGrid] = None,
                         itermax: int = 30):
    """Solve ``A X = B`` (float64 or complex128) with a single precision
    Cholesky factorization and refinement in double precision, as ``dsposv``
    / ``zcposv``. Returns ``(X, iters, info)``.

    ``iters >= 0``: that many refinement steps reached
    ``||b_j - A x_j||_inf <= ||x_j||_inf ||A||_inf eps sqrt(n)`` for every
    column. ``iters < 0``: the solution comes from a double precision
    factorization instead, because an entry overflows single precision
    (``-2``), the single precision factorization failed (``-3``) or the
    refinement did not converge in ``itermax`` steps (``-(itermax + 1)``,
    ``-31`` by default). ``info`` is 0 or the failed pivot of the double
    precision factorization (then ``X`` is None). ``A`` and ``B`` are only
    read: unlike LAPACK, the double precision factor of the fallback is not
    left in ``A``."""
    dlaf_assert(A.dtype in _DEMOTED and B.dtype == A.dtype,
                "float64 or complex128 required", A.dtype, B.dtype)
    _check_square(A)
    n, nrhs = A.dist.m, B.dist.n
    dlaf_assert(B.dist.m == n, "shapes of A and B do not match", A.dist.size,
                B.dist.size)
    if n == 0 or nrhs == 0:
        return B.clone(), 0, 0
    g = _grid_of(A, grid)
    X, iters = _mixed_refine(uplo, A, B, g, itermax)
    if iters >= 0:
        return X, iters, 0
    # double precision all the way
    L = A.clone()
    cholesky_factorization(uplo, L, g)
    info = cholesky_info(L, g)
    if info > 0:
        return None, iters, info
    X = B.clone()
    cholesky_solve(uplo, L, X, g)
    return X, iters, 0


def _mixed_refine(uplo, A, B, g, itermax):
    """``(X, iters)`` when single precision refinement converges, else
    ``(None, negative code)``."""
    n, nrhs = A.dist.m, B.dist.n
    low = _DEMOTED[A.dtype]
    fmax = torch.finfo(real_dtype(low)).max
    amax = matrix_norm("max", A, structure="hermitian", uplo=uplo, grid=g)
    bmax = matrix_norm("max", B, grid=g)
    if not (amax <= fmax and bmax <= fmax):
        return None, -2
    Ls = A.astype(low)
    cholesky_factorization(uplo, Ls, g)
    if cholesky_info(Ls, g) > 0:
        return None, -3
    anrm = matrix_norm("inf", A, structure="hermitian", uplo=uplo, grid=g)
    cte = anrm * _lapack_eps(A.dtype) * math.sqrt(n)
    # few right-hand sides on a local device matrix: the residual and the
    # corrections run column by column on the vector kernels, which read a
    # triangle once per column; otherwise on the tiled HEMM and TRSM
    by_vector = (HermitianVectorProduct.can_run_kernel(A, g)
                 and nrhs <= MIXED_KERNEL_MAX_NRHS)
    if by_vector:
        hv = HermitianVectorProduct(uplo, A, g, "kernel")
        sv = TriangularVectorSolver(uplo, Diag.NonUnit, Ls, g, "kernel")
    first, second = _potrs_ops(uplo)

    def residual(X: Matrix) -> Matrix:  # B - A X in double
        R = B.clone()
        if by_vector:
            Xg, Rg = X.to_global(), R.to_global()
            for j in range(nrhs):
                Rg[:, j] -= hv.apply(Xg[:, j].contiguous())
            R.set_from_global(Rg)
        else:
            hermitian_multiplication(Side.Left, uplo, -1.0, A, X, 1.0, R, g)
        return R

    def colmax(M: Matrix) -> torch.Tensor:  # CABS1 max per column
        return _cabs1(M.to_global()).amax(dim=0)

    def correction(R: Matrix) -> Matrix:  # inv(A) R through single precision
        Rs = R.astype(low)
        if by_vector:
            Rg = Rs.to_global()
            for j in range(nrhs):
                v = Rg[:, j].contiguous()
                sv.solve(first, v)
                sv.solve(second, v)
                Rg[:, j] = v
            Rs.set_from_global(Rg)
        else:
            cholesky_solve(uplo, Ls, Rs, g)
        return Rs.astype(A.dtype)

    X = correction(B)
    for it in range(itermax + 1):
        R = residual(X)
        if bool((colmax(R) <= colmax(X) * cte).all().item()):
            return X, it
        if it == itermax:
            break
        X.storage.add_(correction(R).storage)
        X._set_identity_pad()
    return None, -(itermax + 1)
