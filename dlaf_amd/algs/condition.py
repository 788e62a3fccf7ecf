"""Reciprocal condition estimates and the Cholesky solve.

``triangular_rcond`` (``?trcon``) and ``cholesky_rcond`` (``?pocon``) estimate
``1 / (||A|| ||A^-1||)`` without forming the inverse: ``||A||`` is a
``matrix_norm``, ``||A^-1||_1`` comes from Hager / Higham's one-norm estimator
(``inverse_norm_estimate``, LAPACK ``?lacn2`` written as a loop), which needs a
handful of solves with A and A^H for a single vector each.

``TriangularVectorSolver`` is that solve. On a local device matrix it runs the
memory-bound HIP kernel of ``csrc/trsv.hip`` (method ``"kernel"``): the
triangle is read once per solve, the diagonal tiles are applied through their
inverses, computed once per solver. Everywhere else (CPU, distributed grids)
it is ``triangular_solver`` on an ``n x 1`` matrix (method ``"blocked"``).

``cholesky_solve`` (``?potrs``) is the two ``triangular_solver`` calls with
the factor, in place on B.
"""

from __future__ import annotations

from typing import Callable, Optional

import torch

from ..types import Side, UpLo, Op, Diag, is_complex, real_dtype
from ..core.asserts import dlaf_assert
from ..ops._ext import get_ext
from ..ops import tile_ops as ops
from ..matrix.matrix import Matrix
from ..comm.grid import CommGrid
from ..comm import collectives as coll
from .norm import matrix_norm
from .triangular import triangular_solver

_METHODS = ("auto", "kernel", "blocked")
_OP_CODE = {Op.NoTrans: 0, Op.Trans: 1, Op.ConjTrans: 2}
_ITMAX = 5  # ?lacn2's iteration limit


def _grid_of(A: Matrix, grid: Optional[CommGrid]) -> Optional[CommGrid]:
    g = grid if grid is not None else A.grid
    return g if g is not None and g.distributed else None


def _check_square(A: Matrix) -> None:
    d = A.dist
    dlaf_assert(d.m == d.n and d.mb == d.nb,
                "square matrix with square tiles required", d.size,
                d.tile_size)


class TriangularVectorSolver:
    """Solves ``op(T) x = b`` for single vectors, T the ``uplo`` triangle of
    ``A`` (``Diag.Unit``: the stored diagonal is ignored).

    ``method``: ``"kernel"`` (HIP kernel; local device matrix only),
    ``"blocked"`` (``triangular_solver`` on an ``n x 1`` matrix; anywhere) or
    ``"auto"`` (the kernel where it can run). The solver reads ``A`` as it is
    when constructed: the kernel path keeps the inverses of its diagonal
    tiles for all later solves.
    """

    def __init__(self, uplo: UpLo, diag: Diag, A: Matrix,
                 grid: Optional[CommGrid] = None, method: str = "auto"):
        dlaf_assert(method in _METHODS, "method must be one of", _METHODS,
                    method)
        dlaf_assert(uplo in (UpLo.Lower, UpLo.Upper), "bad uplo", uplo)
        _check_square(A)
        self.uplo, self.diag, self.A = uplo, diag, A
        self.grid = _grid_of(A, grid)
        d = A.dist
        local = (self.grid is None and d.grid_rows == 1 and d.grid_cols == 1)
        can_kernel = local and A.device.type == "cuda"
        if method == "auto":
            method = "kernel" if can_kernel else "blocked"
        dlaf_assert(method != "kernel" or can_kernel,
                    "method='kernel' needs a local matrix on the device",
                    A.device, (d.grid_rows, d.grid_cols))
        self.method = method
        self.n = d.m
        if method == "kernel" and self.n > 0:
            nt = d.nr_tiles[0]
            invs = ops.tri_inverse_full_many(
                (A.tile((k, k)) for k in range(nt)),
                lower=uplo == UpLo.Lower, unit=diag == Diag.Unit)
            self._dinv = torch.stack(invs)
            self._storage = A.storage.contiguous()
            self._xpad = torch.zeros(nt * d.nb, dtype=A.dtype,
                                     device=A.device)

    def solve(self, op: Op, x: torch.Tensor) -> torch.Tensor:
        """In place on the 1-D tensor ``x`` (length n, the same on every
        rank); returns ``x``."""
        dlaf_assert(x.dim() == 1 and x.shape[0] == self.n
                    and x.dtype == self.A.dtype, "x must be a vector of "
                    "length n of the matrix's dtype", tuple(x.shape), x.dtype)
        if self.n == 0:
            return x
        if self.method == "kernel":
            dlaf_assert(x.device == self._xpad.device, "x must be on the "
                        "matrix's device", x.device, self._xpad.device)
            xp = self._xpad
            xp[: self.n] = x
            # a missing kernel is an error: get_ext() raises
            get_ext().trsv_tiles(self._storage, self._dinv, xp, self.n,
                                 int(self.uplo == UpLo.Upper), _OP_CODE[op])
            x.copy_(xp[: self.n])
            return x
        nb = self.A.dist.nb
        B = Matrix.create(self.n, 1, nb, nb, dtype=self.A.dtype,
                          device=self.A.device, grid=self.grid)
        B.set_from_global(x[:, None])
        triangular_solver(Side.Left, self.uplo, op, self.diag, 1.0, self.A, B,
                          self.grid)
        x.copy_(B.to_global()[:, 0])  # all-reduced on a grid
        return x


def _sign(x: torch.Tensor) -> torch.Tensor:
    """?lacn2's sign vector: +-1 (real), x / |x| or 1 (complex)."""
    if x.is_complex():
        ax = x.abs()
        tiny = torch.finfo(x.dtype).tiny
        one = torch.ones((), dtype=x.dtype, device=x.device)
        return torch.where(ax > tiny, x / ax.clamp_min(tiny), one)
    # sign(0) = +1, as the LAPACK builds in use have it
    return torch.where(x >= 0, 1.0, -1.0).to(x.dtype)


def inverse_norm_estimate(n: int, solve: Callable[[torch.Tensor], object],
                          solve_h: Callable[[torch.Tensor], object],
                          dtype: torch.dtype, device) -> float:
    """Estimate of ``||A^-1||_1`` (never above it in exact arithmetic).

    ``solve(x)`` overwrites the vector x with ``A^-1 x``, ``solve_h(x)`` with
    ``A^-H x``. The loop is ``dlacn2`` / ``zlacn2``: at most five
    iterations of Hager's method with Higham's alternating-sign safeguard.
    """
    if n <= 0:
        return 0.0
    cplx = is_complex(dtype)
    x = torch.full((n,), 1.0 / n, dtype=dtype, device=device)
    solve(x)
    if n == 1:
        return float(x.abs().item())
    est = float(x.abs().sum().item())
    sgn = _sign(x)
    x = sgn.clone()
    solve_h(x)
    j = int(x.abs().argmax().item())
    for it in range(2, _ITMAX + 1):
        x.zero_()
        x[j] = 1
        solve(x)
        est_old = est
        est = float(x.abs().sum().item())
        new_sgn = _sign(x)
        if not cplx and bool((new_sgn == sgn).all().item()):
            break  # repeated sign vector: converged
        if est <= est_old:
            break
        sgn = new_sgn
        x = sgn.clone()
        solve_h(x)
        ax = x.abs()
        jlast, j = j, int(ax.argmax().item())
        # real: x[jlast] itself against |x[j]|, as dlacn2 has it
        last = ax[jlast] if cplx else x[jlast]
        if float(last.item()) == float(ax[j].item()):
            break
    # x_i = (-1)^i (1 + i / (n - 1))
    i = torch.arange(n, dtype=torch.float64, device=device)
    alt = (1.0 + i / (n - 1)) * (1.0 - 2.0 * (i % 2))
    x = alt.to(dtype)
    solve(x)
    return max(est, 2.0 * float(x.abs().sum().item()) / (3.0 * n))


def _has_zero_diagonal(A: Matrix, grid: Optional[CommGrid]) -> bool:
    d = A.dist
    found = torch.zeros((), dtype=torch.float64, device=A.device)
    for k in range(d.nr_tiles[0]):
        if d.rank_of_tile((k, k)) != (d.rank_row, d.rank_col):
            continue
        if bool((A.tile_logical((k, k)).diagonal() == 0).any()):
            found.fill_(1.0)
            break
    if grid is not None:
        coll.all_reduce_max(found, grid.full_group)
    return bool(found.item())


def _rcond(anorm: float, ainvnm: float) -> float:
    if ainvnm == 0.0:
        return 0.0
    return (1.0 / ainvnm) / anorm


def triangular_rcond(norm: str, uplo: UpLo, diag: Diag, A: Matrix,
                     grid: Optional[CommGrid] = None,
                     method: str = "auto") -> float:
    """Estimated reciprocal condition number of the triangular matrix in the
    ``uplo`` triangle of ``A`` in the one (``"one"``) or infinity (``"inf"``)
    norm, as ``?trcon``; the same float on every rank. 0.0 when a non-unit
    diagonal entry is exactly zero, 1.0 for an empty matrix."""
    dlaf_assert(norm in ("one", "inf"), "norm must be 'one' or 'inf'", norm)
    _check_square(A)
    n = A.dist.m
    if n == 0:
        return 1.0
    g = _grid_of(A, grid)
    if diag == Diag.NonUnit and _has_zero_diagonal(A, g):
        return 0.0
    anorm = matrix_norm(norm, A, uplo=uplo, structure="triangular", diag=diag,
                        grid=g)
    if not anorm > 0.0:
        return 0.0
    sv = TriangularVectorSolver(uplo, diag, A, g, method)
    fwd = lambda x: sv.solve(Op.NoTrans, x)  # noqa: E731
    adj = lambda x: sv.solve(Op.ConjTrans, x)  # noqa: E731
    if norm == "inf":  # ||A^-1||_inf = ||A^-H||_1
        fwd, adj = adj, fwd
    return _rcond(anorm, inverse_norm_estimate(n, fwd, adj, A.dtype,
                                               A.device))


def cholesky_rcond(uplo: UpLo, L: Matrix, anorm: float,
                   grid: Optional[CommGrid] = None,
                   method: str = "auto") -> float:
    """Estimated reciprocal one-norm condition number of the Hermitian
    positive definite matrix whose Cholesky factor is in the ``uplo`` triangle
    of ``L``, as ``?pocon``; the same float on every rank.

    ``anorm`` is the one-norm of the matrix before it was factored:
    ``matrix_norm("one", A, structure="hermitian", uplo=uplo)``. 0.0 for
    ``anorm == 0``, 1.0 for an empty matrix."""
    _check_square(L)
    n = L.dist.m
    if n == 0:
        return 1.0
    if anorm == 0.0:
        return 0.0
    g = _grid_of(L, grid)
    sv = TriangularVectorSolver(uplo, Diag.NonUnit, L, g, method)
    first, second = ((Op.NoTrans, Op.ConjTrans) if uplo == UpLo.Lower
                     else (Op.ConjTrans, Op.NoTrans))

    def solve(x):  # (L L^H)^-1 x, or (U^H U)^-1 x
        sv.solve(first, x)
        sv.solve(second, x)

    return _rcond(anorm, inverse_norm_estimate(n, solve, solve, L.dtype,
                                               L.device))


def cholesky_solve(uplo: UpLo, L: Matrix, B: Matrix,
                   grid: Optional[CommGrid] = None) -> None:
    """Solve A X = B in place on B with the Cholesky factor of A in the
    ``uplo`` triangle of ``L`` (``A = L L^H`` or ``U^H U``), as ``?potrs``."""
    first, second = ((Op.NoTrans, Op.ConjTrans) if uplo == UpLo.Lower
                     else (Op.ConjTrans, Op.NoTrans))
    for op in (first, second):
        triangular_solver(Side.Left, uplo, op, Diag.NonUnit, 1.0, L, B, grid)


def warn_if_ill_conditioned(uplo: UpLo, L: Matrix, anorm: float,
                            grid: Optional[CommGrid], what: str) -> float:
    """RuntimeWarning when the estimated rcond of the factored matrix is
    below the precision of its dtype (or is not a number)."""
    import warnings
    rcond = cholesky_rcond(uplo, L, anorm, grid)
    eps = torch.finfo(real_dtype(L.dtype)).eps
    if not rcond >= eps:
        warnings.warn(f"{what} is ill-conditioned: estimated rcond = "
                      f"{rcond:.3e} < eps = {eps:.3e}", RuntimeWarning,
                      stacklevel=3)
    return rcond
