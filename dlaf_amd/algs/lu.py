"""LU factorization with partial pivoting, its solves and its condition
estimate: ``?getrf``, ``?getrs``, ``?gesv`` and ``?gecon`` for a local matrix.

``lu_factorization`` is right-looking over tile columns. Per tile column k:

1. the pivoted panel (``ops.lu_panel``; csrc/lu_panel.hip on the device: one
   launch per column, pivots and the zero-pivot record never leave it);
2. the panel's interchanges on the tile columns left and right of it
   (``ops.laswp``), so L ends in final row order as LAPACK stores it;
3. ``U[k, j>k] = inv(L_kk) A[k, j>k]`` against the unit-lower tile inverse
   (TRSM-as-GEMM, one fused launch);
4. ``A[i>k, j>k] -= L[i, k] U[k, j]`` as one fused-GEMM launch with
   descriptors straight off the matrix storage.

The host reads nothing from the device inside that loop; ``info`` is one read
at the end. Pivot rule: the first row of the largest ``|re| + |im|`` (LAPACK's
``i?amax``), on the device and on the CPU alike.

Distributed grids are rejected: the panel kernel addresses one rank's storage.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..types import Side, UpLo, Op, Diag
from ..core.asserts import dlaf_assert
from ..ops import tile_ops as ops
from ..matrix.matrix import Matrix
from ..comm.grid import CommGrid
from .condition import (TriangularVectorSolver, inverse_norm_estimate,
                        _check_square, _grid_of, _has_zero_diagonal, _rcond)
from .triangular import triangular_solver

# Right-hand sides at least this wide take the interchange kernel (one thread
# per column walks the pivots); narrower ones one row gather by the
# permutation vector: n sequential swaps in a handful of threads are the
# wrong shape.
_LASWP_MIN_COLS = 64


def _local_only(A: Matrix, grid: Optional[CommGrid], what: str) -> None:
    d = A.dist
    dlaf_assert(_grid_of(A, grid) is None and d.grid_rows == 1
                and d.grid_cols == 1,
                f"{what} is not implemented on a distributed grid (the "
                "pivoted panel works on one rank's storage); gather the "
                "matrix to one rank", (d.grid_rows, d.grid_cols))


def lu_factorization(A: Matrix,
                     grid: Optional[CommGrid] = None
                     ) -> Tuple[torch.Tensor, int]:
    """``P A = L U`` in place, as ``?getrf``: unit-lower L below the diagonal,
    U on and above it.

    Returns ``(ipiv, info)``. ``ipiv`` is int32 of length n on A's device,
    0-based: row j was interchanged with row ``ipiv[j] >= j``. ``info`` is 0,
    or the 1-based index of the first exactly-zero pivot; the factorization
    is completed regardless (that column is left unscaled)."""
    _check_square(A)
    _local_only(A, grid, "lu_factorization")
    n, nt = A.dist.m, A.dist.nr_tiles[0]
    ipiv = torch.empty(n, dtype=torch.int32, device=A.device)
    if n == 0:
        return ipiv, 0
    dlaf_assert(A.storage.is_contiguous(), "contiguous tile storage required")
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    rowbuf = _row_buffer(A)
    for k in range(nt):
        for step in STEPS:
            step(A, k, ipiv, info, rowbuf)
    return ipiv, int(info.item())


def _row_buffer(A: Matrix) -> Optional[torch.Tensor]:
    nt, nb = A.dist.nr_tiles[0], A.dist.nb
    if nt < 2:
        return None
    return torch.empty((nt - 1, nb, nb), dtype=A.dtype, device=A.device)


def _step_panel(A, k, ipiv, info, rowbuf) -> None:
    ops.lu_panel(A.storage, A.dist.m, k, ipiv, info)


def _step_interchanges(A, k, ipiv, info, rowbuf) -> None:
    n, nb = A.dist.m, A.dist.nb
    s0, s1 = k * nb, min((k + 1) * nb, n)
    ops.laswp(A.storage, ipiv, s0, s1, 0, s0)
    ops.laswp(A.storage, ipiv, s0, s1, s1, n)


def _step_row_solve(A, k, ipiv, info, rowbuf) -> None:
    """U[k, j>k] = inv(L_kk) A[k, j>k], one fused launch and one copy."""
    nt, nb = A.dist.nr_tiles[0], A.dist.nb
    if k + 1 >= nt:
        return
    inv = ops.tri_inverse_full(A.tile((k, k)), lower=True,
                               unit=True).contiguous()
    ops.gemm_items(rowbuf, inv, A.storage,
                   [((j - k - 1) * nb * nb, 0, A.tile_offset((k, j)))
                    for j in range(k + 1, nt)],
                   nb, Op.NoTrans, Op.NoTrans, 1.0, 0.0)
    A.storage[k, k + 1:].copy_(rowbuf[: nt - k - 1])


def _step_trailing(A, k, ipiv, info, rowbuf) -> None:
    """A[i>k, j>k] -= L[i, k] U[k, j]: one fused launch off the storage."""
    nt, nb = A.dist.nr_tiles[0], A.dist.nb
    cols = range(k + 1, nt)
    st = A.storage
    ops.gemm_items(st, st, st,
                   [(A.tile_offset((i, j)), A.tile_offset((i, k)),
                     A.tile_offset((k, j))) for i in cols for j in cols],
                   nb, Op.NoTrans, Op.NoTrans, -1.0, 1.0)


# One tile column of the factorization, in order (tools/bench_lu.py times
# them one by one).
STEPS = (_step_panel, _step_interchanges, _step_row_solve, _step_trailing)


def _permute_rows(B: Matrix, ipiv: torch.Tensor, inverse: bool) -> None:
    """B <- P B (the interchanges in order), or P^T B when ``inverse``."""
    n, nrhs = B.dist.m, B.dist.n
    if n == 0 or nrhs == 0:
        return
    if nrhs >= _LASWP_MIN_COLS:
        ops.laswp(B.storage, ipiv, 0, n, 0, nrhs, reverse=inverse)
        return
    perm = ops.pivots_to_permutation(ipiv).to(B.device)
    b = B.to_global()
    if inverse:
        out = torch.empty_like(b)
        out[perm] = b
    else:
        out = b[perm]
    B.set_from_global(out)


def _check_rhs(LU: Matrix, ipiv: torch.Tensor, B: Matrix) -> None:
    n = LU.dist.m
    dlaf_assert(B.dist.m == n and B.dist.mb == B.dist.nb == LU.dist.nb,
                "B must have n rows and the tile size of the factor",
                B.dist.size, B.dist.tile_size)
    dlaf_assert(ipiv.dim() == 1 and ipiv.shape[0] == n
                and ipiv.dtype == torch.int32, "ipiv must be int32 of "
                "length n", tuple(ipiv.shape), ipiv.dtype)
    dlaf_assert(B.dtype == LU.dtype and B.device == LU.device,
                "B must have the factor's dtype and device", B.dtype,
                B.device)


def lu_solve(op: Op, LU: Matrix, ipiv: torch.Tensor, B: Matrix,
             grid: Optional[CommGrid] = None) -> None:
    """Solve ``op(A) X = B`` in place on B with the factors and the 0-based
    pivots of ``lu_factorization``, as ``?getrs``."""
    _check_square(LU)
    _local_only(LU, grid, "lu_solve")
    _local_only(B, grid, "lu_solve")
    _check_rhs(LU, ipiv, B)
    if LU.dist.m == 0 or B.dist.n == 0:
        return
    ipiv = ipiv.to(LU.device)
    if op == Op.NoTrans:  # A = P^T L U
        _permute_rows(B, ipiv, inverse=False)
        triangular_solver(Side.Left, UpLo.Lower, op, Diag.Unit, 1.0, LU, B)
        triangular_solver(Side.Left, UpLo.Upper, op, Diag.NonUnit, 1.0, LU, B)
    else:  # op(A) = op(U) op(L) P
        triangular_solver(Side.Left, UpLo.Upper, op, Diag.NonUnit, 1.0, LU, B)
        triangular_solver(Side.Left, UpLo.Lower, op, Diag.Unit, 1.0, LU, B)
        _permute_rows(B, ipiv, inverse=True)


def general_solve(A: Matrix, B: Matrix,
                  grid: Optional[CommGrid] = None
                  ) -> Tuple[torch.Tensor, int]:
    """Solve ``A X = B`` as ``?gesv``: A is overwritten by its LU factors, B
    by the solution. Returns ``(ipiv, info)`` of ``lu_factorization``; B is
    left untouched when ``info > 0`` (U is exactly singular)."""
    _check_square(A)
    _local_only(A, grid, "general_solve")
    _local_only(B, grid, "general_solve")
    dlaf_assert(B.dist.m == A.dist.m and B.dist.mb == B.dist.nb == A.dist.nb
                and B.dtype == A.dtype and B.device == A.device,
                "B must have n rows and A's tile size, dtype and device",
                B.dist.size, B.dist.tile_size, B.dtype, B.device)
    ipiv, info = lu_factorization(A)
    if info == 0:
        lu_solve(Op.NoTrans, A, ipiv, B)
    return ipiv, info


def lu_rcond(norm: str, LU: Matrix, anorm: float,
             grid: Optional[CommGrid] = None, method: str = "auto") -> float:
    """Estimated reciprocal condition number, in the one (``"one"``) or
    infinity (``"inf"``) norm, of the matrix whose ``lu_factorization`` is in
    ``LU``, as ``?gecon``. ``anorm`` is that norm of the matrix before it was
    factored (``matrix_norm(norm, A)``).

    The pivots are not needed: ``A^-1 = U^-1 L^-1 P``, and a column
    permutation changes neither norm. 0.0 for a zero on U's diagonal and for
    ``anorm == 0``, 1.0 for an empty matrix (as ``triangular_rcond``)."""
    dlaf_assert(norm in ("one", "inf"), "norm must be 'one' or 'inf'", norm)
    _check_square(LU)
    _local_only(LU, grid, "lu_rcond")
    n = LU.dist.m
    if n == 0:
        return 1.0
    if anorm == 0.0 or _has_zero_diagonal(LU, None):
        return 0.0
    lo = TriangularVectorSolver(UpLo.Lower, Diag.Unit, LU, None, method)
    up = TriangularVectorSolver(UpLo.Upper, Diag.NonUnit, LU, None, method)

    def fwd(x):  # U^-1 L^-1 x
        lo.solve(Op.NoTrans, x)
        up.solve(Op.NoTrans, x)

    def adj(x):  # (U^-1 L^-1)^H x = L^-H U^-H x
        up.solve(Op.ConjTrans, x)
        lo.solve(Op.ConjTrans, x)

    if norm == "inf":  # ||M||_inf = ||M^H||_1
        fwd, adj = adj, fwd
    return _rcond(anorm, inverse_norm_estimate(n, fwd, adj, LU.dtype,
                                               LU.device))
