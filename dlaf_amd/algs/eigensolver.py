"""Symmetric/Hermitian (generalized) eigensolver pipeline.

Counterpart of ``eigensolver/eigensolver/impl.h:37-105`` (HEEV: red2band ->
band2tridiag -> tridiag D&C -> bt_band2tridiag -> bt_red2band, with partial
spectrum) and ``eigensolver/gen_eigensolver/impl.h:30-104`` (HEGV: chol(B) ->
hegst -> heev -> triangular back-substitution).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..types import UpLo, Op, Side, Diag
from ..matrix.matrix import Matrix
from ..comm.grid import CommGrid
from .red2band import reduction_to_band, bt_reduction_to_band
from .band2tridiag import band_to_tridiagonal, bt_band_to_tridiagonal
from .tridiag_dc import tridiagonal_eigensolver
from .tridiag_bisect import _real_dtype, _resolve_value_range, _setup
from .tridiag_invit import tridiagonal_eigensolver_bisect
from .cholesky import cholesky_factorization
from .gen_to_std import generalized_to_standard
from .triangular import triangular_solver
from .norm import matrix_norm
from .condition import warn_if_ill_conditioned
from . import _scaling


def get_band_size(nb: int) -> int:
    """Band size for the two-stage reduction (reference
    ``eigensolver/internal/get_band_size.h:9-20``: nb/divisor >= min_band=100)."""
    band = nb
    d = 2
    # measured on MI355X: band 64 balances the CPU chase (O(n^2 b)) against
    # the GPU back-transform better than the reference's >=100 floor
    while band % d == 0 and band // d >= 64:
        band //= d
    if band == nb and nb > 128:
        # non-power-of-two nb: fall back to the largest divisor-ish cut
        for cand in (128, 96, 112, 100):
            if nb % cand == 0:
                return cand
    return band


def hermitian_eigensolver(
    uplo: UpLo,
    mat: Matrix,
    grid: Optional[CommGrid] = None,
    band: Optional[int] = None,
    eigenvalues_index_begin: int = 0,
    eigenvalues_index_end: Optional[int] = None,
    tridiag_solver: str = "dc",
    eigenvalues_value_range: Optional[Tuple[float, float]] = None,
) -> Tuple[torch.Tensor, Matrix]:
    """Eigendecomposition A = E diag(w) E^H of a Hermitian tiled matrix.

    ``mat`` is overwritten (band + reflectors). Returns (w [real tensor],
    E [Matrix, same dtype/device/grid]); the partial-spectrum indices select
    eigenvector columns (back-transforms applied only to the slice, the
    reference's MatrixRef mechanism).

    ``tridiag_solver`` picks the tridiagonal stage: ``"dc"`` (default) solves
    the whole tridiagonal problem by divide and conquer and slices;
    ``"bisect"`` computes only the selected eigenpairs by Sturm bisection and
    inverse iteration in O(n*k) memory (local grids only), with eigenvalues
    bitwise equal to ``hermitian_eigenvalues``.

    ``eigenvalues_value_range=(vl, vu)`` selects the eigenvalues in the
    HALF-OPEN interval ``[vl, vu)`` instead of an index range (the two are
    mutually exclusive), as in ``hermitian_eigenvalues``.

    Safe at any scale: a matrix whose max-norm is outside the safe range of
    its real type is scaled by a power of two first and the eigenvalues are
    scaled back (``_scaling.py``); inside the range nothing is touched.
    """
    e = 0
    d = mat.dist
    if uplo == UpLo.Lower and d.m == d.n and d.mb == d.nb:
        e = _scaling.scale_hermitian(
            mat, grid if grid is not None else mat.grid)
    w, evecs = _hermitian_eigensolver(
        uplo, mat, grid, band, eigenvalues_index_begin, eigenvalues_index_end,
        tridiag_solver, _scaling.scale_range(eigenvalues_value_range, e))
    return (_scaling.scale_values(w, -e) if e else w), evecs


def _hermitian_eigensolver(uplo, mat, grid, band, eigenvalues_index_begin,
                           eigenvalues_index_end, tridiag_solver,
                           eigenvalues_value_range):
    """``hermitian_eigensolver`` on a matrix already in the safe range."""
    from ..core.asserts import dlaf_assert
    dlaf_assert(uplo == UpLo.Lower,
                "only Lower implemented (as the reference miniapps)")
    d = mat.dist
    dlaf_assert(d.m == d.n and d.mb == d.nb,
                "square matrix with square tiles required", d.size,
                d.tile_size)
    dlaf_assert(tridiag_solver in ("dc", "bisect"),
                "tridiag_solver must be 'dc' or 'bisect'", tridiag_solver)
    dlaf_assert(eigenvalues_value_range is None
                or (eigenvalues_index_begin == 0
                    and eigenvalues_index_end is None),
                "eigenvalues_value_range excludes an index range")
    n = d.m
    g = grid if grid is not None else mat.grid
    if band is None:
        band = get_band_size(d.nb)
    band = max(1, min(band, max(n - 1, 1)))
    distributed = g is not None and g.distributed
    if distributed and d.nb % band != 0:
        # the tiled distributed panels must stay inside one tile column;
        # snap to the largest divisor of nb not above the requested band
        # (reference: get_band_size.h guarantees divisibility by
        # construction — this keeps arbitrary user bands off a dense cliff)
        band = max(bb for bb in range(1, band + 1) if d.nb % bb == 0)
    if n <= max(band, d.nb):
        # tiny problem (at or below one tile/band): direct dense
        # eigendecomposition
        return _eigh_direct(mat, g, eigenvalues_index_begin,
                            eigenvalues_index_end, eigenvalues_value_range)
    if g is not None and g.distributed:
        import os
        dlaf_assert(tridiag_solver == "dc",
                    "tridiag_solver='bisect' is not implemented on a "
                    "distributed grid (eigenvalue clusters cross the "
                    "eigenvector stripes); use 'dc'")
        if os.environ.get("DLAF_DIST_EIG", "tiled") == "replicated":
            dlaf_assert(eigenvalues_value_range is None,
                        "eigenvalues_value_range needs the tiled "
                        "distributed pipeline")
            # round-1 replicated-dense design, kept as a debug fallback
            from .eigensolver_dist import hermitian_eigensolver_dist
            return hermitian_eigensolver_dist(
                uplo, mat, g, band,
                eigenvalues_index_begin=eigenvalues_index_begin,
                eigenvalues_index_end=eigenvalues_index_end)
        from .eigensolver_tiled import hermitian_eigensolver_tiled
        return hermitian_eigensolver_tiled(
            uplo, mat, g, band,
            eigenvalues_index_begin=eigenvalues_index_begin,
            eigenvalues_index_end=eigenvalues_index_end,
            eigenvalues_value_range=eigenvalues_value_range)
    ib = eigenvalues_index_begin
    ie = n if eigenvalues_index_end is None else eigenvalues_index_end

    refl = reduction_to_band(mat, band)
    tri = band_to_tridiagonal(UpLo.Lower, band, mat)
    if eigenvalues_value_range is not None:
        ib, ie = _value_range_indices(tri, eigenvalues_value_range,
                                      mat.device)
    if tridiag_solver == "bisect":
        # only the selected eigenpairs: E_real is [n, ie - ib], never n x n
        dlaf_assert(0 <= ib <= n and ie <= n, "eigenvalue index range out "
                    "of bounds", ib, ie, n)
        w, E_real = tridiagonal_eigensolver_bisect(
            tri.d, tri.e, ib, max(ie, ib), device=mat.device)
        w = w.to(_real_dtype(mat.dtype))
        E = E_real.to(mat.dtype)
        del E_real
    else:
        w, E_real = tridiagonal_eigensolver(tri.d, tri.e, device=mat.device)
        w = w[ib:ie].clone()
        E = E_real[:, ib:ie].to(mat.dtype).contiguous()
    bt_band_to_tridiagonal(E, tri)
    bt_reduction_to_band(E, mat, refl)

    nE = E.shape[1]
    evecs = Matrix.create(n, max(nE, 1), d.mb, d.nb, dtype=mat.dtype,
                          device=mat.device, grid=mat.grid)
    if nE:
        _set_cols(evecs, E)
    return w, evecs


def _value_range_indices(tri, vrange, device) -> Tuple[int, int]:
    """[vl, vu) -> index range, by Sturm counts on the tridiagonal (replicated
    on a distributed grid, so every rank resolves the same range)."""
    dh, e2h, _, _, pivmin = _setup(tri.d, tri.e)
    return _resolve_value_range((dh, e2h, pivmin), vrange, device)


def _eigh_direct(mat: Matrix, g, ib: int, ie,
                 vrange=None) -> Tuple[torch.Tensor, Matrix]:
    """Dense fallback for problems at or below one band/tile: assemble the
    Hermitian matrix, torch.linalg.eigh (rank-replicated when distributed),
    slice the requested spectrum."""
    d = mat.dist
    n = d.m
    ie = n if ie is None else ie
    a = mat.to_global()
    a = torch.tril(a) + torch.tril(a, -1).mH
    w_all, E_all = torch.linalg.eigh(a)
    if vrange is not None:
        ib, ie = _resolve_value_range(w_all, vrange, mat.device)
    w = w_all[ib:ie].clone()
    E = E_all[:, ib:ie].contiguous()
    nE = E.shape[1]
    evecs = Matrix.create(n, max(nE, 1), d.mb, d.nb, dtype=mat.dtype,
                          device=mat.device, grid=mat.grid)
    if nE:
        _set_cols(evecs, E)
    return w, evecs


def _set_cols(evecs: Matrix, E: torch.Tensor) -> None:
    de = evecs.dist
    if (de.m, de.n) == tuple(E.shape):
        evecs.set_from_global(E)
        return
    # partial spectrum: E has fewer columns than the (n x nE) matrix shape
    full = torch.zeros((de.m, de.n), dtype=E.dtype, device=E.device)
    full[:, : E.shape[1]] = E
    evecs.set_from_global(full)


def hermitian_generalized_eigensolver(
    uplo: UpLo,
    mat_a: Matrix,
    mat_b: Matrix,
    grid: Optional[CommGrid] = None,
    factorized: bool = False,
    band: Optional[int] = None,
    eigenvalues_index_begin: int = 0,
    eigenvalues_index_end: Optional[int] = None,
    tridiag_solver: str = "dc",
    eigenvalues_value_range: Optional[Tuple[float, float]] = None,
    warn_b_rcond: bool = False,
) -> Tuple[torch.Tensor, Matrix]:
    """Generalized problem A x = lambda B x (B HPD): returns (w, E).

    ``mat_b`` is overwritten with its Cholesky factor (or is already the
    factor when ``factorized``); ``mat_a`` is overwritten. Reference:
    ``eigensolver/gen_eigensolver/impl.h:30-104``. ``tridiag_solver`` and
    ``eigenvalues_value_range`` as in ``hermitian_eigensolver``.

    A and B (or the given factor) are scaled independently when their norms
    are outside the safe range; eigenvalues, eigenvectors and the factor left
    in ``mat_b`` are those of the caller's A and B.

    ``warn_b_rcond``: estimate the reciprocal condition number of B from its
    factor (``cholesky_rcond``) and emit a ``RuntimeWarning`` carrying it when
    it is below the precision of the dtype. Needs B itself, so it does
    nothing when ``factorized``.
    """
    assert uplo == UpLo.Lower
    g = grid if grid is not None else mat_a.grid
    ea, k = _scaling.scale_generalized(mat_a, mat_b, g, factorized)
    # mat_b holds 4^k B until it is factorized, 2^k L from then on; whatever
    # happens, the caller gets it back in its own units
    undo = k if factorized else 2 * k
    try:
        if not factorized:
            if warn_b_rcond:
                bnorm = matrix_norm("one", mat_b, uplo=UpLo.Lower,
                                    structure="hermitian", grid=g)
            cholesky_factorization(UpLo.Lower, mat_b, g)
            undo = k
            if warn_b_rcond:
                warn_if_ill_conditioned(UpLo.Lower, mat_b, bnorm, g, "B")
        generalized_to_standard(UpLo.Lower, mat_a, mat_b, g)
        w, evecs = hermitian_eigensolver(
            UpLo.Lower, mat_a, g, band=band,
            eigenvalues_index_begin=eigenvalues_index_begin,
            eigenvalues_index_end=eigenvalues_index_end,
            tridiag_solver=tridiag_solver,
            eigenvalues_value_range=_scaling.scale_range(
                eigenvalues_value_range, ea - 2 * k),
        )
        # back-substitute: x = L^-H y
        triangular_solver(Side.Left, UpLo.Lower, Op.ConjTrans, Diag.NonUnit,
                          1.0, mat_b, evecs, g)
    finally:
        _scaling.scale_matrix(mat_b, -undo)
    _scaling.scale_matrix(evecs, k)  # x = 2^k x'
    if ea or k:
        w = _scaling.scale_values(w, 2 * k - ea)
    return w, evecs
