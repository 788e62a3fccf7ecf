"""Eigenvalues-only solvers on Sturm-sequence bisection.

``tridiagonal_eigenvalues`` / ``tridiagonal_eigenvalue_count`` work on a real
symmetric tridiagonal (d, e); ``hermitian_eigenvalues`` and
``hermitian_generalized_eigenvalues`` are the values-only drivers (ScaLAPACK
``jobz='N'``): reduction to band -> bulge chase -> bisection, with no
tridiagonal eigenvectors and no back-transforms.

The recurrence, the pivmin safeguard and the bisection rule live in
``csrc/sturm.h`` (shared by the host loop and the HIP kernel of
``csrc/bisect.hip``, one thread per eigenvalue). Every eigenvalue is computed
independently from the same (d, e2, gl, gu, pivmin), so any index range equals
the corresponding slice of the full result bitwise.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..types import UpLo
from ..matrix.matrix import Matrix
from ..comm.grid import CommGrid
from ..core.asserts import dlaf_assert
from ..ops._ext import get_ext

__all__ = [
    "tridiagonal_eigenvalues",
    "tridiagonal_eigenvalue_count",
    "hermitian_eigenvalues",
    "hermitian_generalized_eigenvalues",
]


def _setup(d: torch.Tensor, e: torch.Tensor):
    """Host float64 (d, e2, gl, gu, pivmin) of ``csrc/sturm.h``."""
    dh = d.detach().to("cpu", torch.float64).contiguous()
    eh = e.detach().to("cpu", torch.float64).contiguous()
    n = dh.shape[0]
    dlaf_assert(dh.dim() == 1 and eh.dim() == 1
                and eh.shape[0] == max(n - 1, 0),
                "tridiagonal: d [n] and e [n-1] required", tuple(d.shape),
                tuple(e.shape))
    gl, gu, pivmin = get_ext().sturm_interval(dh, eh)
    return dh, eh * eh, gl, gu, pivmin


def _resolve_device(d: torch.Tensor, device) -> torch.device:
    if device is None:
        return d.device
    return device if isinstance(device, torch.device) else torch.device(device)


def _bisect_range(dh, e2h, gl, gu, pivmin, ib: int, ie: int, device,
                  grid: Optional[CommGrid]) -> torch.Tensor:
    ext = get_ext()
    dd, ee = dh.to(device), e2h.to(device)
    m = ie - ib
    if grid is None or not grid.distributed:
        w = torch.empty(m, dtype=torch.float64, device=device)
        ext.tridiag_bisect(dd, ee, ib, ie, gl, gu, pivmin, w)
        return w
    # contiguous chunk per rank, one all-gather of equal padded chunks: every
    # rank assembles the same bits
    import torch.distributed as dist
    world = grid.world_size
    chunk = -(-m // world)
    a = min(ib + grid.rank * chunk, ie)
    b = min(a + chunk, ie)
    buf = torch.zeros(chunk, dtype=torch.float64, device=device)
    ext.tridiag_bisect(dd, ee, a, b, gl, gu, pivmin, buf)
    gath = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(gath, buf, group=grid.full_group)
    return torch.cat(gath)[:m].contiguous()


def tridiagonal_eigenvalues(d: torch.Tensor, e: torch.Tensor,
                            index_begin: int = 0,
                            index_end: Optional[int] = None,
                            device=None,
                            grid: Optional[CommGrid] = None) -> torch.Tensor:
    """Eigenvalues ``index_begin <= k < index_end`` (0-based, ascending) of
    the real symmetric tridiagonal matrix with diagonal ``d`` [n] and
    off-diagonal ``e`` [n-1], by Sturm-sequence bisection.

    Returns float64 on ``device`` (default: where ``d`` lives). CUDA devices
    run the HIP kernel, CPU the host twin. With a distributed ``grid`` the
    index range is cut into one contiguous chunk per rank and assembled with
    one all-gather; every rank returns identical bits.
    """
    device = _resolve_device(d, device)
    n = d.shape[0]
    ib = index_begin
    ie = n if index_end is None else index_end
    dlaf_assert(0 <= ib <= n and ie <= n, "eigenvalue index range out of "
                "bounds", ib, ie, n)
    if n == 0 or ie <= ib:
        return torch.zeros(0, dtype=torch.float64, device=device)
    if n == 1:
        return d.detach().to(device, torch.float64).clone()
    dh, e2h, gl, gu, pivmin = _setup(d, e)
    return _bisect_range(dh, e2h, gl, gu, pivmin, ib, ie, device, grid)


def _count(dh, e2h, pivmin, x: torch.Tensor, device) -> torch.Tensor:
    xs = x.detach().to(device, torch.float64).reshape(-1).contiguous()
    cnt = torch.zeros(xs.shape[0], dtype=torch.int64, device=device)
    get_ext().sturm_count(dh.to(device), e2h.to(device), pivmin, xs, cnt)
    return cnt


def tridiagonal_eigenvalue_count(d: torch.Tensor, e: torch.Tensor,
                                 x) -> torch.Tensor:
    """Number of eigenvalues of tridiag(d, e) strictly below each ``x``
    (int64 tensor of ``x``'s shape, on ``d``'s device)."""
    xt = torch.as_tensor(x, dtype=torch.float64)
    dh, e2h, _, _, pivmin = _setup(d, e)
    return _count(dh, e2h, pivmin, xt, d.device).reshape(xt.shape)


def _resolve_value_range(w_or_tri, vrange, device) -> Tuple[int, int]:
    """[vl, vu) -> index range [count(vl), count(vu))."""
    vl, vu = float(vrange[0]), float(vrange[1])
    dlaf_assert(vl <= vu, "eigenvalues_value_range: vl <= vu required", vl, vu)
    x = torch.tensor([vl, vu], dtype=torch.float64)
    if isinstance(w_or_tri, torch.Tensor):   # tiny path: sorted eigenvalues
        w = w_or_tri.detach().to("cpu", torch.float64)
        c = torch.searchsorted(w, x, right=False)
    else:
        dh, e2h, pivmin = w_or_tri
        c = _count(dh, e2h, pivmin, x, device).cpu()
    return int(c[0]), int(c[1])


def _real_dtype(dt: torch.dtype) -> torch.dtype:
    return torch.empty(0, dtype=dt).real.dtype if dt.is_complex else dt


def hermitian_eigenvalues(
    uplo: UpLo,
    mat: Matrix,
    grid: Optional[CommGrid] = None,
    band: Optional[int] = None,
    eigenvalues_index_begin: int = 0,
    eigenvalues_index_end: Optional[int] = None,
    eigenvalues_value_range: Optional[Tuple[float, float]] = None,
) -> torch.Tensor:
    """Eigenvalues only of a Hermitian tiled matrix (ScaLAPACK ``jobz='N'``).

    Runs reduction to band and the bulge chase exactly like
    ``hermitian_eigensolver`` (same asserts, band choice and overwrite of
    ``mat``), then Sturm bisection on the tridiagonal; the reflectors are
    discarded, no eigenvector is formed and nothing is back-transformed.

    The spectrum slice is either the 0-based index range
    [``eigenvalues_index_begin``, ``eigenvalues_index_end``) or
    ``eigenvalues_value_range=(vl, vu)``, the eigenvalues in the HALF-OPEN
    interval ``[vl, vu)`` — note this differs from LAPACK's ``(vl, vu]``. The
    two are mutually exclusive. Returns ``w`` ascending in the real dtype of
    ``mat``; identical on every rank of a distributed grid.

    Safe at any scale, by the same power-of-two scaling as
    ``hermitian_eigensolver``.
    """
    from . import _scaling
    e = 0
    d = mat.dist
    if uplo == UpLo.Lower and d.m == d.n and d.mb == d.nb:
        e = _scaling.scale_hermitian(
            mat, grid if grid is not None else mat.grid)
    w = _hermitian_eigenvalues(
        uplo, mat, grid, band, eigenvalues_index_begin, eigenvalues_index_end,
        _scaling.scale_range(eigenvalues_value_range, e))
    return _scaling.scale_values(w, -e) if e else w


def _hermitian_eigenvalues(uplo, mat, grid, band, eigenvalues_index_begin,
                           eigenvalues_index_end, eigenvalues_value_range):
    """``hermitian_eigenvalues`` on a matrix already in the safe range."""
    from .eigensolver import get_band_size
    dlaf_assert(uplo == UpLo.Lower,
                "only Lower implemented (as the reference miniapps)")
    d = mat.dist
    dlaf_assert(d.m == d.n and d.mb == d.nb,
                "square matrix with square tiles required", d.size,
                d.tile_size)
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
        # same divisor snap as hermitian_eigensolver
        band = max(bb for bb in range(1, band + 1) if d.nb % bb == 0)
    ib = eigenvalues_index_begin
    ie = n if eigenvalues_index_end is None else eigenvalues_index_end
    rdt = _real_dtype(mat.dtype)
    dev = mat.device

    if n <= max(band, d.nb):
        # tiny problem (at or below one tile/band): direct dense eigenvalues
        a = mat.to_global()
        a = torch.tril(a) + torch.tril(a, -1).mH
        w_all = torch.linalg.eigvalsh(a)
        if eigenvalues_value_range is not None:
            ib, ie = _resolve_value_range(w_all, eigenvalues_value_range, dev)
        return w_all[ib:ie].to(rdt).clone()

    if distributed:
        from .eigensolver_tiled import red2band_tiled, extract_band_tiled
        from .band2tridiag import chase_band
        red2band_tiled(mat, band, g)
        tri = chase_band(extract_band_tiled(mat, band, g), band)
    else:
        from .red2band import reduction_to_band
        from .band2tridiag import band_to_tridiagonal
        reduction_to_band(mat, band)
        tri = band_to_tridiagonal(UpLo.Lower, band, mat)
        g = None
    td, te = tri.d, tri.e
    del tri  # chase reflectors are not needed for eigenvalues

    dh, e2h, gl, gu, pivmin = _setup(td, te)
    if eigenvalues_value_range is not None:
        ib, ie = _resolve_value_range((dh, e2h, pivmin),
                                      eigenvalues_value_range, dev)
    dlaf_assert(0 <= ib <= n and ie <= n, "eigenvalue index range out of "
                "bounds", ib, ie, n)
    if ie <= ib:
        return torch.zeros(0, dtype=rdt, device=dev)
    w = _bisect_range(dh, e2h, gl, gu, pivmin, ib, ie, dev, g)
    return w.to(rdt)


def hermitian_generalized_eigenvalues(
    uplo: UpLo,
    mat_a: Matrix,
    mat_b: Matrix,
    grid: Optional[CommGrid] = None,
    factorized: bool = False,
    band: Optional[int] = None,
    eigenvalues_index_begin: int = 0,
    eigenvalues_index_end: Optional[int] = None,
    eigenvalues_value_range: Optional[Tuple[float, float]] = None,
    warn_b_rcond: bool = False,
) -> torch.Tensor:
    """Eigenvalues only of A x = lambda B x (B HPD).

    ``mat_b`` is overwritten with its Cholesky factor (or already is the
    factor when ``factorized``); ``mat_a`` is overwritten. Cholesky ->
    generalized_to_standard -> ``hermitian_eigenvalues``; there is no
    back-substitution. Range arguments as in ``hermitian_eigenvalues``
    (value range half-open ``[vl, vu)``). ``warn_b_rcond`` as in
    ``hermitian_generalized_eigensolver``.
    """
    from .cholesky import cholesky_factorization
    from .gen_to_std import generalized_to_standard
    from .norm import matrix_norm
    from .condition import warn_if_ill_conditioned
    from . import _scaling
    dlaf_assert(uplo == UpLo.Lower, "only Lower implemented")
    g = grid if grid is not None else mat_a.grid
    # A, B (or the factor) scaled as in hermitian_generalized_eigensolver
    ea, k = _scaling.scale_generalized(mat_a, mat_b, g, factorized)
    undo = k if factorized else 2 * k  # 4^k B until factorized, then 2^k L
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
        w = hermitian_eigenvalues(
            UpLo.Lower, mat_a, g, band=band,
            eigenvalues_index_begin=eigenvalues_index_begin,
            eigenvalues_index_end=eigenvalues_index_end,
            eigenvalues_value_range=_scaling.scale_range(
                eigenvalues_value_range, ea - 2 * k))
    finally:
        _scaling.scale_matrix(mat_b, -undo)
    return _scaling.scale_values(w, 2 * k - ea) if (ea or k) else w
