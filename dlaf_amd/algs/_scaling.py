"""Safe scaling of the eigenvalue drivers' inputs (LAPACK ``syevd`` style).

The pipeline squares and divides by entries of the matrix; outside
``[sqrt(safmin / eps), sqrt(eps / safmin)]`` that overflows or underflows
without any error. The drivers therefore measure the matrix with
``matrix_norm("max", ...)`` and, when the norm is outside that range, scale
the matrix by a power of two (exact) so that its norm lands in ``[1, 2)``,
solve, and scale the eigenvalues back. Inside the range nothing is touched.
"""

from __future__ import annotations

import math
from typing import Tuple

import torch

from ..types import UpLo, Diag, real_dtype
from ..matrix.matrix import Matrix
from .norm import matrix_norm

# log2 of [lo, hi] = [sqrt(safmin/eps), its inverse] rounded to powers of two
_LOG2_RANGE = {torch.float64: 485, torch.float32: 51}
# largest |exponent| of a single scaling step: 2^e must itself be a normal
# number of the element type (a norm down in the denormals is lifted into the
# safe range, not all the way to 1)
_MAX_STEP = {torch.float64: 1000, torch.float32: 100}


def _record(what: str, anrm: float, e: int) -> None:
    """Test hook: called once per measured matrix with the chosen exponent
    (``sigma = 2^e``; 0 means the matrix is left alone)."""


def scale_exponent(anrm: float, dtype: torch.dtype, *, root: bool = False,
                   even: bool = False) -> int:
    """e such that ``2^e * anrm`` is in [1, 2) ([1, 4) with ``even``), or 0
    when ``anrm`` is zero, not finite or inside the safe range of ``dtype``
    (the square root of that range with ``root``, for Cholesky factors)."""
    rdt = real_dtype(dtype)
    lim = _LOG2_RANGE[rdt] // 2 if root else _LOG2_RANGE[rdt]
    if not (anrm > 0.0 and math.isfinite(anrm)):
        return 0
    if 2.0 ** -lim <= anrm <= 2.0 ** lim:
        return 0
    e = 1 - math.frexp(anrm)[1]  # anrm = f * 2^-e, f in [1, 2)
    if even and e % 2:
        e += 1
    step = _MAX_STEP[rdt]
    return max(-step, min(step, e))


def scale_matrix(mat: Matrix, e: int) -> None:
    """mat <- 2^e * mat on the logical part; the identity padding is kept."""
    if e == 0:
        return
    mat.storage.mul_(2.0 ** e)
    mat._set_identity_pad()


def scale_values(w: torch.Tensor, e: int) -> torch.Tensor:
    """w * 2^e without an intermediate that overflows before the result."""
    step = 60
    while e != 0:
        s = max(-step, min(step, e))
        w = w * (2.0 ** s)
        e -= s
    return w


def scale_float(x: float, e: int) -> float:
    try:
        return math.ldexp(x, e)
    except OverflowError:
        return math.copysign(math.inf, x)


def scale_range(vrange, e: int):
    if vrange is None:
        return None
    return (scale_float(float(vrange[0]), e), scale_float(float(vrange[1]), e))


def scale_hermitian(mat: Matrix, grid, what: str = "A",
                    even: bool = False) -> int:
    """Measure the Lower-stored Hermitian ``mat`` and scale it if needed;
    returns the exponent applied."""
    anrm = matrix_norm("max", mat, uplo=UpLo.Lower, structure="hermitian",
                       grid=grid)
    e = scale_exponent(anrm, mat.dtype, even=even)
    _record(what, anrm, e)
    scale_matrix(mat, e)
    return e


def scale_factor(mat: Matrix, grid) -> int:
    """Same for a given Lower Cholesky factor, against the root range."""
    lnrm = matrix_norm("max", mat, uplo=UpLo.Lower, structure="triangular",
                       diag=Diag.NonUnit, grid=grid)
    e = scale_exponent(lnrm, mat.dtype, root=True)
    _record("L", lnrm, e)
    scale_matrix(mat, e)
    return e


def scale_generalized(mat_a: Matrix, mat_b: Matrix, grid,
                      factorized: bool) -> Tuple[int, int]:
    """Scale A by 2^ea and B by 4^k (or its given factor by 2^k). Returns
    (ea, k): the solver then sees ``2^ea A x' = lambda' 4^k B x'``, so
    ``lambda = lambda' * 2^(2k - ea)``, ``x = 2^k x'``, and the factor left
    in ``mat_b`` is ``2^k`` times the caller's."""
    ea = scale_hermitian(mat_a, grid, "A")
    if factorized:
        k = scale_factor(mat_b, grid)
    else:
        k = scale_hermitian(mat_b, grid, "B", even=True) // 2
    return ea, k
