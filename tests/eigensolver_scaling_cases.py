"""Checks shared by the eigensolver-scaling tests (CPU and GPU).

``A = s * A0`` with ``A0`` a random Hermitian matrix of moderate norm and
``s`` a power of two far outside the safe range of the element type, so
``w / s`` must reproduce the eigenvalues of ``A0`` (float64 ``eigvalsh`` is
the reference) to the tolerances tests/test_eigensolver.py uses in range:
float64 1e-11 n values, 1e-10 n residual, 1e-11 n orthogonality; float32
1e-2. Multiplying by a power of two is exact, so A0 is recovered exactly.
"""

from functools import lru_cache
import math

import numpy as np
import scipy.linalg as sl
import torch

from dlaf_amd import (
    Matrix, UpLo, hermitian_eigensolver, hermitian_eigenvalues,
    hermitian_generalized_eigensolver, hermitian_generalized_eigenvalues,
)
from dlaf_amd.algs import _scaling

# dtype -> out-of-range powers of two
SCALES = {
    "float64": (-600, 520), "complex128": (-600, 520),
    "float32": (-70, 66), "complex64": (-70, 66),
}
# generalized pairs (log2 s_A, log2 s_B)
GEN_PAIRS = [(-600, 0), (0, 600), (0, -600), (-300, 300)]


def tolerances(dtype: str, n: int):
    """(values, residual, orthogonality), absolute, in units of A0."""
    if dtype in ("float64", "complex128"):
        return 1e-11 * n, 1e-10 * n, 1e-11 * n
    return 1e-2, 1e-2, 1e-2


@lru_cache(maxsize=None)
def base_matrix(n: int, dtype: str, seed: int = 0):
    """(A0 as float64/complex128 numpy, its eigenvalues); A0 is exactly
    representable in ``dtype``."""
    rng = np.random.default_rng(77 + seed + n)
    a = rng.standard_normal((n, n))
    if dtype.startswith("complex"):
        a = a + 1j * rng.standard_normal((n, n))
    a = ((a + a.conj().T) / 2).astype(dtype)
    a = a.astype(np.complex128 if dtype.startswith("complex")
                 else np.float64)
    a = (a + a.conj().T) / 2   # exact: the halves are equal
    w = np.linalg.eigvalsh(a)
    a.setflags(write=False)
    return a, w


@lru_cache(maxsize=None)
def base_spd(n: int, dtype: str):
    rng = np.random.default_rng(991 + n)
    b = rng.standard_normal((n, n))
    if dtype.startswith("complex"):
        b = b + 1j * rng.standard_normal((n, n))
    b = b @ b.conj().T / n + 2 * np.eye(n)
    b = (b + b.conj().T) / 2
    b.setflags(write=False)
    return b


def scaled_matrix(a0, p: int, n: int, nb: int, dtype: str, device,
                  grid=None) -> Matrix:
    mat = Matrix.create(n, n, nb, nb, dtype=getattr(torch, dtype),
                        device=device, grid=grid)
    # scale in the target dtype: a0 * 2^p may overflow float64 -> float32
    # conversion order otherwise
    t = torch.from_numpy(np.ldexp(1.0, p) * np.array(a0))
    mat.set_from_global(t.to(getattr(torch, dtype)))
    return mat


def unscale(w: torch.Tensor, p: int) -> np.ndarray:
    return np.ldexp(w.detach().cpu().numpy().astype(np.float64), -p)


def check_eigensolver(n, nb, dtype, p, device, tridiag_solver="dc",
                      index_end=None, grid=None):
    a0, w0 = base_matrix(n, dtype)
    tv, tr, to = tolerances(dtype, n)
    mat = scaled_matrix(a0, p, n, nb, dtype, device, grid)
    w, ev = hermitian_eigensolver(UpLo.Lower, mat, grid,
                                  tridiag_solver=tridiag_solver,
                                  eigenvalues_index_end=index_end)
    k = n if index_end is None else index_end
    ws = unscale(w, p)
    assert ws.shape == (k,)
    verr = np.abs(ws - w0[:k]).max()
    E = ev.to_global().cpu().numpy()[:, :k].astype(a0.dtype)
    res = np.abs(a0 @ E - E * ws[None, :]).max()
    orth = np.abs(E.conj().T @ E - np.eye(k)).max()
    print(f"{dtype} 2^{p} {tridiag_solver}: values {verr:.3e} (tol {tv:.1e})"
          f" residual {res:.3e} (tol {tr:.1e}) orth {orth:.3e} (tol {to:.1e})")
    assert verr < tv and res < tr and orth < to, (verr, res, orth)


def check_eigenvalues(n, nb, dtype, p, device, grid=None):
    a0, w0 = base_matrix(n, dtype)
    tv = tolerances(dtype, n)[0]
    mat = scaled_matrix(a0, p, n, nb, dtype, device, grid)
    w = hermitian_eigenvalues(UpLo.Lower, mat, grid)
    verr = np.abs(unscale(w, p) - w0).max()
    print(f"{dtype} 2^{p} eigenvalues: {verr:.3e} (tol {tv:.1e})")
    assert verr < tv, verr
    return unscale(w, p)


def check_value_range(n, nb, dtype, p, device, with_vectors: bool):
    """A range given in the units of s*A0 selects the indices that the
    unscaled range selects on A0."""
    a0, w0 = base_matrix(n, dtype)
    # bounds in gaps of the spectrum, away from any eigenvalue
    ib, ie = n // 4, n // 2
    vl = (w0[ib - 1] + w0[ib]) / 2
    vu = (w0[ie - 1] + w0[ie]) / 2
    vr = (math.ldexp(vl, p), math.ldexp(vu, p))
    mat = scaled_matrix(a0, p, n, nb, dtype, device)
    if with_vectors:
        w, _ = hermitian_eigensolver(UpLo.Lower, mat,
                                     eigenvalues_value_range=vr)
    else:
        w = hermitian_eigenvalues(UpLo.Lower, mat,
                                  eigenvalues_value_range=vr)
    assert w.shape[0] == ie - ib, (w.shape, ib, ie)
    tv = tolerances(dtype, n)[0]
    assert np.abs(unscale(w, p) - w0[ib:ie]).max() < tv


def check_generalized(n, nb, dtype, pa, pb, device, factorized=False,
                      values_only=False):
    a0, _ = base_matrix(n, dtype)
    b0 = base_spd(n, dtype)
    wref = sl.eigh(a0, b0, eigvals_only=True)
    A = scaled_matrix(a0, pa, n, nb, dtype, device)
    if factorized:
        # the caller's factor, scaled: L * 2^pb is the factor of B0 * 4^pb
        l0 = np.linalg.cholesky(b0)
        B = scaled_matrix(l0, pb, n, nb, dtype, device)
        pw = pa - 2 * pb
    else:
        B = scaled_matrix(b0, pb, n, nb, dtype, device)
        pw = pa - pb
    if values_only:
        w = hermitian_generalized_eigenvalues(UpLo.Lower, A, B,
                                              factorized=factorized)
    else:
        w, X = hermitian_generalized_eigensolver(UpLo.Lower, A, B,
                                                 factorized=factorized)
    ws = unscale(w, pw)
    verr = np.abs(ws - wref).max()
    print(f"gen ({pa}, {pb}) factorized={factorized}: values {verr:.3e}")
    assert verr < 1e-9 * n, verr
    # B leaves holding the factor of the caller's B, to the tolerance of
    # tests/test_cholesky.py (1e-11 n relative to the factor); the exact
    # power of two is removed before comparing
    pl = pb if factorized else pb // 2
    Lg = np.tril(B.to_global().cpu().numpy()) * np.ldexp(1.0, -pl)
    l0 = np.linalg.cholesky(b0)
    if factorized:
        assert np.array_equal(Lg, l0), "given factor not restored"
    else:
        assert pb % 2 == 0
        lerr = np.abs(Lg - l0).max()
        assert lerr <= 1e-11 * max(1.0, np.abs(l0).max()) * n, lerr
    if not values_only:
        # X^H B X = I against the caller's B = 2^pb' B0: X = 2^(-pb'/2) X0
        pbb = 2 * pb if factorized else pb
        X0 = X.to_global().cpu().numpy() * np.ldexp(1.0, pbb // 2)
        borth = np.abs(X0.conj().T @ b0 @ X0 - np.eye(n)).max()
        res = np.abs(a0 @ X0 - b0 @ X0 * ws[None, :]).max()
        print(f"  B-orth {borth:.3e} residual {res:.3e}")
        assert borth < 1e-9 * n and res < 1e-9 * n, (borth, res)


class Recorder:
    """Captures the (what, norm, exponent) triples the drivers record."""

    def __init__(self, monkeypatch):
        self.calls = []
        monkeypatch.setattr(_scaling, "_record",
                            lambda what, anrm, e: self.calls.append(
                                (what, anrm, e)))


def check_in_range_untouched(n, nb, dtype, p, device, monkeypatch):
    """Inside the safe range the norm is taken, sigma is 1 and the storage
    is what the caller passed when the pipeline starts."""
    a0, _ = base_matrix(n, dtype)
    rec = Recorder(monkeypatch)
    seen = {}
    import dlaf_amd.algs.eigensolver as es
    inner = es._hermitian_eigensolver

    def spy(uplo, mat, *args):
        seen["storage"] = mat.storage.clone()
        return inner(uplo, mat, *args)

    monkeypatch.setattr(es, "_hermitian_eigensolver", spy)
    mat = scaled_matrix(a0, p, n, nb, dtype, device)
    before = mat.storage.clone()
    hermitian_eigensolver(UpLo.Lower, mat)
    assert len(rec.calls) == 1 and rec.calls[0][2] == 0, rec.calls
    assert rec.calls[0][1] == math.ldexp(float(np.abs(np.tril(a0)).max()), p)
    assert torch.equal(seen["storage"], before)
