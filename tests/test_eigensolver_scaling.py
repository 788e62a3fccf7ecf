"""The eigenvalue drivers far outside the safe range of the element type
(CPU): values, residual and orthogonality must be those of the same matrix
at scale 1. Checks and tolerances live in eigensolver_scaling_cases.py."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eigensolver_scaling_cases as sc  # noqa: E402
from dist_utils import run_distributed  # noqa: E402

N, NB = 96, 16
DEV = "cpu"
SCALED = [(dt, p) for dt, ps in sc.SCALES.items() for p in ps]


@pytest.mark.parametrize("dtype,p", SCALED)
def test_eigensolver_dc(dtype, p):
    sc.check_eigensolver(N, NB, dtype, p, DEV)


@pytest.mark.parametrize("dtype,p", SCALED)
def test_eigensolver_bisect_partial(dtype, p):
    sc.check_eigensolver(N, NB, dtype, p, DEV, tridiag_solver="bisect",
                         index_end=10)


@pytest.mark.parametrize("dtype,p", SCALED)
def test_eigenvalues(dtype, p):
    sc.check_eigenvalues(N, NB, dtype, p, DEV)


@pytest.mark.parametrize("with_vectors", [False, True])
@pytest.mark.parametrize("p", sc.SCALES["float64"])
def test_value_range_in_scaled_units(p, with_vectors):
    sc.check_value_range(N, NB, "float64", p, DEV, with_vectors)


@pytest.mark.parametrize("pa,pb", sc.GEN_PAIRS)
def test_generalized(pa, pb):
    sc.check_generalized(N, NB, "float64", pa, pb, DEV)


def test_generalized_complex():
    sc.check_generalized(N, NB, "complex128", -600, 0, DEV)


@pytest.mark.parametrize("pa,pb", [(0, 600), (-300, 300)])
def test_generalized_eigenvalues_only(pa, pb):
    sc.check_generalized(N, NB, "float64", pa, pb, DEV, values_only=True)


@pytest.mark.parametrize("values_only", [False, True])
def test_generalized_factorized(values_only):
    sc.check_generalized(N, NB, "float64", 0, 300, DEV, factorized=True,
                         values_only=values_only)


@pytest.mark.parametrize("factorized", [True, False])
def test_b_is_unscaled_when_the_solve_raises(factorized, monkeypatch):
    """An exception after B (or the given factor) was scaled must not leave
    it scaled: the factor comes back bitwise, B by the same power of two."""
    import dlaf_amd.algs.eigensolver as es
    from dlaf_amd import UpLo, hermitian_generalized_eigensolver
    a0, _ = sc.base_matrix(N, "float64")
    src = np.linalg.cholesky(sc.base_spd(N, "float64")) if factorized \
        else sc.base_spd(N, "float64")
    A = sc.scaled_matrix(a0, 0, N, NB, "float64", DEV)
    B = sc.scaled_matrix(src, 300 if factorized else 600, N, NB, "float64",
                         DEV)
    before = B.storage.clone()

    def boom(*args, **kwargs):
        raise RuntimeError("boom")

    # fails before anything but the scaling has written to B
    monkeypatch.setattr(es, "generalized_to_standard" if factorized
                        else "cholesky_factorization", boom)
    with pytest.raises(RuntimeError, match="boom"):
        hermitian_generalized_eigensolver(UpLo.Lower, A, B,
                                          factorized=factorized)
    assert torch.equal(B.storage, before)


@pytest.mark.parametrize("p", [0, 100])
def test_in_range_input_is_not_touched(p, monkeypatch):
    sc.check_in_range_untouched(N, NB, "float64", p, DEV, monkeypatch)


def test_scale_exponent():
    from dlaf_amd.algs._scaling import scale_exponent
    f64, f32 = torch.float64, torch.float32
    assert scale_exponent(1.0, f64) == 0
    assert scale_exponent(2.0 ** 485, f64) == 0
    assert scale_exponent(2.0 ** -485, f64) == 0
    assert scale_exponent(1.5 * 2.0 ** 485, f64) == -485
    assert scale_exponent(1.5 * 2.0 ** -600, torch.complex128) == 600
    assert scale_exponent(2.0 ** 52, f32) == -52
    assert scale_exponent(2.0 ** -70, torch.complex64) == 70
    assert scale_exponent(0.0, f64) == 0
    assert scale_exponent(float("inf"), f64) == 0
    assert scale_exponent(float("nan"), f64) == 0
    # B: an even exponent, so its square root is a power of two
    assert scale_exponent(2.0 ** 601, f64, even=True) % 2 == 0
    # a given factor: the square root of the range
    assert scale_exponent(2.0 ** 242, f64, root=True) == 0
    assert scale_exponent(2.0 ** 300, f64, root=True) == -300


# ---------------- distributed (gloo) ----------------

def _dist_worker(rank, ws, values_only):
    from dlaf_amd import CommGrid
    grid = CommGrid(2, 2)
    if values_only:
        sc.check_eigenvalues(N, NB, "float64", -600, DEV, grid)
    else:
        sc.check_eigensolver(N, NB, "float64", -600, DEV, grid=grid)
    return True


@pytest.mark.parametrize("values_only", [False, True])
def test_distributed_2x2(values_only):
    assert all(run_distributed(_dist_worker, 4, args=(values_only,)))
