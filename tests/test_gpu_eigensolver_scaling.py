"""The eigenvalue drivers far outside the safe range of the element type, on
the device: n=150, nb=32 has a padded edge tile and is above the direct-eigh
cut-off, so the norm kernel, the scaling of the padded storage and the whole
HIP pipeline run. Checks live in eigensolver_scaling_cases.py."""

import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eigensolver_scaling_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

N, NB = 150, 32
DEV = "cuda:0"
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


def test_generalized_eigenvalues_only():
    sc.check_generalized(N, NB, "float64", -300, 300, DEV, values_only=True)


def test_generalized_factorized():
    sc.check_generalized(N, NB, "float64", 0, 300, DEV, factorized=True)


@pytest.mark.parametrize("p", [0, 100])
def test_in_range_input_is_not_touched(p, monkeypatch):
    sc.check_in_range_untouched(N, NB, "float64", p, DEV, monkeypatch)
