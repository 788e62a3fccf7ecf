"""Sturm-bisection tridiagonal eigenvalues, host path (csrc/sturm.h via the
host twins in csrc/ext.cpp).

Accuracy is checked against the independent long-double bisection of
``tridiag_cases`` at 4*eps*G (64*eps*G against dense LAPACK where no 80-bit
long double exists), G the Gershgorin bound.
"""

import numpy as np
import pytest
import torch

from dlaf_amd import (
    tridiagonal_eigenvalues, tridiagonal_eigenvalue_count,
    tridiagonal_eigensolver,
)
import tridiag_cases as tc

SIZES = [1, 2, 3, 64, 65, 257]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_accuracy_and_order(family, n):
    d, e = tc.make_case(family, n)
    w = tridiagonal_eigenvalues(_t(d), _t(e))
    assert w.dtype == torch.float64 and w.shape == (n,)
    wn = w.numpy()
    assert np.all(np.diff(wn) >= 0), "eigenvalues not ascending"
    err = tc.max_err_units(wn, family, n)
    print(f"{family} n={n}: max err = {err:.3f} eps*G")
    assert err <= tc.TOL_FACTOR


@pytest.mark.parametrize("family", ["random", "glued_wilkinson"])
@pytest.mark.parametrize("ib,ie", [(0, 257), (0, 1), (256, 257), (5, 5),
                                   (17, 93)])
def test_index_ranges_bitwise(family, ib, ie):
    n = 257
    d, e = tc.make_case(family, n)
    full = tridiagonal_eigenvalues(_t(d), _t(e))
    part = tridiagonal_eigenvalues(_t(d), _t(e), ib, ie)
    assert part.shape == (ie - ib,)
    assert torch.equal(part, full[ib:ie])


def test_empty_and_single():
    z = torch.zeros(0, dtype=torch.float64)
    assert tridiagonal_eigenvalues(z, z).shape == (0,)
    d1 = torch.tensor([2.5], dtype=torch.float64)
    assert torch.equal(tridiagonal_eigenvalues(d1, z), d1)
    assert tridiagonal_eigenvalues(d1, z, 1, 1).shape == (0,)


def test_float32_input_is_widened():
    d, e = tc.make_case("random", 65)
    d32, e32 = _t(d).float(), _t(e).float()
    w = tridiagonal_eigenvalues(d32, e32)
    assert w.dtype == torch.float64
    assert torch.equal(w, tridiagonal_eigenvalues(d32.double(), e32.double()))


def test_count_exact_index():
    n = 257
    d, e = tc.make_case("random", n)
    ref = np.asarray(tc.reference("random", n), dtype=np.float64)
    x = 0.5 * (ref[:-1] + ref[1:])
    cnt = tridiagonal_eigenvalue_count(_t(d), _t(e), _t(x))
    assert cnt.dtype == torch.int64
    assert torch.equal(cnt, torch.arange(1, n, dtype=torch.int64))
    gl, gu, G = tc.gershgorin(d, e)
    out = tridiagonal_eigenvalue_count(
        _t(d), _t(e), torch.tensor([gl - 1e-3 * G, gu + 1e-3 * G]))
    assert out.tolist() == [0, n]


def test_count_split_and_exact_hit():
    # zero off-diagonals and x exactly on an eigenvalue are well defined
    d, e = tc.make_case("constant_diag", 64)
    cnt = tridiagonal_eigenvalue_count(_t(d), _t(e),
                                       torch.tensor([2.0, 4.0]))
    assert cnt.tolist() == [0, 64]
    x = torch.linspace(-1.0, 5.0, 101, dtype=torch.float64)
    c = tridiagonal_eigenvalue_count(_t(d), _t(e), x)
    assert bool((c[1:] >= c[:-1]).all())


def test_agrees_with_divide_and_conquer():
    n = 300
    rng = np.random.default_rng(7)
    d, e = rng.standard_normal(n), rng.standard_normal(n - 1)
    w = tridiagonal_eigenvalues(_t(d), _t(e))
    w_dc = tridiagonal_eigensolver(_t(d), _t(e))[0]
    G = tc.gershgorin(d, e)[2]
    assert float((w - w_dc).abs().max()) <= 1e-11 * n * G
