"""Shifted-solve HIP kernel (csrc/invit.hip), inverse iteration and the
``tridiag_solver="bisect"`` drivers on device.

Same bounds as the host tests; sizes sit around the 64-thread workgroup
(63/64/65), use several workgroups (257) and cross the LDS staging chunk
(kBisectChunk + 1 = 1025).
"""

import pytest
import torch

import tridiag_cases as tc
import invit_checks as ic
import eigensolver_bisect_cases as ec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("n", ic.SIZES)
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_full_range(family, n):
    ic.check_eigenvectors(family, n, device=DEV)


@pytest.mark.parametrize("ib,ie", ic.RANGES_257)
def test_index_ranges(ib, ie):
    ic.check_eigenvectors("random", 257, ib, ie, device=DEV)


@pytest.mark.parametrize("family", ic.CHUNK_CASES)
def test_across_lds_chunk(family):
    ic.check_eigenvectors(family, 1025, 400, 520, device=DEV)


@pytest.mark.parametrize("family", ["random", "graded"])
def test_several_column_chunks(family):
    """_work_cols=64 at n = 257: five launches, the last one partial."""
    Z = ic.check_eigenvectors(family, 257, device=DEV, _work_cols=64)
    assert torch.equal(Z, ic.check_eigenvectors(family, 257, device=DEV))


def test_deterministic():
    Z1 = ic.check_eigenvectors("glued_wilkinson", 257, 17, 93, device=DEV)
    Z2 = ic.check_eigenvectors("glued_wilkinson", 257, 17, 93, device=DEV)
    assert torch.equal(Z1, Z2)


@pytest.mark.parametrize("at_eigenvalues", [False, True],
                         ids=["midpoints", "eigenvalues"])
@pytest.mark.parametrize("n", ic.SOLVE_SIZES)
@pytest.mark.parametrize("family", ic.SOLVE_FAMILIES)
def test_shifted_solve_backward_error(family, n, at_eigenvalues):
    Y = ic.check_solve(family, n, at_eigenvalues, device=DEV)
    ds, es, lam, t1, X = ic.solve_case(family, n, at_eigenvalues)
    Yh = ic.run_solve(ds, es, lam, t1, X, "cpu").numpy()
    print(f"  gpu and host twin bitwise equal: {bool((Y == Yh).all())}")


def test_shifted_solve_column_slice():
    """A column slice of a wider matrix, narrower than the workspace: the
    other columns stay untouched."""
    from dlaf_amd.ops._ext import get_ext
    ds, es, lam, t1, X = ic.solve_case("random", 65, True)
    full = ic.run_solve(ds, es, lam, t1, X, DEV)
    Y = X.clone().to(DEV)
    work = torch.empty((3, 65, 64), dtype=torch.float64, device=DEV)
    get_ext().tridiag_shifted_solve(
        ic._t(ds, DEV), ic._t(es, DEV), ic._t(lam[10:40].copy(), DEV),
        tc.EPS * t1, Y[:, 10:40], work)
    Y = Y.cpu()
    assert torch.equal(Y[:, 10:40], full[:, 10:40])
    assert torch.equal(Y[:, :10], X[:, :10])
    assert torch.equal(Y[:, 40:], X[:, 40:])


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128])
def test_bisect_index_range(dtype):
    ec.check_standard(dtype, DEV)


def test_value_range_equals_index_range():
    ec.check_value_range(torch.float64, DEV, exact_vectors=False)


def test_generalized_bisect():
    ec.check_generalized(torch.float64, DEV)
