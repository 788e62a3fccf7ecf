"""Sturm-bisection HIP kernels (csrc/bisect.hip) and the values-only driver
on device.

Same long-double reference and 4*eps*G bound as the host tests; sizes sit
around the 64-thread workgroup (63/64/65), use several workgroups (257) and
cross the LDS staging chunk (kBisectChunk + 1 = 1025).
"""

import numpy as np
import pytest
import torch

from dlaf_amd import (
    Matrix, UpLo, hermitian_eigenvalues, tridiagonal_eigenvalues,
    tridiagonal_eigenvalue_count,
)
from dlaf_amd.matrix import util as mutil
import tridiag_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK = 1024  # kBisectChunk of csrc/kernels.h
SIZES = [1, 2, 3, 63, 64, 65, 257]


def _t(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_kernel_accuracy_and_order(family, n):
    d, e = tc.make_case(family, n)
    w = tridiagonal_eigenvalues(_t(d, DEV), _t(e, DEV))
    assert w.is_cuda and w.dtype == torch.float64 and w.shape == (n,)
    wn = w.cpu().numpy()
    assert np.all(np.diff(wn) >= 0), "eigenvalues not ascending"
    err = tc.max_err_units(wn, family, n)
    print(f"{family} n={n}: max err = {err:.3f} eps*G")
    assert err <= tc.TOL_FACTOR


@pytest.mark.parametrize("family", ["random", "glued_wilkinson"])
def test_kernel_across_lds_chunk(family):
    n = CHUNK + 1
    d, e = tc.make_case(family, n)
    w = tridiagonal_eigenvalues(_t(d, DEV), _t(e, DEV)).cpu().numpy()
    assert np.all(np.diff(w) >= 0)
    err = tc.max_err_units(w, family, n)
    print(f"{family} n={n}: max err = {err:.3f} eps*G")
    assert err <= tc.TOL_FACTOR
    # host twin on the same input, well inside 2*eps*G
    wh = tridiagonal_eigenvalues(_t(d), _t(e)).numpy()
    G = tc.gershgorin(d, e)[2]
    assert np.abs(w - wh).max() <= 2 * tc.EPS * G


@pytest.mark.parametrize("ib,ie", [(0, 257), (0, 1), (256, 257), (5, 5),
                                   (17, 93)])
def test_index_ranges_bitwise(ib, ie):
    n = 257
    d, e = tc.make_case("random", n)
    full = tridiagonal_eigenvalues(_t(d, DEV), _t(e, DEV))
    part = tridiagonal_eigenvalues(_t(d, DEV), _t(e, DEV), ib, ie)
    assert part.is_cuda and part.shape == (ie - ib,)
    assert torch.equal(part, full[ib:ie])


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_gpu_matches_host_twin(family):
    n = 257
    d, e = tc.make_case(family, n)
    wg = tridiagonal_eigenvalues(_t(d, DEV), _t(e, DEV)).cpu().numpy()
    wh = tridiagonal_eigenvalues(_t(d), _t(e)).numpy()
    G = tc.gershgorin(d, e)[2]
    diff = np.abs(wg - wh).max()
    print(f"{family}: |gpu - host| max = {diff / (tc.EPS * G):.3f} eps*G, "
          f"bitwise equal: {np.array_equal(wg, wh)}")
    assert diff <= 2 * tc.EPS * G


def test_sturm_count_gpu():
    n = 257
    d, e = tc.make_case("random", n)
    ref = np.asarray(tc.reference("random", n), dtype=np.float64)
    x = 0.5 * (ref[:-1] + ref[1:])
    cnt = tridiagonal_eigenvalue_count(_t(d, DEV), _t(e, DEV), _t(x))
    assert cnt.is_cuda and cnt.dtype == torch.int64
    assert torch.equal(cnt.cpu(), torch.arange(1, n, dtype=torch.int64))
    gl, gu, G = tc.gershgorin(d, e)
    out = tridiagonal_eigenvalue_count(
        _t(d, DEV), _t(e, DEV), torch.tensor([gl - 1e-3 * G, gu + 1e-3 * G]))
    assert out.tolist() == [0, n]


def test_sturm_count_gpu_across_lds_chunk():
    n = CHUNK + 1
    d, e = tc.make_case("random", n)
    x = torch.linspace(-3.0, 3.0, 130, dtype=torch.float64)
    cg = tridiagonal_eigenvalue_count(_t(d, DEV), _t(e, DEV), x).cpu()
    ch = tridiagonal_eigenvalue_count(_t(d), _t(e), x)
    assert torch.equal(cg, ch)


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128])
def test_hermitian_eigenvalues_device(dtype):
    n, nb = 320, 64
    mat = Matrix.create(n, n, nb, nb, dtype=dtype, device=DEV)
    mutil.set_random_hermitian(mat, seed=51)
    a0 = mat.to_global()
    a0 = (torch.tril(a0) + torch.tril(a0, -1).mH).cpu().numpy()
    wref = np.linalg.eigvalsh(a0)
    w = hermitian_eigenvalues(UpLo.Lower, mat)
    assert w.is_cuda and w.dtype == torch.float64 and w.shape == (n,)
    scale = max(1.0, float(np.abs(wref).max()))
    assert np.abs(w.cpu().numpy() - wref).max() < 1e-11 * n * scale
    if dtype == torch.float64:
        vl = 0.5 * (wref[99] + wref[100])
        vu = 0.5 * (wref[199] + wref[200])
        mat2 = Matrix.create(n, n, nb, nb, dtype=dtype, device=DEV)
        mutil.set_random_hermitian(mat2, seed=51)
        wv = hermitian_eigenvalues(UpLo.Lower, mat2,
                                   eigenvalues_value_range=(vl, vu))
        assert torch.equal(wv, w[100:200])
