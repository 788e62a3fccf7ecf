"""Driver cases of ``tridiag_solver="bisect"`` shared by the CPU and GPU
tests: n = 320, nb = 64, index range [100, 200); residual and orthogonality
checks and tolerances of ``tests/test_eigensolver.py``.
"""

import torch

from dlaf_amd import (
    Matrix, UpLo, hermitian_eigensolver, hermitian_eigenvalues,
    hermitian_generalized_eigensolver,
)
from dlaf_amd.matrix import util as mutil

N, NB, IB, IE = 320, 64, 100, 200


def herm(a):
    return torch.tril(a) + torch.tril(a, -1).mH


def make(dtype, device, seed=51):
    mat = Matrix.create(N, N, NB, NB, dtype=dtype, device=device)
    mutil.set_random_hermitian(mat, seed=seed)
    return mat, herm(mat.to_global())


def check_standard(dtype, device):
    mat, a0 = make(dtype, device)
    w, evecs = hermitian_eigensolver(
        UpLo.Lower, mat, eigenvalues_index_begin=IB, eigenvalues_index_end=IE,
        tridiag_solver="bisect")
    k = IE - IB
    assert w.shape == (k,) and w.dtype == torch.float64
    assert w.device.type == torch.device(device).type
    E = evecs.to_global()[:, :k]
    scale = max(1.0, w.abs().max().item())
    res = (a0 @ E - E @ torch.diag(w.to(dtype))).abs().max().item()
    orth = (E.mH @ E - torch.eye(k, dtype=dtype, device=E.device)
            ).abs().max().item()
    print(f"{dtype} {device}: res = {res:.3e} (bound {1e-10 * N * scale:.1e})"
          f", orth = {orth:.3e} (bound {1e-11 * N:.1e})")
    assert res < 1e-10 * N * scale, f"res={res}"
    assert orth < 1e-11 * N, f"orth={orth}"
    wv = hermitian_eigenvalues(UpLo.Lower, make(dtype, device)[0],
                               eigenvalues_index_begin=IB,
                               eigenvalues_index_end=IE)
    assert torch.equal(w, wv), "eigenvalues differ from hermitian_eigenvalues"
    return w, E


def check_value_range(dtype, device, exact_vectors=True):
    """[vl, vu) between w[99]/w[100] and w[199]/w[200] selects exactly the
    index range, under both tridiagonal solvers. The eigenvalues are always
    compared bitwise; the eigenvectors bitwise too unless ``exact_vectors``
    is off (device GEMMs may reduce in a different order run to run), where
    they meet the residual and orthogonality bounds instead."""
    a0 = make(dtype, device)[1]
    w_all = hermitian_eigenvalues(UpLo.Lower, make(dtype, device)[0])
    vl = 0.5 * (w_all[IB - 1].item() + w_all[IB].item())
    vu = 0.5 * (w_all[IE - 1].item() + w_all[IE].item())
    for solver in ("dc", "bisect"):
        wi, Ei = hermitian_eigensolver(
            UpLo.Lower, make(dtype, device)[0], eigenvalues_index_begin=IB,
            eigenvalues_index_end=IE, tridiag_solver=solver)
        wv, Ev = hermitian_eigensolver(
            UpLo.Lower, make(dtype, device)[0], tridiag_solver=solver,
            eigenvalues_value_range=(vl, vu))
        assert wv.shape == (IE - IB,)
        assert torch.equal(wv, wi), solver
        assert Ev.dist.size == Ei.dist.size
        if exact_vectors:
            assert torch.equal(Ev.to_global(), Ei.to_global()), solver
            continue
        k = IE - IB
        E = Ev.to_global()[:, :k]
        scale = max(1.0, wv.abs().max().item())
        res = (a0 @ E - E @ torch.diag(wv.to(dtype))).abs().max().item()
        orth = (E.mH @ E - torch.eye(k, dtype=dtype, device=E.device)
                ).abs().max().item()
        assert res < 1e-10 * N * scale, f"{solver}: res={res}"
        assert orth < 1e-11 * N, f"{solver}: orth={orth}"


def check_generalized(dtype, device):
    A = Matrix.create(N, N, NB, NB, dtype=dtype, device=device)
    B = Matrix.create(N, N, NB, NB, dtype=dtype, device=device)
    mutil.set_random_hermitian(A, seed=61)
    mutil.set_random_hermitian_positive_definite(B, seed=62)
    a0, b0 = herm(A.to_global()), herm(B.to_global())
    w, evecs = hermitian_generalized_eigensolver(
        UpLo.Lower, A, B, eigenvalues_index_begin=IB,
        eigenvalues_index_end=IE, tridiag_solver="bisect")
    k = IE - IB
    E = evecs.to_global()[:, :k]
    res = (a0 @ E - b0 @ E @ torch.diag(w.to(dtype))).abs().max().item()
    scale = max(1.0, w.abs().max().item())
    borth = (E.mH @ b0 @ E - torch.eye(k, dtype=dtype, device=E.device)
             ).abs().max().item()
    print(f"generalized {dtype} {device}: res = {res:.3e} "
          f"(bound {1e-9 * N * scale:.1e}), borth = {borth:.3e}")
    assert res < 1e-9 * N * scale, f"res={res}"
    assert borth < 1e-9 * N, f"borth={borth}"
