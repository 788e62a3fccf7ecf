"""Band matrices and the checks shared by the band-stage tests (CPU and GPU).

The band stage is the bulge chase (``chase_band``) followed by the
back-transform (``bt_band_to_tridiagonal``). Every check is against the dense
band matrix itself, never against another path of the project:

    tri = chase_band(store, b);  Q = bt_band_to_tridiagonal(I_n, tri)
    T   = tridiag(tri.d, tri.e)

    sim   max|Q T Q^H - full|                 <= C n eps max|full|
    orth  max|Q^H Q - I|                      <= C n eps
    eig   max|eigvalsh(T) - eigvalsh(full)|   <= C n eps max|w|

evaluated in float64 / complex128 on the host, ``eps = finfo(dtype).eps`` of
the tested dtype. ``full`` is built from the band entries AFTER rounding to
the tested dtype, so the reference sees exactly the numbers the kernels see.

C = 8 was fixed before any kernel ran: the CPU chase with the torch GEMM
chain reaches at most 1.55 in these units over the whole table below (sim 1.55
at (5, 2) float64 rand, orth 0.80, eig 0.70; at most 0.24 from n = 130 on).
The margin of about 5x is for the kernels' different summation order (4-way
split with a fixed-order LDS reduce in the chase, MFMA accumulation in the
back-transform). The GPU figures are in ``test_gpu_band_stage.py``.

Kinds (``randn`` entries, real diagonal, seeded by shape, dtype and kind):

    rand    lower band, no diagonal dominance
    holes   as rand, every third column (0, 3, 6, ...) of the lower band zero
            before symmetrising: zero reflectors (tau == 0) in the chase and
            masked columns in the T factor
    graded  s_i a_ij s_j, s = logspace(0, -6, n)

Nothing is scaled outside the safe range: the eigensolver rescales before this
stage, so that is the kernels' contract.
"""

import math
import warnings
from functools import lru_cache

import numpy as np
import torch

from dlaf_amd.algs.band2tridiag import bt_band_to_tridiagonal, chase_band

DTYPES = ("float32", "float64", "complex64", "complex128")
KINDS = ("rand", "holes", "graded")

# (n, b): the smallest shapes at which each path can still go wrong
SHAPES = [
    (5, 2), (9, 4),
    (17, 16),            # n = b + 1
    (18, 16),            # n = b + 2
    (65, 64), (66, 64),
    (130, 64),           # n = 2b + 2; one full sweep group of 128
    (67, 16),
    (97, 5),             # odd b, ld no multiple of 4
    (131, 16),           # two sweep groups, the second with a single sweep
    (140, 32),           # bt ring R = 160
    (150, 48),           # bt ring R = 192 with the window height 175 padded
    (200, 64),           # production b: R = 192 at the full LDS
    (300, 16), (300, 64),  # three sweep groups, the last partial (42 sweeps)
]

C = 8.0
BT_GROUP = 128           # sweeps per group the bt kernel is built for


def torch_dtype(dtype: str) -> torch.dtype:
    return getattr(torch, dtype)


def eps_of(dtype: str) -> float:
    return float(torch.finfo(torch_dtype(dtype)).eps)


def wide(dtype: str) -> str:
    return "complex128" if dtype.startswith("complex") else "float64"


def seed_of(n: int, b: int, dtype: str, kind: str) -> int:
    return ((n * 131 + b) * 4 + DTYPES.index(dtype)) * 3 + KINDS.index(kind)


def band(n: int, b: int, dtype: str, kind: str, seed: int):
    """(store [n, 2b] in ``dtype``, full [n, n] in float64 / complex128).

    ``store[j, d] = A[j + d, j]`` for d <= b, zero beyond."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, n, generator=g, dtype=torch.float64)
    if dtype.startswith("complex"):
        a = torch.complex(a, torch.randn(n, n, generator=g,
                                         dtype=torch.float64))
        a = a - torch.diag(1j * torch.diagonal(a).imag)
    a = torch.triu(torch.tril(a), -b)
    if kind == "holes":
        a[:, 0::3] = 0
    elif kind == "graded":
        s = torch.logspace(0, -6, n, dtype=torch.float64).to(a.dtype)
        a = s.unsqueeze(1) * a * s.unsqueeze(0)
    elif kind != "rand":
        raise ValueError(kind)
    a = a.to(torch_dtype(dtype))                   # what the kernels get
    store = torch.zeros((n, 2 * b), dtype=a.dtype)
    for d in range(min(b, n - 1) + 1):
        store[: n - d, d] = torch.diagonal(a, -d)
    aw = a.to(torch_dtype(wide(dtype)))
    full = aw + torch.tril(aw, -1).mH
    return store, full


@lru_cache(maxsize=None)
def case(n: int, b: int, dtype: str, kind: str):
    """(store, full, w_full): built once per case, never modified."""
    store, full = band(n, b, dtype, kind, seed_of(n, b, dtype, kind))
    w = np.linalg.eigvalsh(full.numpy())
    return store, full, w


def sweep_groups(n: int) -> int:
    return -(-(n - 2) // BT_GROUP)


def bt_kernel_expected(n: int, b: int, dtype: str) -> bool:
    """The whole-group bt kernel covers f64 / c128, b % 16 == 0 and groups of
    128 sweeps (n - 2 >= 128)."""
    return n >= BT_GROUP + 2 and b % 16 == 0 and dtype in ("float64",
                                                           "complex128")


def run_case(n: int, b: int, dtype: str, kind: str, device="cpu",
             expect_gpu_chase=None):
    """Chase + back-transform of one case on ``device``; returns the three
    figures in units of n eps scale. Warnings are errors, so the bounded-spin
    fallback of the GPU chase cannot pass for the kernel."""
    store0, full, w_full = case(n, b, dtype, kind)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        store = store0.clone().to(device)
        tri = chase_band(store, b)
        if expect_gpu_chase is not None:
            assert tri.vstore.is_cuda == expect_gpu_chase, \
                f"chase ran on {tri.vstore.device}"
        Q = torch.eye(n, dtype=store0.dtype, device=device)
        bt_band_to_tridiagonal(Q, tri)
    Q = Q.cpu().to(full.dtype).numpy()
    d = tri.d.cpu().to(torch.float64).numpy()
    e = tri.e.cpu().to(torch.float64).numpy()
    assert d.shape == (n,) and e.shape == (n - 1,)
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    A = full.numpy()
    unit = n * eps_of(dtype)
    sim = np.abs(Q @ T @ Q.conj().T - A).max() / (unit * np.abs(A).max())
    orth = np.abs(Q.conj().T @ Q - np.eye(n)).max() / unit
    eig = (np.abs(np.linalg.eigvalsh(T) - w_full).max()
           / (unit * np.abs(w_full).max()))
    return {"sim": float(sim), "orth": float(orth), "eig": float(eig)}


def check_case(n: int, b: int, dtype: str, kind: str, device="cpu",
               expect_gpu_chase=None, tag="cpu"):
    fig = run_case(n, b, dtype, kind, device, expect_gpu_chase)
    print(f"BANDFIG {tag} {dtype} {kind} n={n} b={b} sim={fig['sim']:.3f} "
          f"orth={fig['orth']:.3f} eig={fig['eig']:.3f}")
    for name, v in fig.items():
        assert math.isfinite(v) and v <= C, \
            f"{name} = {v:.3g} n eps scale > {C} ({tag} {dtype} {kind} " \
            f"n={n} b={b})"
    return fig
