"""Panels, matrices and the checks shared by the reduction-to-band tests (CPU
and GPU).

Reduction to band is the panel QR (``panel_qr_``), the compact-WY T factor
(``t_factor`` on top of ``tri_inverse_full``), the two-sided trailing update
(``reduction_to_band_dense``) and the back-transform
(``bt_reduction_to_band``). Every check is against the input itself and an
orthogonal factor that is independent of the project:

    Q_ref = H_0 H_1 ...,   H_j = I - tau_j v_j v_j^H

with ``v_j`` (a unit 1 followed by the stored tail) and ``tau_j`` read from
the output and the product accumulated column by column on the host in
float64 / complex128. ``t_factor`` never enters ``Q_ref``.

Every figure is evaluated on the host in float64 / complex128 with
``eps = finfo(dtype).eps`` of the tested dtype. Inputs are generated in
float64 and rounded to the tested dtype before the reference sees them, so
the reference works on exactly the numbers the kernels get.

    panel QR (m x nb), unit max(m, 2) eps
        rec    max|Q_ref R - P0| / max|P0|            R = triu(output)
        orth   max|Q_ref^H Q_ref - I|
        LAPACK convention: Im R_jj == 0 exactly; tau == 0 exactly or
        1 <= Re tau <= 2 and |tau - 1| <= 1 (slack 4 eps), which pins the
        sign of beta without a forward comparison
    triangular inverse (n x n), unit max(n, 2) eps
        left   max|A T - I| / max(|A| |T|)
        right  max|T A - I| / max(|T| |A|)
        the other triangle of T exactly zero
    T factor (m x k), unit m eps
        wy     max|(I - V T V^H) - Q_ref|
        T upper triangular; rows and columns of zero taus exactly zero
    whole stage (n, band), unit n eps
        sim    max|Q_ref^H A0 Q_ref - B| / max|A0|
        orth   max|Q_ref^H Q_ref - I|
        eig    max|eigvalsh(B) - eigvalsh(A0)| / max|w|
        bt     max|bt_reduction_to_band(I) - Q_ref|   (the only one that
               involves t_factor)

C = 8 is the band stage's bound (``band_stage_cases.py``) and was fixed
before any kernel ran. The project's CPU path reaches at most, over all
shapes, kinds, dtypes and both layouts below:

    panel QR            rec   0.89   orth  1.21   ((3, 5) complex64 dup, orth)
    whole stage         sim   0.66   orth  0.67   eig 0.74   bt 0.37
                        ((5, 2) float64 holes, eig)
    triangular inverse  left  0.25   right 0.25   (n = 2)
    T factor            wy    0.12

which leaves about 6x for the kernels' different summation order. The device
figures are in ``test_gpu_red2band.py``.

Panel kinds (``randn`` entries, seeded by shape, dtype and kind):

    rand
    holes   columns 0, 3, ... entirely zero (tau == 0, column untouched);
            columns 1, 4, ... with a zero tail below a kept diagonal: column
            1 is degenerate in the real dtypes and a pure phase
            (|tau - 1| = 1) in the complex ones
    graded  rows scaled by logspace(0, -6, m)
    dup     the right half of the columns copies the left half: rank
            deficient, so there is no forward comparison to make; the
            backward figures above do not depend on the rank

Every panel runs twice: contiguous, and as the column window ``buf[:, 3:3+nb]``
of an ``[m, nb + 7]`` buffer whose 7 foreign columns hold NaN and must come
back bitwise unchanged, as must a guard element behind ``taus``. That window
has unit column stride, which is what every production call passes.

Stage kinds (Hermitian, real diagonal): ``rand``; ``holes`` (every third
column empty below the band); ``banded`` (already of bandwidth ``band``: in
the real dtypes every tau is exactly 0 and the lower triangle is bitwise
unchanged, in the complex dtypes the reflectors are pure phases, as in LAPACK,
and everything below the band stays exactly zero); ``graded``
(s_i a_ij s_j, s = logspace(0, -6, n)).

Nothing is scaled outside the safe range: the eigensolver rescales before this
stage, so that is the kernels' contract.
"""

import math
import warnings
from functools import lru_cache

import numpy as np
import torch

from dlaf_amd.algs.red2band import (bt_reduction_to_band, panel_qr_,
                                    reduction_to_band_dense, t_factor)
from dlaf_amd.ops import tile_ops as ops

DTYPES = ("float32", "float64", "complex64", "complex128")

C = 8.0

# (m, nb): the smallest shapes at which each loop of the kernel can go wrong
PANEL_SHAPES = [
    (1, 1), (2, 1), (5, 3),
    (3, 5),              # m < nb: the last reflector has no tail
    (64, 64),            # square: last column degenerate (real) / a phase
    (65, 64),
    (100, 128),          # m < nb with 2 nb tasks > 128 blocks
    (129, 128),
    (300, 64),
    (520, 16),           # second trip of the 2 x 256-row reducer loop
    (777, 64),           # phase-B grid-stride loop taken more than once
    (600, 128),          # task loop twice, phase-B loop more than once
]
PANEL_KINDS = ("rand", "holes", "graded", "dup")
LAYOUTS = ("contig", "window")
WINDOW_LEFT, WINDOW_EXTRA = 3, 7

TRI_SIZES = [1, 2, 63, 64, 65, 100, 128, 129, 200, 300]

TFACTOR_SHAPES = [(4, 1), (9, 5), (70, 64), (140, 100), (140, 128),
                  (140, 129), (210, 200)]

# (n, band)
STAGE_SHAPES = [
    (3, 1), (5, 2), (9, 4),
    (17, 16),            # n = b + 1: a 1 x 1 panel
    (18, 16),
    (33, 16),
    (40, 16),            # capped last panel, bw = 8 < band
    (37, 8),
    (97, 5),             # odd band
    (130, 64), (200, 64),
    (150, 128),          # one capped panel only
    (257, 128),          # bw = 1 last panel
    (300, 128),          # full panel, then a capped 44-wide one
]
STAGE_KINDS = ("rand", "holes", "banded", "graded")

GUARD = 12345.0


def torch_dtype(dtype: str) -> torch.dtype:
    return getattr(torch, dtype)


def eps_of(dtype: str) -> float:
    return float(torch.finfo(torch_dtype(dtype)).eps)


def is_complex(dtype: str) -> bool:
    return dtype.startswith("complex")


def wide(dtype: str) -> torch.dtype:
    return torch.complex128 if is_complex(dtype) else torch.float64


def _seed(tag: int, a: int, b: int, dtype: str, kind: int) -> int:
    return (((tag * 1009 + a) * 1009 + b) * 4 + DTYPES.index(dtype)) * 5 + kind


def _randn(shape, dtype: str, g) -> torch.Tensor:
    a = torch.randn(*shape, generator=g, dtype=torch.float64)
    if is_complex(dtype):
        a = torch.complex(a, torch.randn(*shape, generator=g,
                                         dtype=torch.float64))
    return a


def bits(t: torch.Tensor) -> torch.Tensor:
    """The bit pattern of a tensor (NaN and signed zeros compare exactly)."""
    t = t.detach().cpu().contiguous()
    if t.is_complex():
        t = torch.view_as_real(t).contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def to_wide_np(t: torch.Tensor, dtype: str) -> np.ndarray:
    return t.detach().cpu().to(wide(dtype)).numpy()


def apply_reflector(Q: np.ndarray, v: np.ndarray, tau, r0: int = 0) -> None:
    """Q <- Q H in place, H = I - tau v v^H acting on rows / columns r0:."""
    if tau == 0:
        return
    Qv = Q[:, r0:] @ v
    Q[:, r0:] -= np.outer(Qv, tau * v.conj())


def q_from_reflectors(a: np.ndarray, taus: np.ndarray) -> np.ndarray:
    """H_0 H_1 ... of a LAPACK-style factored m x k panel, m x m."""
    m = a.shape[0]
    Q = np.eye(m, dtype=a.dtype)
    for j in range(len(taus)):
        v = np.concatenate([np.ones(1, dtype=a.dtype), a[j + 1:, j]])
        apply_reflector(Q, v, taus[j], j)
    return Q


def _check_bound(figs: dict, where: str) -> None:
    for name, v in figs.items():
        assert math.isfinite(v) and v <= C, \
            f"{name} = {v:.3g} > {C} ({where})"


# ---- 1. panel QR -----------------------------------------------------------

@lru_cache(maxsize=None)
def panel(m: int, nb: int, dtype: str, kind: str) -> torch.Tensor:
    """The m x nb panel in ``dtype``: built once per case, never modified."""
    g = torch.Generator().manual_seed(
        _seed(1, m, nb, dtype, PANEL_KINDS.index(kind)))
    a = _randn((m, nb), dtype, g)
    if kind == "holes":
        for j in range(1, nb, 3):
            a[j + 1:, j] = 0
        a[:, 0::3] = 0
    elif kind == "graded":
        a = torch.logspace(0, -6, m, dtype=torch.float64).unsqueeze(1) * a
    elif kind == "dup":
        h = nb // 2
        a[:, h:2 * h] = a[:, :h]
    elif kind != "rand":
        raise ValueError(kind)
    return a.to(torch_dtype(dtype))


def tau_convention_ok(taus: np.ndarray, eps: float) -> bool:
    """Each tau exactly 0, or 1 <= Re tau <= 2 and |tau - 1| <= 1."""
    s = 4 * eps
    nz = taus[taus != 0]
    return bool(np.all((nz.real >= 1 - s) & (nz.real <= 2 + s)
                       & (np.abs(nz - 1) <= 1 + s)))


def run_panel(m: int, nb: int, dtype: str, kind: str, layout: str,
              device="cpu"):
    """Factor one panel in one layout; returns the figures in units of
    max(m, 2) eps after asserting everything that is exact."""
    where = f"{device} {dtype} {kind} {layout} m={m} nb={nb}"
    P0 = panel(m, nb, dtype, kind)
    td = torch_dtype(dtype)
    k = min(m, nb)
    if layout == "window":
        buf = torch.full((m, nb + WINDOW_EXTRA), float("nan"), dtype=td)
        buf[:, WINDOW_LEFT:WINDOW_LEFT + nb] = P0
    else:
        buf = P0.clone()
    buf0 = buf.clone()
    tbuf = torch.zeros(k + 1, dtype=td)
    tbuf[k] = GUARD
    buf, tbuf = buf.to(device), tbuf.to(device)
    P = buf[:, WINDOW_LEFT:WINDOW_LEFT + nb] if layout == "window" else buf
    assert P.stride(1) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        panel_qr_(P, tbuf[:k])
    assert buf.device.type == torch.device(device).type
    if layout == "window":
        assert same_bits(buf[:, :WINDOW_LEFT], buf0[:, :WINDOW_LEFT]), \
            f"columns left of the panel changed ({where})"
        assert same_bits(buf[:, WINDOW_LEFT + nb:],
                         buf0[:, WINDOW_LEFT + nb:]), \
            f"columns right of the panel changed ({where})"
    assert same_bits(tbuf[k:], torch.full((1,), GUARD, dtype=td)), \
        f"element behind taus changed ({where})"

    out = P.cpu()
    a = to_wide_np(out, dtype)
    taus = to_wide_np(tbuf[:k], dtype)
    p0 = to_wide_np(P0, dtype)
    eps = eps_of(dtype)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(taus)), where

    # LAPACK convention
    if is_complex(dtype):
        assert np.all(np.diagonal(a)[:k].imag == 0), \
            f"complex diagonal of R ({where})"
    assert tau_convention_ok(taus, eps), f"taus {taus} ({where})"

    # degenerate columns
    if kind == "holes":
        assert taus[0] == 0, f"tau[0] = {taus[0]} ({where})"
        assert same_bits(out[:, 0], P0[:, 0]), f"zero column changed ({where})"
        if k >= 2 and m >= 3:
            if is_complex(dtype):
                assert taus[1] != 0 and abs(abs(taus[1] - 1) - 1) <= 4 * eps, \
                    f"zero tail, complex diagonal: tau = {taus[1]} ({where})"
                assert np.all(a[2:, 1] == 0), where
            else:
                assert taus[1] == 0, f"tau[1] = {taus[1]} ({where})"
                assert same_bits(out[:, 1], P0[:, 1]), where
    if (m, nb) == (64, 64):
        if not is_complex(dtype):
            assert taus[-1] == 0, f"last tau = {taus[-1]} ({where})"
        elif kind == "rand":
            assert taus[-1] != 0 and abs(abs(taus[-1] - 1) - 1) <= 4 * eps, \
                f"last tau = {taus[-1]} ({where})"

    Q = q_from_reflectors(a, taus)
    unit = max(m, 2) * eps
    scale = np.abs(p0).max()
    rec = np.abs(Q @ np.triu(a) - p0).max() / (unit * scale) if scale else \
        float(np.abs(Q @ np.triu(a) - p0).max())
    orth = np.abs(Q.conj().T @ Q - np.eye(m)).max() / unit
    return {"rec": float(rec), "orth": float(orth)}


def check_panel(m, nb, dtype, kind, device="cpu", tag="cpu"):
    """Both layouts of one panel case; returns the larger figures."""
    worst = {}
    for layout in LAYOUTS:
        fig = run_panel(m, nb, dtype, kind, layout, device)
        print(f"R2BFIG {tag} panel {dtype} {kind} {layout} m={m} nb={nb} "
              f"rec={fig['rec']:.3f} orth={fig['orth']:.3f}")
        _check_bound(fig, f"{tag} panel {dtype} {kind} {layout} "
                          f"m={m} nb={nb}")
        for key, v in fig.items():
            worst[key] = max(worst.get(key, 0.0), v)
    return worst


# ---- 2. triangular inverse and T factor ------------------------------------

@lru_cache(maxsize=None)
def triangle(n: int, lower: bool, unit: bool, dtype: str):
    """(stored [n, n] in ``dtype`` with garbage outside the triangle, the
    triangular matrix it stands for in float64 / complex128)."""
    g = torch.Generator().manual_seed(
        _seed(2, n, 2 * int(lower) + int(unit), dtype, 0))
    a = _randn((n, n), dtype, g) / math.sqrt(n)
    mod = 1 + torch.rand(n, generator=g, dtype=torch.float64)
    if is_complex(dtype):
        ph = torch.rand(n, generator=g, dtype=torch.float64) * (2 * math.pi)
        diag = torch.polar(mod, ph)
    else:
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        diag = mod * sign.to(torch.float64)
    tri = torch.tril(a, -1) if lower else torch.triu(a, 1)
    tri = tri + torch.diag(diag.to(tri.dtype))
    tri = tri.to(torch_dtype(dtype))                 # what the kernels get
    inside = torch.ones(n, n).tril().bool() if lower else \
        torch.ones(n, n).triu().bool()
    stored = torch.where(inside, tri, torch.full_like(tri, 7.0))
    ref = tri.to(wide(dtype))
    if unit:
        stored = stored.clone()
        stored.diagonal().fill_(7.0)
        ref = ref - torch.diag(torch.diagonal(ref)) + torch.eye(
            n, dtype=ref.dtype)
    return stored, ref.numpy()


def run_tri_inverse(n: int, lower: bool, unit: bool, dtype: str,
                    device="cpu"):
    where = f"{device} {dtype} n={n} lower={lower} unit={unit}"
    stored, A = triangle(n, lower, unit, dtype)
    dev_in = stored.clone().to(device)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T = ops.tri_inverse_full(dev_in, lower=lower, unit=unit)
    assert T.device.type == torch.device(device).type, where
    assert T.shape == (n, n) and T.dtype == stored.dtype, where
    assert same_bits(dev_in, stored), f"input modified ({where})"
    other = torch.triu(T, 1) if lower else torch.tril(T, -1)
    assert bool((other == 0).all()), f"other triangle not zero ({where})"
    Tn = to_wide_np(T, dtype)
    assert np.all(np.isfinite(Tn)), where
    unit_ = max(n, 2) * eps_of(dtype)
    eye = np.eye(n)
    left = np.abs(A @ Tn - eye).max() / (unit_ * (np.abs(A) @ np.abs(Tn)).max())
    right = np.abs(Tn @ A - eye).max() / (unit_
                                          * (np.abs(Tn) @ np.abs(A)).max())
    return {"left": float(left), "right": float(right)}


def check_tri_inverse(n, lower, unit, dtype, device="cpu", tag="cpu"):
    fig = run_tri_inverse(n, lower, unit, dtype, device)
    print(f"R2BFIG {tag} trinv {dtype} n={n} lower={int(lower)} "
          f"unit={int(unit)} left={fig['left']:.3f} right={fig['right']:.3f}")
    _check_bound(fig, f"{tag} trinv {dtype} n={n} lower={lower} unit={unit}")
    return fig


@lru_cache(maxsize=None)
def reflectors(m: int, k: int, dtype: str):
    """(V [m, k], taus [k]) in ``dtype`` from LAPACK's geqrf in float64 /
    complex128 of a panel whose columns 0, 3, ... are zero, and Q_ref of the
    rounded pair."""
    g = torch.Generator().manual_seed(_seed(3, m, k, dtype, 0))
    a = _randn((m, k), dtype, g)
    a[:, 0::3] = 0
    f, taus = torch.geqrf(a)
    td = torch_dtype(dtype)
    V = (torch.tril(f, -1) + torch.eye(m, k, dtype=f.dtype)).to(td)
    taus = taus.to(td)
    Q = q_from_reflectors(to_wide_np(V, dtype), to_wide_np(taus, dtype))
    return V, taus, Q


def run_t_factor(m: int, k: int, dtype: str, device="cpu"):
    where = f"{device} {dtype} m={m} k={k}"
    V, taus, Q = reflectors(m, k, dtype)
    zero = (taus == 0)
    assert bool(zero[0::3].all()) and int(zero.sum()) == len(range(0, k, 3)), \
        f"geqrf did not leave the expected zero taus ({where})"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T = t_factor(V.clone().to(device), taus.clone().to(device))
    assert T.device.type == torch.device(device).type, where
    assert T.shape == (k, k), where
    assert bool((torch.tril(T, -1) == 0).all()), \
        f"T not upper triangular ({where})"
    Tc = T.cpu()
    assert bool((Tc[zero, :] == 0).all()) and bool((Tc[:, zero] == 0).all()), \
        f"rows / columns of zero taus not zero ({where})"
    Tn, Vn = to_wide_np(T, dtype), to_wide_np(V, dtype)
    assert np.all(np.isfinite(Tn)), where
    wy = np.abs((np.eye(m) - Vn @ Tn @ Vn.conj().T) - Q).max() \
        / (m * eps_of(dtype))
    return {"wy": float(wy)}


def check_t_factor(m, k, dtype, device="cpu", tag="cpu"):
    fig = run_t_factor(m, k, dtype, device)
    print(f"R2BFIG {tag} tfactor {dtype} m={m} k={k} wy={fig['wy']:.3f}")
    _check_bound(fig, f"{tag} tfactor {dtype} m={m} k={k}")
    return fig


# ---- 3. the whole stage ----------------------------------------------------

@lru_cache(maxsize=None)
def hermitian(n: int, band: int, dtype: str, kind: str):
    """(A [n, n] full Hermitian in ``dtype``, A0 the same in float64 /
    complex128, eigvalsh(A0)): built once per case, never modified."""
    g = torch.Generator().manual_seed(
        _seed(4, n, band, dtype, STAGE_KINDS.index(kind)))
    a = torch.tril(_randn((n, n), dtype, g))
    if is_complex(dtype):
        a = a - torch.diag(1j * torch.diagonal(a).imag)
    if kind == "holes":
        for j in range(0, n, 3):
            a[j + band + 1:, j] = 0
    elif kind == "banded":
        a = torch.triu(a, -band)
    elif kind == "graded":
        s = torch.logspace(0, -6, n, dtype=torch.float64).to(a.dtype)
        a = s.unsqueeze(1) * a * s.unsqueeze(0)
    elif kind != "rand":
        raise ValueError(kind)
    a = a.to(torch_dtype(dtype))                     # what the kernels get
    A = a + torch.tril(a, -1).mH
    A0 = A.to(wide(dtype)).numpy()
    return A, A0, np.linalg.eigvalsh(A0)


def expected_panels(n: int, band: int):
    """(j0, bw, nrefl) of every panel the stage factors."""
    out = []
    for j0 in range(0, max(n - band, 0), band):
        bw = min(band, n - j0 - band)
        out.append((j0, bw, min(n - j0 - band, bw)))
    return out


class _Dense:
    """The least ``bt_reduction_to_band`` needs of its ``mat_v``."""

    def __init__(self, a: torch.Tensor):
        self._a = a

    def to_global(self) -> torch.Tensor:
        return self._a


def run_stage(n: int, band: int, dtype: str, kind: str, device="cpu"):
    where = f"{device} {dtype} {kind} n={n} band={band}"
    A_in, A0, w0 = hermitian(n, band, dtype, kind)
    td = torch_dtype(dtype)
    dev_type = torch.device(device).type
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        A = A_in.clone().to(device)
        taus_all, panels = reduction_to_band_dense(A, band)
        refl = {"taus": taus_all, "panels": panels, "band": band}
        E = torch.eye(n, dtype=td, device=device)
        bt_reduction_to_band(E, _Dense(A), refl)
    assert [tuple(p) for p in panels] == expected_panels(n, band), where
    assert A.device.type == dev_type and E.device.type == dev_type, where
    for (j0, bw, nrefl), taus in zip(panels, taus_all):
        assert taus.device.type == dev_type and taus.shape == (nrefl,), where

    out = A.cpu()
    a = to_wide_np(out, dtype)
    assert np.all(np.isfinite(a)), where
    eps = eps_of(dtype)

    if kind == "banded":
        if is_complex(dtype):
            assert np.all(np.tril(a, -band - 1) == 0), \
                f"fill-in below the band ({where})"
        else:
            for taus in taus_all:
                assert bool((taus == 0).all()), f"taus {taus} ({where})"
            assert same_bits(torch.tril(out), torch.tril(A_in)), \
                f"banded input changed ({where})"

    Q = np.eye(n, dtype=a.dtype)
    for (j0, bw, nrefl), taus in zip(panels, taus_all):
        r0 = j0 + band
        t = to_wide_np(taus, dtype)
        assert tau_convention_ok(t, eps), f"taus {t} ({where})"
        for c in range(nrefl):
            v = np.concatenate([np.ones(1, dtype=a.dtype),
                                a[r0 + c + 1:, j0 + c]])
            apply_reflector(Q, v, t[c], r0 + c)

    L = np.triu(np.tril(a), -band)
    B = L + np.tril(L, -1).conj().T
    unit = n * eps
    sim = np.abs(Q.conj().T @ A0 @ Q - B).max() / (unit * np.abs(A0).max())
    orth = np.abs(Q.conj().T @ Q - np.eye(n)).max() / unit
    eig = np.abs(np.linalg.eigvalsh(B) - w0).max() / (unit * np.abs(w0).max())
    bt = np.abs(to_wide_np(E, dtype) - Q).max() / unit
    return {"sim": float(sim), "orth": float(orth), "eig": float(eig),
            "bt": float(bt)}


def check_stage(n, band, dtype, kind, device="cpu", tag="cpu"):
    fig = run_stage(n, band, dtype, kind, device)
    print(f"R2BFIG {tag} stage {dtype} {kind} n={n} band={band} "
          f"sim={fig['sim']:.3f} orth={fig['orth']:.3f} "
          f"eig={fig['eig']:.3f} bt={fig['bt']:.3f}")
    _check_bound(fig, f"{tag} stage {dtype} {kind} n={n} band={band}")
    return fig
