"""Inputs, the 50-digit reference and the checks shared by the secular-root
tests: the torch path on the CPU (``test_secular.py``) and the HIP kernels of
csrc/secular.hip (``test_gpu_secular.py``).

The solver returns the roots of f(lam) = 1 + rho sum_i z_i^2 / (d_i - lam) as
(sidx, mu), lam_j = d[sidx_j] + mu_j. Inputs are what the merge passes after
deflation: d ascending, ||z|| = 1, rho > 0, and every pole gap and every
rho |z_i| above 8 eps max(max|d|, rho) (``check_legal``). d and z are numpy
float64 from fixed seeds; z2 = z * z is the float64 product, the number the
kernel receives.

    random-K   d sorted normal, z normal, rho 1.7; K = 2, 3, 5, 127, 128, 129,
               131: 127 / 128 / 129 straddle the switch between the two
               kernels, 129 and 131 leave a partial last workgroup in the
               wave-per-root kernel (4 roots per workgroup)
    at k = 130:
    pairs        65 poles on linspace(-1, 1), each with a twin at +1e-13
    clusters     10 clusters of 13 poles spaced 1e-12, rho 0.5
    graded-z     z = 10^(-7 U[0, 1))
    log-d        d = logspace(-8, 0)
    rho-1e-6, rho-1e6   d = linspace(0, 1), z normal
    one-heavy    z = [1, 1e-6, ...], rho 2
    heavy-last   z = [..., 1e-6, 1], rho 2

Reference: mpmath at 50 digits. With delta_ij = (d_i - d_p) - mu_j formed from
the returned pair, f and f' are evaluated there; |f / f'| is the distance to
the true root (a Newton step, quadratically accurate from any point the solver
returns), and zhat_i = sqrt(prod_j |delta_ij| / (rho prod_{j != i} |d_j - d_i|))
is the Gu / Eisenstat vector the roots are exact for.

Assertions (eps = 2^-52):

    A  sidx_j in {j, j + 1}, sidx_{k-1} = k - 1; mu_j strictly inside its open
       pole gap in shifted coordinates, the last strictly inside (0, rho): mu
       is never 0, which would put an inf into U
    B  |f / f'| <= 4 eps (max|d| + rho) for every root. Rounding d_p + mu alone
       costs 0.5 in these units.
    C  max_i |zhat_i - |z_i|| <= 4 k eps: what Gu / Eisenstat needs
    D  U built from the returned roots by the merge's own assembly
       (``tridiag_dc._secular_eigvecs``):
       max|A U - U Lambda| <= 8 k eps max|A|, max|U^T U - I| <= 8 k eps,
       A = diag(d) + rho z z^T in float64

The bounds were fixed on the CPU path before the kernel ran. Its maxima over
all cases are B 0.36, C 0.17 (random-3; at most 0.003 from k = 127 on), D 1.80
and 5.00 of the units above.

Recorded, not asserted: the root error relative to the nearer pole gap,
max_j |f / f'| / min_i |delta_ij|, in units of eps. The iteration runs on a
fixed budget (40 rational + 24 Illinois steps) with exits relative to the
root's offset from its pole; stopping on a laed4-style criterion is a
follow-up. Per-case maxima (torch path on the CPU, HIP kernel on an MI355X):

                  torch     kernel
    random-2      0.28      0.76
    random-3      1.7       0.72
    random-5      1.2       0.41
    random-127    3.6       12
    random-128    4.5       2.7
    random-129    11        10
    random-131    64        160
    pairs         7.8       2.2
    clusters      3.3       4.7
    graded-z      510       160
    log-d         6.2       7.3
    rho-1e-6      1.0e3     1.4
    rho-1e6       52        25
    one-heavy     4.4e5     3.7e5
    heavy-last    2.4       2.2

one-heavy leaves roots next to the light poles at 4e5 eps of their gap in both
paths; z-hat absorbs it (C 0.004, D 0.03 and 0.1 there). Before its exit was
made relative, the torch path left ``clusters`` at 2.9e8 eps, with C at 3.9e4
and the residual of D at 1.3e4.
"""

import math
from functools import lru_cache

import mpmath
import numpy as np
import torch

EPS = 2.0 ** -52
K_BIG = 130
RANDOM_K = (2, 3, 5, 127, 128, 129, 131)
NAMES = tuple(f"random-{k}" for k in RANDOM_K) + (
    "pairs", "clusters", "graded-z", "log-d", "rho-1e-6", "rho-1e6",
    "one-heavy", "heavy-last")

B_C = 4.0      # |f/f'| <= B_C eps (max|d| + rho)
C_C = 4.0      # zhat error <= C_C k eps
D_C = 8.0      # residual and orthogonality of U


def _unit(z):
    return z / np.linalg.norm(z)


@lru_cache(maxsize=None)
def case(name: str):
    """(d [k], z [k], rho): numpy float64, read-only."""
    rng = np.random.default_rng(1000 + NAMES.index(name))
    k = K_BIG
    if name.startswith("random-"):
        k = int(name.split("-")[1])
        d, z, rho = np.sort(rng.standard_normal(k)), rng.standard_normal(k), 1.7
    elif name == "pairs":
        base = np.linspace(-1.0, 1.0, k // 2)
        d = np.sort(np.concatenate([base, base + 1e-13]))
        z, rho = rng.standard_normal(k), 1.0
    elif name == "clusters":
        centres = np.linspace(-1.0, 1.0, 10)
        d = np.sort((centres[:, None] + 1e-12 * np.arange(13)[None, :]).ravel())
        z, rho = rng.standard_normal(k), 0.5
    elif name == "graded-z":
        d = np.linspace(-1.0, 1.0, k)
        z, rho = 10.0 ** (-7.0 * rng.random(k)), 1.0
    elif name == "log-d":
        d = np.logspace(-8, 0, k)
        z, rho = rng.standard_normal(k), 1.0
    elif name in ("rho-1e-6", "rho-1e6"):
        d = np.linspace(0.0, 1.0, k)
        z, rho = rng.standard_normal(k), float(name[4:])
    elif name in ("one-heavy", "heavy-last"):
        d = np.linspace(-1.0, 1.0, k)
        z = np.full(k, 1e-6)
        z[0 if name == "one-heavy" else -1] = 1.0
        rho = 2.0
    else:
        raise ValueError(name)
    z = _unit(z)
    check_legal(d, z, rho)
    d.setflags(write=False)
    z.setflags(write=False)
    return d, z, rho


def check_legal(d, z, rho):
    """What the merge guarantees after deflation."""
    tol = 8.0 * EPS * max(np.abs(d).max(), rho)
    assert rho > 0 and abs(np.linalg.norm(z) - 1.0) < 4 * EPS
    assert (np.diff(d) > tol).all(), "pole gap below the deflation tolerance"
    assert (rho * np.abs(z) > tol).all(), "weight below the deflation tolerance"


def reference(d, z, rho, sidx, mu):
    """50-digit figures of the returned roots: (|f/f'| [k], min_i|delta_ij|
    [k], zhat [k]) as floats."""
    k = len(d)
    with mpmath.workprec(170):
        mp = mpmath.mpf
        dm = [mp(float(x)) for x in d]
        z2 = [mp(float(x)) for x in (z * z)]        # the float64 product
        r = mp(rho)
        num = [mp(1)] * k
        step, gap = [], []
        for j in range(k):
            dp, m = dm[int(sidx[j])], mp(float(mu[j]))
            f, fp, mn = mp(1), mp(0), None
            for i in range(k):
                delta = (dm[i] - dp) - m
                t = z2[i] / delta
                f += r * t
                fp += r * t / delta
                a = abs(delta)
                mn = a if mn is None or a < mn else mn
                num[i] *= a
            step.append(float(abs(f / fp)))
            gap.append(float(mn))
        zhat = []
        for i in range(k):
            den = r
            for j in range(k):
                if j != i:
                    den *= abs(dm[j] - dm[i])
            zhat.append(float(mpmath.sqrt(num[i] / den)))
    return np.array(step), np.array(gap), np.array(zhat)


def eigvecs(d, z, rho, sidx, mu):
    """(lam, U) from the returned roots by the merge's own eigenvector
    assembly (``tridiag_dc._secular_eigvecs``, float64 on the host)."""
    from dlaf_amd.algs.tridiag_dc import _secular_eigvecs
    lam, U = _secular_eigvecs(torch.from_numpy(np.array(d)),
                              torch.from_numpy(np.array(z)), rho,
                              torch.as_tensor(sidx, dtype=torch.int64),
                              torch.as_tensor(mu, dtype=torch.float64))
    return lam.numpy(), U.numpy()


def figures(name, sidx, mu):
    """Assertion A (exact), then the figures of B, C, D in their units and
    the recorded gap-relative error in eps."""
    d, z, rho = case(name)
    k = len(d)
    sidx = np.asarray(sidx, dtype=np.int64)
    mu = np.asarray(mu, dtype=np.float64)
    assert sidx.shape == (k,) and mu.shape == (k,)
    # A
    j = np.arange(k)
    assert ((sidx == j) | (sidx == j + 1)).all(), f"{name}: sidx {sidx}"
    assert sidx[k - 1] == k - 1, f"{name}: last root shifted to {sidx[k - 1]}"
    assert np.isfinite(mu).all(), f"{name}: non-finite mu"
    width = np.append(np.diff(d), rho)               # exact float64 gaps
    left = sidx == j
    inside = np.where(left, (mu > 0) & (mu < width), (mu < 0) & (mu > -width))
    assert inside.all(), \
        f"{name}: roots {np.nonzero(~inside)[0]} not strictly inside their " \
        f"gap, mu={mu[~inside]}, width={width[~inside]}"
    # B, C and the recorded figure
    step, gap, zhat = reference(d, z, rho, sidx, mu)
    fig = {
        "B": step.max() / (EPS * (np.abs(d).max() + rho)),
        "C": np.abs(zhat - np.abs(z)).max() / (k * EPS),
        "gap": (step / gap).max() / EPS,
    }
    # D
    lam, U = eigvecs(d, z, rho, sidx, mu)
    A = np.diag(d) + rho * np.outer(z, z)
    fig["D_res"] = (np.abs(A @ U - U * lam[None, :]).max()
                    / (k * EPS * np.abs(A).max()))
    fig["D_orth"] = np.abs(U.T @ U - np.eye(k)).max() / (k * EPS)
    return {key: float(v) for key, v in fig.items()}


def check(name, sidx, mu, tag):
    fig = figures(name, sidx, mu)
    print(f"SECFIG {tag} {name} B={fig['B']:.3g} C={fig['C']:.3g} "
          f"D_res={fig['D_res']:.3g} D_orth={fig['D_orth']:.3g} "
          f"gap={fig['gap']:.3g}")
    for key, bound in (("B", B_C), ("C", C_C), ("D_res", D_C),
                       ("D_orth", D_C)):
        assert math.isfinite(fig[key]) and fig[key] <= bound, \
            f"{tag} {name}: {key} = {fig[key]:.3g} > {bound}"
    return fig
