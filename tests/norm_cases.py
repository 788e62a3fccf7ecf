"""Matrix generators, the extended-precision reference and the error bounds
shared by the matrix-norm tests (CPU and GPU).

The reference assembles the matrix that the (structure, uplo, diag) triple
MEANS, as ``numpy.longdouble`` moduli, and takes its norm there; it imports
nothing from the code under test. The bounds are first-order summation bounds
that hold for any order of summation, with ``eps`` that of the input's real
type (the code accumulates in float64, so for float32 inputs they are loose
by design, never tight by luck):

    max        equal for real types; relative 2 eps for complex (one modulus)
    one / inf  relative (t + 2) eps, t = number of terms in the largest sum
    fro        relative (N + 4) eps, N = number of real squares summed
               (a complex element contributes two)

Entries are drawn with |a| <= 0.5, so a padding 1.0 that leaked into a result
would change max, one and inf visibly.
"""

from functools import lru_cache

import numpy as np
import torch

from dlaf_amd import Matrix, UpLo, Diag, matrix_norm

LD = np.longdouble
NORMS = ("max", "one", "inf", "fro")
DTYPES = ("float32", "float64", "complex64", "complex128")

# (m, n, mb, nb) of the issue's table
SHAPES = [
    (32, 32, 16, 16),   # exact tiles
    (37, 29, 16, 16),   # both edges padded
    (5, 5, 8, 8),       # one partial tile: only the padding can go wrong
    (40, 40, 17, 17),   # odd tile size (misaligned tile bases in float32)
    (1, 1, 4, 4),
]
# extra device shapes. The kernel gives one workgroup a strip of 64 rows of a
# tile and walks it in column blocks of 64 vectors (256 columns in float32,
# 128 in float64 / complex64, 64 in complex128 and on the scalar path), and
# takes a mask-free path for a block that lies wholly inside the tile, the
# matrix and the triangle. The first two shapes have several tiles but one
# strip and one block per tile; the others have mb > 64 that is no multiple
# of 64 (several strips, the last one partial), nb above every block width
# (several blocks, the first ones interior, the last one partial), padded
# edges, and diagonals that cross strip and block boundaries. nb=161 is odd,
# so every dtype takes the scalar path there.
GPU_SHAPES = [
    (130, 130, 64, 64),
    (200, 136, 32, 32),
    (300, 300, 160, 160),
    (330, 330, 161, 161),
    (700, 650, 288, 288),
    (520, 520, 512, 512),
]

# (structure, uplo, diag)
VARIANTS = [
    ("general", None, Diag.NonUnit),
    ("hermitian", UpLo.Lower, Diag.NonUnit),
    ("hermitian", UpLo.Upper, Diag.NonUnit),
    ("triangular", UpLo.Lower, Diag.NonUnit),
    ("triangular", UpLo.Upper, Diag.NonUnit),
    ("triangular", UpLo.Lower, Diag.Unit),
    ("triangular", UpLo.Upper, Diag.Unit),
]


def variants_for(m, n):
    return [v for v in VARIANTS if v[0] != "hermitian" or m == n]


def eps_of(dtype: str) -> float:
    return 2.0 ** -23 if dtype in ("float32", "complex64") else 2.0 ** -52


def is_complex(dtype: str) -> bool:
    return dtype.startswith("complex")


@lru_cache(maxsize=None)
def make_general(m, n, dtype):
    """Random m x n numpy array of ``dtype`` with |a| <= 0.5."""
    rng = np.random.default_rng(1000 * m + n + len(dtype))
    if is_complex(dtype):
        a = (rng.uniform(-0.35, 0.35, (m, n))
             + 1j * rng.uniform(-0.35, 0.35, (m, n)))
    else:
        a = rng.uniform(-0.5, 0.5, (m, n))
    a = a.astype(dtype)
    a.setflags(write=False)
    return a


def to_matrix(a, mb, nb, device="cpu", grid=None):
    m, n = a.shape
    mat = Matrix.create(m, n, mb, nb, dtype=getattr(torch, a.dtype.name),
                        device=device, grid=grid)
    if a.size:
        mat.set_from_global(torch.from_numpy(np.array(a)))
    return mat


def effective_parts(a, structure, uplo, diag):
    """(re, im) longdouble parts of the full matrix that the stored array
    ``a`` stands for; im is None for real input."""
    m, n = a.shape
    re = np.real(a).astype(LD)
    im = np.imag(a).astype(LD) if np.iscomplexobj(a) else None
    if structure == "general":
        return re, im
    i, j = np.indices((m, n))
    keep = (j <= i) if uplo == UpLo.Lower else (j >= i)
    dg = i == j
    re = np.where(keep, re, LD(0))
    if im is not None:
        im = np.where(keep, im, LD(0))
    if structure == "hermitian":
        if im is not None:
            im = np.where(dg, LD(0), im)
        strict = keep & ~dg
        re = re + np.where(strict, re, LD(0)).T
        if im is not None:
            im = im - np.where(strict, im, LD(0)).T
    elif diag == Diag.Unit:
        re = np.where(dg, LD(1), re)
        if im is not None:
            im = np.where(dg, LD(0), im)
    return re, im


def reference(a, structure="general", uplo=None, diag=Diag.NonUnit):
    """{norm: (longdouble value, terms)}: ``terms`` is t for one / inf, N for
    fro and unused for max."""
    m, n = a.shape
    if m == 0 or n == 0:
        return {k: (LD(0), 0) for k in NORMS}
    re, im = effective_parts(a, structure, uplo, diag)
    mod = np.abs(re) if im is None else np.hypot(re, im)
    sq = re * re if im is None else re * re + im * im
    nsq = m * n * (1 if im is None else 2)
    return {
        "max": (mod.max(), 0),
        "one": (mod.sum(axis=0).max(), m),
        "inf": (mod.sum(axis=1).max(), n),
        "fro": (np.sqrt(sq.sum()), nsq),
    }


def bound(norm, dtype, terms):
    """Relative error bound of the module docstring."""
    eps = eps_of(dtype)
    if norm == "max":
        return 2 * eps if is_complex(dtype) else 0.0
    if norm in ("one", "inf"):
        return (terms + 2) * eps
    return (terms + 4) * eps


def within(got, ref, rel):
    """|got - ref| <= rel * ref, evaluated in longdouble."""
    return abs(LD(got) - ref) <= LD(rel) * abs(ref)


def all_norms(mat, structure, uplo, diag, grid=None):
    return {k: matrix_norm(k, mat, uplo=uplo, structure=structure, diag=diag,
                           grid=grid) for k in NORMS}


def check_against_reference(got, a, dtype, structure, uplo, diag, factor=1.0):
    ref = reference(a, structure, uplo, diag)
    for k in NORMS:
        val, terms = ref[k]
        rel = factor * bound(k, dtype, terms)
        print(f"{k}: got={got[k]!r} ref={float(val)!r} "
              f"rel={float(abs(LD(got[k]) - val) / val) if val else 0.0:.3e} "
              f"bound={rel:.3e}")
        if rel == 0.0:
            assert got[k] == float(val), (k, got[k], float(val))
        else:
            assert within(got[k], val, rel), (k, got[k], float(val), rel)


def stored_with_garbage(a, structure, uplo, diag):
    """``a`` with everything the structure must not read set to 1e30: the
    other triangle, the imaginary part of a Hermitian diagonal (set nonzero),
    a unit diagonal."""
    if structure == "general":
        return a
    m, n = a.shape
    s = np.array(a)
    i, j = np.indices((m, n))
    other = (j > i) if uplo == UpLo.Lower else (j < i)
    s[other] = 1e30
    dg = i == j
    if structure == "hermitian" and np.iscomplexobj(s):
        s[dg] = np.real(s[dg]) + 0.25j
    if structure == "triangular" and diag == Diag.Unit:
        s[dg] = 1e30
    return s


def check_case(m, n, mb, nb, dtype, structure, uplo, diag, device):
    """The table check: every norm of one (shape, dtype, variant) on
    ``device`` against the longdouble reference; with a triangle, the result
    must not depend on what the unread part of the storage holds."""
    a = make_general(m, n, dtype)
    stored = stored_with_garbage(a, structure, uplo, diag)
    got = all_norms(to_matrix(stored, mb, nb, device), structure, uplo, diag)
    check_against_reference(got, stored, dtype, structure, uplo, diag)
    if structure == "hermitian":
        # equal to the general norm of the assembled full matrix
        re, im = effective_parts(stored, structure, uplo, diag)
        full = (re if im is None else re + 1j * im).astype(dtype)
        check_against_reference(got, full, dtype, "general", None,
                                Diag.NonUnit)
    return got


def check_nan_inf(device, dtype="float64"):
    m = n = 21
    for structure, uplo in (("general", None), ("hermitian", UpLo.Lower),
                            ("triangular", UpLo.Upper)):
        pos = (13, 4) if uplo != UpLo.Upper else (4, 13)
        for bad in (np.nan, np.inf):
            a = np.array(make_general(m, n, dtype))
            a[pos] = bad
            got = all_norms(to_matrix(a, 8, 8, device), structure, uplo,
                            Diag.NonUnit)
            for k in NORMS:
                if bad != bad:
                    assert got[k] != got[k], (structure, k, got[k])
                else:
                    assert got[k] == np.inf, (structure, k, got[k])


def check_fro_extremes(device):
    n, nb = 24, 8
    sign = np.where(np.indices((n, n)).sum(axis=0) % 2 == 0, 1.0, -1.0)
    for p in (600, -600):
        a = sign * 2.0 ** p
        got = matrix_norm("fro", to_matrix(a, nb, nb, device))
        assert got == 24 * 2.0 ** p, (p, got)
    a = np.ones((n, n))
    a[5, 17] = 2.0 ** 600
    got = matrix_norm("fro", to_matrix(a, nb, nb, device))
    ref, terms = reference(a)["fro"]
    assert within(got, ref, bound("fro", "float64", terms)), (got, float(ref))
