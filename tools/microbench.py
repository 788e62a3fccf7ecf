#!/usr/bin/env python3
"""Kernel microbenchmarks on one MI355X: fused GEMM TF/s, potrf/trtri latency.

``--hemv [n nb]``: the Hermitian vector-product kernel against the floor of
reading the stored triangle once at 6.3 TB/s and against
``hermitian_multiplication`` on n x nrhs (the per-column crossover).
``--mixed [n nb]``: ``cholesky_solve_mixed`` against the float64
factorization and solve. ``--trsm``: the Cholesky panel solve, gemm_fused
launches against the single-launch kernel. Each runs alone, without the
default list."""

import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

from dlaf_amd.ops import tile_ops as ops
from dlaf_amd.types import Op


def bench_gemm(dtype=torch.float64, nb=512, ntiles=128, iters=10, opB=Op.Trans, inplace=False):
    dev = "cuda"
    A = torch.randn(ntiles, nb, nb, dtype=dtype, device=dev) if not dtype.is_complex else (
        torch.randn(ntiles, nb, nb, dtype=torch.float64, device=dev)
        + 1j * torch.randn(ntiles, nb, nb, dtype=torch.float64, device=dev)).to(dtype)
    C = torch.zeros_like(A)
    ts = nb * nb
    offs = [i * ts for i in range(ntiles)]
    descs = ops.make_descs(offs, offs, offs)
    dt = torch.from_numpy(descs).to(dev)
    # warmup
    for _ in range(3):
        ops.gemm_fused(C, A, A, dt, nb, nb, nb, nb, nb, nb, Op.NoTrans, opB, -1.0, 1.0, inplace=inplace)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        ops.gemm_fused(C, A, A, dt, nb, nb, nb, nb, nb, nb, Op.NoTrans, opB, -1.0, 1.0, inplace=inplace)
    torch.cuda.synchronize()
    dt_s = (time.perf_counter() - t0) / iters
    flops = 2.0 * ntiles * nb * nb * nb * (4 if dtype.is_complex else 1)
    print(f"gemm {dtype} nb={nb} ntiles={ntiles} opB={opB} bn128={inplace}: {dt_s*1e3:.2f} ms  "
          f"{flops/dt_s/1e12:.2f} TFLOP/s")


def bench_torch_bmm(dtype=torch.float64, nb=512, ntiles=128, iters=10):
    """rocBLAS batched GEMM baseline for the same shape (library comparison)."""
    dev = "cuda"
    A = torch.randn(ntiles, nb, nb, dtype=dtype, device=dev) if not dtype.is_complex else (
        torch.randn(ntiles, nb, nb, dtype=torch.float64, device=dev)
        + 1j * torch.randn(ntiles, nb, nb, dtype=torch.float64, device=dev)).to(dtype)
    C = torch.zeros_like(A)
    for _ in range(3):
        torch.bmm(A, A.mT, out=C)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        torch.bmm(A, A.mT, out=C)
    torch.cuda.synchronize()
    dt_s = (time.perf_counter() - t0) / iters
    flops = 2.0 * ntiles * nb * nb * nb * (4 if dtype.is_complex else 1)
    print(f"torch.bmm {dtype} nb={nb} ntiles={ntiles}: {dt_s*1e3:.2f} ms  "
          f"{flops/dt_s/1e12:.2f} TFLOP/s")


def bench_big_dgemm(dtype=torch.float64, n=16384, iters=5):
    """Single large library DGEMM: the machine speed-of-light reference."""
    a = torch.randn(n, n, dtype=dtype, device="cuda")
    c = torch.zeros_like(a)
    for _ in range(2):
        torch.mm(a, a.mT, out=c)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        torch.mm(a, a.mT, out=c)
    torch.cuda.synchronize()
    dt_s = (time.perf_counter() - t0) / iters
    print(f"torch.mm {dtype} n={n}: {dt_s*1e3:.1f} ms  {2*n**3/dt_s/1e12:.2f} TFLOP/s")


def bench_potrf(dtype=torch.float64, nb=512, iters=20):
    a = torch.randn(nb, nb, dtype=dtype, device="cuda")
    a = a @ a.mH + nb * torch.eye(nb, dtype=dtype, device="cuda")
    t = a.clone()
    dinv = ops.dinv_workspace(nb, dtype, "cuda")
    for _ in range(3):
        t.copy_(a)
        ops.potrf_tile(t, dinv)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        t.copy_(a)
        ops.potrf_tile(t, dinv)
    torch.cuda.synchronize()
    dt_s = (time.perf_counter() - t0) / iters
    print(f"potrf_tile {dtype} nb={nb}: {dt_s*1e6:.0f} us")


def bench_trtri(dtype=torch.float64, nb=512, iters=20):
    L = torch.tril(torch.randn(nb, nb, dtype=dtype, device="cuda")) + \
        2 * nb * torch.eye(nb, dtype=dtype, device="cuda")
    T = torch.empty_like(L)
    for _ in range(3):
        ops.tri_inverse_full(L, lower=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        ops.tri_inverse_full(L, lower=True)
    torch.cuda.synchronize()
    dt_s = (time.perf_counter() - t0) / iters
    print(f"trtri_tile {dtype} nb={nb}: {dt_s*1e6:.0f} us")



def bench_lib_batched(dtype=torch.float64, nb=512, nt=63, iters=5):
    """rocBLAS batched vs fused kernel on the POTRF trailing geometry:
    C[i,j] -= P[i] @ P[j]^T over the lower triangle (i >= j)."""
    from dlaf_amd.ops import tile_ops as ops
    from dlaf_amd.types import Op
    dev = "cuda"
    panel = torch.randn(nt, nb, nb, dtype=dtype, device=dev) if not dtype.is_complex \
        else torch.randn(nt, nb, nb, dtype=dtype, device=dev)
    items = [(i, j) for j in range(nt) for i in range(j, nt)]
    ntc = len(items)
    C = torch.randn(ntc, nb, nb, dtype=dtype, device=dev)
    C2 = C.clone()
    offc = [e * nb * nb for e in range(ntc)]
    offa = [i * nb * nb for i, _ in items]
    offb = [j * nb * nb for _, j in items]
    pC, pA, pB = (ops.ptr_array(C, offc), ops.ptr_array(panel, offa),
                  ops.ptr_array(panel, offb))
    pC2 = ops.ptr_array(C2, offc)
    d = ops.make_descs(offc, offa, offb)
    opB = Op.ConjTrans if dtype.is_complex else Op.Trans
    # numerics: lib vs fused
    ops.gemm_fused(C.reshape(-1), panel.reshape(-1), panel.reshape(-1), d,
                   nb, nb, nb, nb, nb, nb, Op.NoTrans, opB, -1.0, 1.0)
    ops.gemm_batched_lib(C2, pC2, pA, pB, nb, nb, nb, nb, nb, nb,
                         Op.NoTrans, opB, -1.0, 1.0)
    torch.cuda.synchronize()
    print(f"lib vs fused max diff: {(C - C2).abs().max().item():.3e}")
    import time
    for tag, fn in (
        ("fused", lambda: ops.gemm_fused(C.reshape(-1), panel.reshape(-1),
                                         panel.reshape(-1), d, nb, nb, nb, nb, nb, nb,
                                         Op.NoTrans, opB, -1.0, 1.0)),
        ("rocblas_batched", lambda: ops.gemm_batched_lib(
            C, pC, pA, pB, nb, nb, nb, nb, nb, nb, Op.NoTrans, opB, -1.0, 1.0)),
    ):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        dt_s = (time.perf_counter() - t0) / iters
        mul = 4 if dtype.is_complex else 1
        fl = 2.0 * nb**3 * ntc * mul
        print(f"trailing {tag} {dtype} nb={nb} tiles={ntc}: {dt_s*1e3:.2f} ms  "
              f"{fl/dt_s/1e12:.2f} TFLOP/s", flush=True)

def _median_ms(fn, reps=7, warm=2, before=None):
    import statistics
    ts = []
    for i in range(warm + reps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def _spd(n, nb, dtype):
    from dlaf_amd import Matrix
    from dlaf_amd.matrix import util as mutil
    mat = Matrix.create(n, n, nb, nb, dtype=dtype, device="cuda")
    mutil.set_random_hermitian_positive_definite(mat, seed=1)
    return mat


def bench_hemv(dtype=torch.float64, n=32768, nb=512, nrhs_list=(1, 2, 4, 8, 16, 32)):
    """hemv_tiles (y alone, and with |A||x|) against the read floor of the
    stored triangle, and against hermitian_multiplication on n x nrhs."""
    from dlaf_amd import (Matrix, Side, UpLo, HermitianVectorProduct,
                          hermitian_multiplication)
    from dlaf_amd.ops._ext import get_ext
    A = _spd(n, nb, dtype)
    esz = A.storage.element_size()
    nt = A.dist.nr_tiles[0]
    floor = n * (n + 1) / 2 * esz / 6.3e12 * 1e3
    work = get_ext().hemv_work_size(nt, nb) * 8
    hv = HermitianVectorProduct(UpLo.Lower, A, method="kernel")
    x = torch.randn(n, dtype=dtype, device="cuda")
    print(f"hemv {dtype} n={n} nb={nb}: triangle {n * (n + 1) / 2 * esz / 2**30:.2f} GiB, "
          f"read floor {floor:.3f} ms, workspace {work / 2**20:.1f} MiB", flush=True)
    for want_abs in (False, True):
        med, mn = _median_ms(lambda: hv.apply(x, want_abs=want_abs), reps=15)
        print(f"  hemv kernel abs={int(want_abs)}: median {med:.3f} ms  min {mn:.3f} ms  "
              f"{med / floor:.2f} x floor  {n * (n + 1) / 2 * esz / med / 1e6:.0f} GB/s",
              flush=True)
    for nrhs in nrhs_list:
        X = Matrix.create(n, nrhs, nb, nb, dtype=dtype, device="cuda")
        X.storage.normal_()
        Y = X.like()
        hemm, _ = _median_ms(lambda: hermitian_multiplication(
            Side.Left, UpLo.Lower, 1.0, A, X, 0.0, Y), reps=5, warm=1)
        cols, _ = _median_ms(lambda: [hv.apply(x) for _ in range(nrhs)], reps=5, warm=1)
        print(f"  nrhs={nrhs:3d}: hermitian_multiplication {hemm:9.3f} ms   "
              f"kernel per column {cols:9.3f} ms", flush=True)


def bench_mixed_solve(dtype=torch.float64, n=16384, nb=512, nrhs=4):
    """cholesky_solve_mixed against cholesky_factorization + cholesky_solve
    in the same precision as the input, and the two factorizations alone."""
    from dlaf_amd import (Matrix, UpLo, cholesky_factorization, cholesky_solve,
                          cholesky_solve_mixed)
    A = _spd(n, nb, dtype)
    B = Matrix.create(n, nrhs, nb, nb, dtype=dtype, device="cuda")
    B.set_from_global(torch.randn(n, nrhs, dtype=dtype, device="cuda"))
    low = torch.float32 if dtype == torch.float64 else torch.complex64
    out = {}

    def plain():
        L = A.clone()
        cholesky_factorization(UpLo.Lower, L)
        X = B.clone()
        cholesky_solve(UpLo.Lower, L, X)

    def mixed():
        out["r"] = cholesky_solve_mixed(UpLo.Lower, A, B)

    Ls = A.astype(low)
    keep_s, keep_d = Ls.storage.clone(), A.storage.clone()
    L = A.clone()
    f_lo, _ = _median_ms(lambda: cholesky_factorization(UpLo.Lower, Ls), reps=3, warm=1,
                         before=lambda: Ls.storage.copy_(keep_s))
    f_hi, _ = _median_ms(lambda: cholesky_factorization(UpLo.Lower, L), reps=3, warm=1,
                         before=lambda: L.storage.copy_(keep_d))
    del Ls, L, keep_s, keep_d
    t_plain, _ = _median_ms(plain, reps=3, warm=1)
    t_mixed, _ = _median_ms(mixed, reps=3, warm=1)
    print(f"mixed solve {dtype} n={n} nb={nb} nrhs={nrhs}: factorization {low} {f_lo:.1f} ms, "
          f"{dtype} {f_hi:.1f} ms ({f_hi / f_lo:.2f} x); potrf+potrs {t_plain:.1f} ms, "
          f"cholesky_solve_mixed {t_mixed:.1f} ms ({t_plain / t_mixed:.2f} x), "
          f"iters={out['r'][1]} info={out['r'][2]}", flush=True)


def bench_trsm_panel(dtype=torch.float64, nb=512, tiles=(1, 8, 31, 63)):
    """Solo time of the Cholesky panel solve X <- X L^-T at nb: the
    gemm_fused path (two launches per 64-column block) against the
    single-launch kernel at each strip height (0 = the kernel's own choice).
    Timed with events over ``inner`` back-to-back solves in place; L is scaled
    to singular values around 1 so that X stays in range."""
    a = torch.randn(nb, nb, dtype=dtype, device="cuda")
    L = a @ a.mH + nb * torch.eye(nb, dtype=dtype, device="cuda")
    dinv = ops.potrf_tile(L)
    L = torch.tril(L) / (2 * nb) ** 0.5   # singular values around 1
    dinv = dinv * 0
    bsz = dinv.shape[-1]
    for d in range((nb + bsz - 1) // bsz):
        c0 = d * bsz
        ops.get_ext().trtri_lower(L[c0:, c0:], dinv[d], min(bsz, nb - c0),
                                  L.stride(0), bsz, False)
    inner = 10
    for nt in tiles:
        x = torch.randn(nt, nb, nb, dtype=dtype, device="cuda")
        offs = [i * nb * nb for i in range(nt)]
        doffs = torch.tensor(offs, device="cuda")
        fl = nt * nb ** 3 * (2 if dtype.is_complex else 1) * inner

        def timed(fn):
            for _ in range(2):
                fn()
            ts = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            return sorted(ts)[len(ts) // 2]

        ms = timed(lambda: ops.trsm_panel_right_lowerH(x, offs, L, dinv, nb, nb, nb, fused=False))
        line = f"trsm_panel {dtype} nb={nb} tiles={nt}: gemm_fused {ms / inner * 1e3:.0f} us"
        if ops.has_trsm_panel_fused(dtype):
            for strip in (0, 16, 32):
                ms = timed(lambda: ops.trsm_panel_fused(x, doffs, L, dinv, nb, nb, nb, strip=strip))
                line += f" | strip {strip}: {ms / inner * 1e3:.0f} us ({fl / ms / 1e9:.1f} TF/s)"
        print(line, flush=True)


def _shape_args(flag, n, nb):
    rest = sys.argv[sys.argv.index(flag) + 1:]
    nums = []
    for a in rest:
        if not a.isdigit():
            break
        nums.append(int(a))
    return (nums + [n, nb][len(nums):])[:2]


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    if "--trsm" in sys.argv:
        bench_trsm_panel(torch.float64)
        bench_trsm_panel(torch.float32)
        sys.exit(0)
    if "--hemv" in sys.argv or "--mixed" in sys.argv:
        if "--hemv" in sys.argv:
            n, nb = _shape_args("--hemv", 32768, 512)
            bench_hemv(torch.float64, n, nb)
            bench_hemv(torch.complex128, n // 2, nb)
        if "--mixed" in sys.argv:
            n, nb = _shape_args("--mixed", 16384, 512)
            bench_mixed_solve(torch.float64, n, nb, nrhs=4)    # vector kernels
            bench_mixed_solve(torch.float64, n, nb, nrhs=64)   # tiled HEMM / TRSM
        sys.exit(0)
    bench_gemm(torch.float64, 512, 128)
    bench_gemm(torch.float64, 512, 1024, iters=5)
    bench_gemm(torch.float32, 512, 128)
    bench_gemm(torch.complex128, 512, 64)
    bench_torch_bmm(torch.float64, 512, 128)
    bench_torch_bmm(torch.float64, 512, 1024, iters=5)
    if "--lib" in sys.argv:
        bench_lib_batched(torch.float64)
        bench_lib_batched(torch.complex128, nt=44)
    bench_big_dgemm(torch.float64, 16384)
    bench_potrf(torch.float64)
    bench_potrf(torch.complex128, 512)
    bench_trtri(torch.float64)
