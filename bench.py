#!/usr/bin/env python3
"""Flagship benchmark: fp64 tiled Cholesky (POTRF), N=32768, nb=512.

BASELINE.json config 2 ("fp64 Cholesky (POTRF) N=32768 nb=512 on 1 MI355X") and
its multi-GPU strong-scaling variants (grid 1x2 / 2x2 / 2x4 over RCCL/xGMI).
Metric: GFlop/s with the reference's flop count n^3/3 (n^3/6 mul + n^3/6 add,
``miniapp/miniapp_cholesky.cpp:157-163``; complex weights would be 2/6).

One step = restore the matrix from a device-resident pristine copy (D2D,
~1-2%% of step time, included in the timing) + full in-place factorization.
Protocol: W untimed warmup steps, then exactly K timed steps bracketed by a
barrier + torch.cuda.synchronize on both sides; elapsed time is the MAX over
ranks; rank 0 prints one JSON line.

A plain run does only that. ``--full`` adds the driver-timed single-GPU extras
(TRSM N=32768, SYEV N=20000, ZHEGV N=16384; ``config.extra_configs``).
``--dump-outputs DIR`` writes the factor left by the last timed step as
``DIR/<name>.npy`` (float64) so two builds can be compared output for output.
"""

import argparse
import json
import os
import time

import torch


def _rccl_dry_run(grid, device, rank):
    """Validate collective creation/order on every grid group before the
    timed loop (round-1 verdict item 4a): one small all-reduce on full/row/
    col groups in a fixed order, then a broadcast, with value checks."""
    import torch.distributed as dist
    dev = device if device.type == "cuda" else torch.device("cpu")
    t = torch.ones(8, dtype=torch.float64, device=dev)
    dist.all_reduce(t, group=grid.full_group)
    assert float(t[0].item()) == grid.world_size, "full-group all-reduce"
    for g, size in ((grid.row_group, grid.grid_cols),
                    (grid.col_group, grid.grid_rows)):
        if g is None:
            continue
        t2 = torch.ones(8, dtype=torch.float64, device=dev)
        dist.all_reduce(t2, group=g)
        assert float(t2[0].item()) == size, "sub-group all-reduce"
    b = torch.full((4,), float(rank == 0), dtype=torch.float64, device=dev)
    dist.broadcast(b, src=0, group=grid.full_group)
    assert float(b[0].item()) == 1.0, "broadcast from rank 0"
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def _extra_configs(device):
    """Driver-timed single-GPU measurements of BASELINE configs 3' (TRSM
    N=32768), 4 (SYEV N=20000) and 5 (ZHEGV N=16384); one warmup-free or
    single-warmup run each, barrier-bracketed like the headline."""
    import torch

    from dlaf_amd import (Matrix, Side, UpLo, Op, Diag, triangular_solver,
                          hermitian_eigensolver,
                          hermitian_generalized_eigensolver)
    from dlaf_amd.matrix import util as mutil

    out = {}

    def timed(fn, warm=1):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0

    # config 3 shape on one GPU: fp64 TRSM Left-Lower-N N=32768 nb=512
    n, nb = 32768, 512
    a = Matrix.create(n, n, nb, nb, dtype=torch.float64, device=device)
    mutil.set_random_hermitian_positive_definite(a, seed=3)
    b = Matrix.create(n, n, nb, nb, dtype=torch.float64, device=device)
    mutil.set_random(b, seed=4)
    b0 = b.storage.clone()

    def trsm():
        b.storage.copy_(b0)
        triangular_solver(Side.Left, UpLo.Lower, Op.NoTrans, Diag.NonUnit,
                          1.0, a, b)

    t = timed(trsm)
    out["trsm_fp64_n32768_nb512_1gpu"] = {
        "time_s": t, "gflops": (n * n * n) / t / 1e9}
    del a, b, b0
    torch.cuda.empty_cache()

    # config 4 on one GPU: fp64 SYEV N=20000
    n = 20000
    a = Matrix.create(n, n, nb, nb, dtype=torch.float64, device=device)
    mutil.set_random_hermitian(a, seed=5)
    a0 = a.storage.clone()

    def syev():
        a.storage.copy_(a0)
        hermitian_eigensolver(UpLo.Lower, a)

    out["syev_fp64_n20000_nb512_1gpu"] = {"time_s": timed(syev)}
    del a, a0
    torch.cuda.empty_cache()

    # config 5 on one GPU: complex128 ZHEGV N=16384
    n = 16384
    a = Matrix.create(n, n, nb, nb, dtype=torch.complex128, device=device)
    mutil.set_random_hermitian(a, seed=6)
    bm = Matrix.create(n, n, nb, nb, dtype=torch.complex128, device=device)
    mutil.set_random_hermitian_positive_definite(bm, seed=7)
    a0 = a.storage.clone()
    bm0 = bm.storage.clone()

    def zhegv():
        a.storage.copy_(a0)
        bm.storage.copy_(bm0)
        hermitian_generalized_eigensolver(UpLo.Lower, a, bm)

    out["zhegv_c128_n16384_nb512_1gpu"] = {"time_s": timed(zhegv)}
    del a, bm, a0, bm0
    torch.cuda.empty_cache()
    return out


_DUMP_FULL_MAX_BYTES = 32 << 20   # dump the whole factor up to this size
_DUMP_SAMPLES = 2 << 20           # seeded lower-triangle samples beyond it
_DUMP_TAIL_ROWS = 64              # trailing rows (depend on every panel)


def _dump_outputs(out_dir, mat, rank):
    """Write what the last timed step left in ``mat`` (the lower Cholesky
    factor, as a caller of cholesky_factorization receives it) as float64
    ``.npy`` files. Small factors are written whole (``L.npy``); large ones
    as the diagonal, the last rows and a fixed seeded sample of the lower
    triangle (~33 MB in all). Collective on a distributed grid."""
    import numpy as np

    d = mat.dist
    n, nb = d.n, d.nb
    distributed = mat.grid is not None and mat.grid.distributed
    glob = mat.to_global() if distributed or n * n * 8 <= _DUMP_FULL_MAX_BYTES else None

    def gather(rows, cols):
        r = torch.as_tensor(rows, device=mat.storage.device)
        c = torch.as_tensor(cols, device=mat.storage.device)
        if glob is not None:
            v = glob[r, c]
        else:
            v = mat.storage[r // nb, c // nb, r % nb, c % nb]
        return v.to(torch.float64).cpu().numpy()

    arrays = {}
    if n * n * 8 <= _DUMP_FULL_MAX_BYTES:
        arrays["L"] = torch.tril(glob).to(torch.float64).cpu().numpy()
    else:
        idx = np.arange(n, dtype=np.int64)
        arrays["L_diag"] = gather(idx, idx)
        tail = np.arange(n - _DUMP_TAIL_ROWS, n, dtype=np.int64)
        rr, cc = np.meshgrid(tail, idx, indexing="ij")
        arrays["L_tail_rows"] = np.where(cc <= rr, gather(rr, cc), 0.0)
        rng = np.random.RandomState(20240607)
        a = rng.randint(0, n, size=_DUMP_SAMPLES).astype(np.int64)
        b = rng.randint(0, n, size=_DUMP_SAMPLES).astype(np.int64)
        arrays["L_sample"] = gather(np.maximum(a, b), np.minimum(a, b))
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        for name, arr in arrays.items():
            np.save(os.path.join(out_dir, name + ".npy"), arr)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--n", type=int, default=32768)
    p.add_argument("--nb", type=int, default=512)
    p.add_argument("--device", type=str, default=None, help="debug override (cpu)")
    p.add_argument("--full", action="store_true",
                   help="also time the single-GPU extra configs (TRSM/SYEV/ZHEGV)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="write the last timed step's factor as DIR/<name>.npy")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")

    import torch.distributed as dist

    from dlaf_amd import Matrix, CommGrid, UpLo, cholesky_factorization
    from dlaf_amd.matrix import util as mutil

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    if args.device == "cpu":
        device = torch.device("cpu")
    else:
        assert torch.cuda.is_available(), "bench needs a GPU (or --device cpu)"
        device = torch.device(f"cuda:{local_rank}")
        torch.cuda.set_device(device)

    if world_size > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = "nccl" if device.type == "cuda" else "gloo"
        dist.init_process_group(backend, rank=rank, world_size=world_size)

    grids = {1: (1, 1), 2: (1, 2), 4: (2, 2), 8: (2, 4)}
    gr, gc = grids.get(world_size, (1, world_size))
    grid = CommGrid(gr, gc, device=device)

    if world_size > 1:
        _rccl_dry_run(grid, device, rank)

    # env overrides (torchrun's argparse eats abbreviated --n/--nb)
    n = int(os.environ.get("DLAF_BENCH_N", args.n))
    nb = int(os.environ.get("DLAF_BENCH_NB", args.nb))
    mat = Matrix.create(n, n, nb, nb, dtype=torch.float64, device=device, grid=grid)
    mutil.set_random_hermitian_positive_definite(mat, seed=42)
    pristine = mat.storage.clone()

    def barrier_sync():
        if world_size > 1:
            dist.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    def step():
        mat.storage.copy_(pristine)
        cholesky_factorization(UpLo.Lower, mat, grid)

    for _ in range(args.warmup):
        step()
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier_sync()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if world_size > 1:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if device.type == "cuda" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    ms_per_step = elapsed / args.steps * 1000.0
    flops = n ** 3 / 3.0  # fp64 POTRF: n^3/6 mul + n^3/6 add
    gflops = flops / (elapsed / args.steps) / 1e9

    if args.dump_outputs:
        _dump_outputs(args.dump_outputs, mat, rank)

    # Extra BASELINE configs (3', 4, 5), behind --full: measured in the same
    # invocation on a single GPU so a full run carries driver-timed values
    # for more than the headline config. Each block has its own warmup and
    # barrier-bracketed timed region; results ride in config.extra_configs.
    extra = {}
    if (args.full and world_size == 1 and device.type == "cuda" and n == 32768
            and os.environ.get("DLAF_BENCH_EXTRA", "1") != "0"):
        extra = _extra_configs(device)

    if rank == 0:
        print(json.dumps({
            "metric": "cholesky_fp64_gflops",
            "value": gflops,
            "unit": "GFlop/s",
            "n_gpus": world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "fp64",
            "data": "synthetic random SPD (diagonally dominant), restore included in step",
            "config": {
                "model": "fp64 Cholesky (POTRF)",
                "n": n,
                "nb": nb,
                "parallelism": f"grid{gr}x{gc}",
                "global_batch": 1,
                "seq_len": n,
                "extra_configs": extra,
            },
        }))

    if world_size > 1:
        # drain before teardown: destroying while a peer is still inside its
        # last collective is a known gloo/nccl shutdown race (same fix as
        # tests/dist_utils.py)
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
