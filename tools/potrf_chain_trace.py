#!/usr/bin/env python3
"""Per-step breakdown of the Cholesky lookahead chain from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- \\
        python bench.py --steps 2 --warmup 1
    python tools/potrf_chain_trace.py DIR/NAME_kernel_trace.csv [nt] [nblocks]

Takes the LAST factorization in the trace (nt steps; default 64 for N=32768,
nb=512), finds for each step k the kernels of ``potrf_tile`` (everything from
the first diagonal-block kernel of the step to its last), the panel-TRSM
launches behind them, the head update and the tail update, and prints their
kernel time, the idle time between the chain's launches, and the three
regimes of the issue: early (k < 16), middle, late (k >= 32). Times in us.
"""

import csv
import sys
from collections import defaultdict


def main():
    path = sys.argv[1]
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    nblocks = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                         r["Kernel_Name"], int(r["Grid_Size_X"]), r.get("Queue_Id", "")))
    rows.sort()
    # diagonal-block kernels: the stand-alone factor+invert launch opens a tile
    is_block = lambda n: "potrf_invert_block_k" in n
    is_step = lambda n: "potrf_step_k" in n
    is_gemm = lambda n: "gemm_v2_k" in n or "gemm_tiles_k" in n
    # the single-launch panel solve (csrc/trsm_panel.hip); builds without it
    # solve the panel with gemm_tiles_k launches
    is_trsm = lambda n: "trsm_panel_k" in n
    fused = any(is_step(r[2]) for r in rows)
    # index of the kernel that opens each potrf_tile
    opens = []
    seen_in_tile = 0
    for i, r in enumerate(rows):
        if is_block(r[2]):
            if fused or seen_in_tile % nblocks == 0:
                opens.append(i)
            seen_in_tile += 1
    opens = opens[-nt:]
    assert len(opens) == nt, f"found {len(opens)} tile factorizations, wanted {nt}"
    per_step = []
    for k, i0 in enumerate(opens):
        i1 = opens[k + 1] if k + 1 < nt else len(rows)
        seg = rows[i0:i1]
        q = seg[0][4]
        chain = [r for r in seg if r[4] == q and (is_block(r[2]) or is_step(r[2])
                                                  or is_gemm(r[2]) or is_trsm(r[2]))]
        # potrf_tile = up to the last diagonal-block / step kernel (parent build:
        # plus the small GEMMs between them)
        last_diag = max(j for j, r in enumerate(chain) if is_block(r[2]) or is_step(r[2]))
        tile = chain[:last_diag + 1]
        rest = chain[last_diag + 1:]
        nrem = nt - 1 - k
        # program order on the chain's stream: TRSM launches, then the head update
        head = rest[-1:] if nrem > 0 else []
        trsm = rest[:-1] if nrem > 0 else rest
        tail = [r for r in seg if r[4] != q and is_gemm(r[2])]
        dur = lambda rs: sum(e - s for s, e, *_ in rs) / 1e3
        def gaps(rs):
            return sum(max(0, rs[j + 1][0] - rs[j][1]) for j in range(len(rs) - 1)) / 1e3
        t_block = dur([r for r in tile if is_block(r[2]) or is_step(r[2])])
        t_small = dur([r for r in tile if is_gemm(r[2])])
        span = (chain[-1][1] - chain[0][0]) / 1e3 if chain else 0.0
        per_step.append(dict(
            k=k, launches=len(tile), block=t_block, small=t_small, tile_gaps=gaps(tile),
            tile_span=(tile[-1][1] - tile[0][0]) / 1e3, ntrsm=len(trsm), trsm=dur(trsm),
            trsm_span=((trsm[-1][1] - trsm[0][0]) / 1e3 if trsm else 0.0),
            head=dur(head), tail=dur(tail), chain_span=span,
            step=((rows[i1][0] if i1 < len(rows) else seg[-1][1]) - seg[0][0]) / 1e3))
    cols = ["launches", "block", "small", "tile_gaps", "tile_span", "ntrsm", "trsm",
            "trsm_span", "head", "tail", "chain_span", "step"]
    print("potrf_tile launches per tile:", sorted(set(p["launches"] for p in per_step)))
    print("| regime | " + " | ".join(cols) + " |")
    print("|---|" + "---|" * len(cols))
    regimes = [("early k<16", range(0, 16)), ("middle 16<=k<32", range(16, 32)),
               ("late k>=32", range(32, nt)), ("all", range(0, nt))]
    for name, ks in regimes:
        sel = [p for p in per_step if p["k"] in ks]
        tot = defaultdict(float)
        for p in sel:
            for c in cols:
                tot[c] += p[c]
        cells = []
        for c in cols:
            if c in ("launches", "ntrsm"):
                cells.append(f"{tot[c] / len(sel):.0f}")
            else:
                cells.append(f"{tot[c] / 1e3:.2f} ms")
        print(f"| {name} | " + " | ".join(cells) + " |")
    total = (rows[-1][1] - rows[opens[0]][0]) / 1e6
    print(f"last factorization, first potrf kernel to last kernel: {total:.1f} ms")


if __name__ == "__main__":
    main()
