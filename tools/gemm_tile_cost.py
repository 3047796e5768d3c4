"""Where the numbers of TILE_COST (csrc/gemm.hip, the cost table of plan_tiles) come from: microseconds per 64-deep K-step and per
tile of each tile configuration of the DMA GEMM engine, for a block that is alone on its CU and for one that shares it.

Each configuration is forced (knob GEMM_CFG) on linear problems of exactly `ncu` tiles (one block per CU, one tile each), 2 ncu
tiles (two blocks per CU) and 4 ncu tiles (two blocks per CU, two tiles each) - for the large configurations ncu and 2 ncu tiles
(one block per CU, one and two tiles) - at K = 1152 and K = 2304.  The slope over K of the 2 ncu-tile problems is the K-step of a block that shares
its CU; what a block's second tile adds beyond its K-steps is the per-tile cost; what remains of a one-tile launch is the launch; the
K-step of a block alone on its CU follows from the long ncu-tile problem.  (The 4 ncu-tile problem at K = 2304 is printed for
reference only: its operands no longer fit the Infinity Cache, which the tails the table prices always do.)

    python tools/gemm_tile_cost.py [--iters 20] [--rounds 5]
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viewcrafter_amd import ops  # noqa: E402
from viewcrafter_amd.packing import pack_geglu  # noqa: E402

CFGS = {0: (128, 128, 2), 1: (128, 160, 2), 2: (256, 256, 1), 3: (256, 320, 1), 4: (64, 128, 2), 5: (64, 64, 2), 6: (64, 128, 2)}
K1, K2 = 1152, 2304      # both long enough that the launch rate of the host does not show


def _time(fn, iters):
    fn(); fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3      # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# {torch.cuda.get_device_name(0)}, {ncu} CUs; us per launch, min over {args.rounds} rounds of {args.iters} back-to-back launches")
    print(f"{'cfg':>3} {'tile':>9} {'tiles':>6} {'M':>7} {'N':>5} {'K':>5} {'us':>8}")
    table = {}
    for cfg, (tbm, tbn, bpc) in CFGS.items():
        geglu = cfg == 6
        tiles_n = 2
        N = tbn * tiles_n
        t = {}
        for mult in ((1, 2, 4) if bpc == 2 else (1, 2)):
            M = tbm * ncu * mult // tiles_n
            for K in (K1, K2):
                x = (torch.randn(M, K, device="cuda")).half()
                if geglu:
                    w, b = pack_geglu(torch.randn(N, K, device="cuda") / math.sqrt(K), torch.randn(N, device="cuda"))
                    w = w.half()
                else:
                    w = (torch.randn(N, K, device="cuda") / math.sqrt(K)).half()
                    b = torch.randn(N, device="cuda")
                out = torch.empty(M, N // 2 if geglu else N, dtype=torch.float16, device="cuda")
                prev = ops.tune_set("GEMM_CFG", cfg)
                try:
                    us = min(_time(lambda: ops.linear(x, w, b, geglu=geglu, out=out), args.iters) for _ in range(args.rounds))
                finally:
                    ops.tune_set("GEMM_CFG", prev)
                t[(mult, K)] = us
                print(f"{cfg:3d} {tbm:4d}x{tbn:<4d} {ncu * mult:6d} {M:7d} {N:5d} {K:5d} {us:8.2f}")
        nk1, nk2, dk = K1 // 64, K2 // 64, (K2 - K1) // 64
        if bpc == 2:
            k_share = (t[(2, K2)] - t[(2, K1)]) / dk                  # two blocks per CU, one tile each; both problems sit in the Infinity Cache
            e = (t[(4, K1)] - t[(2, K1)]) - nk1 * k_share           # what a block's second tile adds beyond its K-steps
            launch = t[(2, K1)] - nk1 * k_share - e
            k_alone = (t[(1, K2)] - launch - e) / nk2                 # from the long problem alone: the short one of a 64-row configuration runs at the host's launch rate
        else:
            k_alone = k_share = (t[(1, K2)] - t[(1, K1)]) / dk
            e = (t[(2, K1)] - t[(1, K1)]) - nk1 * k_alone
            launch = t[(1, K1)] - nk1 * k_alone - e
        table[cfg] = (tbm, tbn, bpc, k_alone, k_share, e, launch)
    print("# TILE_COST rows: {tbm, tbn, blocks/CU, k_alone, k_share, e}   (launch: what a launch costs beyond its tiles)")
    for cfg, (tbm, tbn, bpc, ka, ks, e, la) in table.items():
        print(f"    {{{tbm}, {tbn}, {bpc}, {ka:.2f}f, {ks:.2f}f, {e:.1f}f}},   // cfg {cfg}; launch {la:.1f}")


if __name__ == "__main__":
    main()
