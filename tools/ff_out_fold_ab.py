"""Isolated A/B of the transformers' last two linear layers at the benchmark's rows (B = 2, 25 x 72 x 128 latent), per UNet level:

    pair    ff.net[2] (+ block residual), then proj_out (+ transformer residual)            - two launches, as under VCX_FF_OUT_FOLD=0
    merged  one GEMM over [g ; t] with the K tail in linear mode                            - ops.linear(g, wcat, bcat, tail=[t], ...)
    conv1   the same GEMM as a 1x1 convolution with a K tail through the gather kernel      - the form that existed before (comparison only)

each with and without proj_out's column moments.  One process, legs interleaved round by round, HIP events around `--iters` back-to-back
calls, the mean graphics clock (tools/telemetry.py) beside every leg.  Prints a table and, with --json, one JSON document.

    python tools/ff_out_fold_ab.py [--rounds 5] [--iters 10] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEVELS = [(0, 460800, 320), (1, 115200, 640), (2, 28800, 1280)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from telemetry import Telemetry
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_ff_out_folded
    ops.require_gpu()
    dev = "cuda"

    def rh(*s, sc=1.0):
        return (torch.randn(*s, device=dev) * sc).half()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with Telemetry(device_index=0, period_s=0.02) as tm:
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
        clk = (tm.summary().get("sclk_mhz") or {}).get("mean")
        return a.elapsed_time(b) / args.iters, clk

    doc = []
    for level, M, D in LEVELS:
        g, t, xin = rh(M, 4 * D), rh(M, D), rh(M, D)
        w2, b2 = rh(D, 4 * D, sc=(4 * D) ** -0.5), torch.randn(D, device=dev) * 0.1
        wout, bout = rh(D, D, sc=D ** -0.5), torch.randn(D, device=dev) * 0.1
        wcat, bcat = pack_ff_out_folded(w2, b2, wout, bout)
        cs = ops.colstats_buffer(M, D, dev)
        gimg = g.view(1, 1, M, 4 * D)
        for with_cs in (False, True):
            kw = dict(colstats=cs) if with_cs else {}
            assert ops.linear_tail_ok(M, D, 4 * D, [D], residual=True, colstats=with_cs)
            legs = {
                "ff2": lambda: ops.linear(g, w2, b2, residual=t),
                "proj_out": lambda: ops.linear(t, wout, bout, residual=xin, **kw),
                "pair": lambda: ops.linear(ops.linear(g, w2, b2, residual=t), wout, bout, residual=xin, **kw),
                "merged": lambda: ops.linear(g, wcat, bcat, tail=[t], residual=xin, **kw),
                "conv1": lambda: ops.conv2d(gimg, wcat, bcat, kh=1, kw=1, tail=[t], residual=xin, **kw),
            }
            assert torch.equal(legs["merged"](), legs["conv1"]().view(M, D)), "the linear and the convolution form of the tailed GEMM differ"
            times = {k: [] for k in legs}
            clocks = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    ms, clk = timed(fn)
                    times[k].append(ms)
                    clocks[k].append(clk)
            row = dict(level=level, M=M, D=D, colstats=with_cs)
            print(f"level {level} M={M} D={D} colstats={with_cs}")
            for k in legs:
                v = sorted(times[k])
                c = [x for x in clocks[k] if x]
                row[k] = dict(median_ms=v[len(v) // 2], min_ms=v[0], max_ms=v[-1], sclk_mhz=(sum(c) / len(c)) if c else None)
                print(f"    {k:9s} median {row[k]['median_ms']:.4f} ms  min {v[0]:.4f}  max {v[-1]:.4f}  spread {v[-1] - v[0]:.4f}  sclk {row[k]['sclk_mhz']}")
            doc.append(row)
        del g, t, xin, cs, gimg
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
