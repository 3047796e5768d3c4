"""Per-shape A/B of the feed-forward pair, MXFP8 (VCX_FF_MXFP8 route) against fp16 (the default route), isolated, with clock / power
telemetry beside every figure (tools/telemetry.py).  Writes the table of profiles/mxfp8_ff.md to stdout.

    python tools/mxfp8_ff_ab.py [--rows-scale 1.0] [--rounds 3]

Per level (dim 320 / 640 / 1280 at the config-1 row counts 460800 / 115200 / 28800): the LayerNorm + GEGLU projection and the output
projection of both routes, each timed alone, interleaved rounds, median.  fp16: layer_norm (or row_stats where the fold is on) + GEGLU
GEMM, then ff.2 with residual.  MX: layer_norm_mxfp8 + GEGLU GEMM with MXFP8 out, then ff.2 reading those bytes."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.telemetry import Telemetry  # noqa: E402
from viewcrafter_amd import ops  # noqa: E402
from viewcrafter_amd.packing import fold_layernorm, pack_geglu, pack_mxfp8  # noqa: E402

DEV = "cuda"
LEVELS = [(460800, 320), (115200, 640), (28800, 1280)]


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def level(rows, dim, fold):
    g = torch.Generator(device=DEV).manual_seed(dim)
    rn = lambda *s, sc=1.0: torch.randn(*s, device=DEV, generator=g) * sc
    t = (rn(rows, dim) * 1.5).half()
    gamma, beta = 1 + 0.2 * rn(dim), 0.1 * rn(dim)
    w1, b1 = rn(8 * dim, dim, sc=dim ** -0.5), rn(8 * dim)
    w2, b2 = rn(dim, 4 * dim, sc=(4 * dim) ** -0.5).half(), rn(dim)
    w1p, b1p = pack_geglu(w1.half(), b1)
    wf, cs, bf = fold_layernorm(w1, gamma, beta, b1)
    wfp, bfp = pack_geglu(wf, bf)
    csp = pack_geglu(wf, cs)[1]
    mx1, mx2 = pack_mxfp8(w1p), pack_mxfp8(w2)
    state = {}

    def f16_ff1():
        if fold:
            state["g"] = ops.linear(t, wfp, bfp, geglu=True, ln_stats=ops.row_stats(t, 1e-5), ln_colsum=csp)
        else:
            state["g"] = ops.linear(ops.layer_norm(t, gamma, beta, 1e-5), w1p, b1p, geglu=True)

    def f16_ff2():
        ops.linear(state["g"], w2, b2, residual=t)

    def mx_ff1():
        state["q"] = ops.linear_mxfp8(ops.layer_norm_mxfp8(t, gamma, beta, 1e-5), mx1, b1p, K=dim, geglu=True, mx_out=True)

    def mx_ff2():
        ops.linear_mxfp8(state["q"], mx2, b2, K=4 * dim, residual=t)

    def mx_ln():
        ops.layer_norm_mxfp8(t, gamma, beta, 1e-5)

    return dict(f16_ff1=f16_ff1, f16_ff2=f16_ff2, mx_ff1=mx_ff1, mx_ff2=mx_ff2, mx_ln=mx_ln)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    ops.require_gpu()
    out = []
    for rows, dim in LEVELS:
        rows = max(64, int(rows * a.rows_scale))
        fns = level(rows, dim, fold=dim >= 640)
        samples = {k: [] for k in fns}
        with Telemetry(device_index=0, period_s=0.05) as tm:
            for _ in range(a.rounds):
                for k in ("f16_ff1", "f16_ff2", "mx_ff1", "mx_ff2", "mx_ln"):
                    samples[k].append(timed(fns[k], a.iters))
        med = {k: statistics.median(v) for k, v in samples.items()}
        fl1, fl2 = 2.0 * rows * 8 * dim * dim, 2.0 * rows * dim * 4 * dim
        tel = tm.summary()
        row = dict(rows=rows, dim=dim, ms=med, tflops=dict(f16_ff1=fl1 / med["f16_ff1"] / 1e9, mx_ff1=fl1 / med["mx_ff1"] / 1e9,
                                                            f16_ff2=fl2 / med["f16_ff2"] / 1e9, mx_ff2=fl2 / med["mx_ff2"] / 1e9), telemetry=tel)
        out.append(row)
        sclk, pw = (tel.get("sclk_mhz") or {}).get("mean"), (tel.get("power_w") or {}).get("mean")
        print(f"| {rows} x {dim} | LN + GEGLU {rows}x{8 * dim}x{dim} | {med['f16_ff1']:.3f} | {med['mx_ff1']:.3f} (LN+quant alone {med['mx_ln']:.3f}) | "
              f"{med['f16_ff1'] / med['mx_ff1']:.2f}x | {sclk and round(sclk)} MHz / {pw and round(pw)} W |")
        print(f"| {rows} x {dim} | ff.2 {rows}x{dim}x{4 * dim} + residual | {med['f16_ff2']:.3f} | {med['mx_ff2']:.3f} | {med['f16_ff2'] / med['mx_ff2']:.2f}x | |")
        sys.stdout.flush()
        del fns
        torch.cuda.empty_cache()
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
