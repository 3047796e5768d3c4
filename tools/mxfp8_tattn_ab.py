"""Per-width A/B of one temporal attention layer (LayerNorm -> q|k|v -> attention over T -> to_out + residual), MXFP8 (VCX_TATTN_MXFP8
route) against fp16 (the default route), isolated, with clock / power telemetry beside every figure (tools/telemetry.py).  Writes the table
of profiles/mxfp8_tattn.md to stdout.

    python tools/mxfp8_tattn_ab.py [--rows-scale 1.0] [--rounds 5] [--iters 20]

Per level (width 320 / 640 / 1280 at the row counts of 576x1024x25: B = 2 videos x T = 25 frames x P = 9216 / 2304 / 576 pixels): the
whole layer on either route, and its parts timed apart - the pass in front of q|k|v (row statistics for the folded fp16 projection, the
quantising LayerNorm for MX), the q|k|v projection, the attention kernel, to_out.  The fp16 layer is timed in two forms: with the row
statistics handed in (in the model the GEMM that writes the token stream supplies them where ops.rowstats_ok holds - the form that is
kindest to fp16, and the one the skip rule compares against) and with its own statistics pass.  Every variant is warmed up, rounds are
interleaved (fp16 - MX - fp16 again: the two fp16 series give the fp16 route's own spread on this box), median over the rounds."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.telemetry import Telemetry  # noqa: E402
from viewcrafter_amd import ops  # noqa: E402
from viewcrafter_amd.lvdm.modules import attention as A  # noqa: E402

DEV = "cuda"
B, T = 2, 25
LEVELS = [(9216, 320), (2304, 640), (576, 1280)]


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


def level(P, D):
    torch.manual_seed(D)
    heads = D // 64
    tr = A.TemporalTransformer(D, heads, 64).eval()
    with torch.no_grad():
        for m in tr.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.2 * torch.randn(D))
                m.bias.copy_(0.1 * torch.randn(D))
    tr = tr.to(DEV)
    blk = tr.transformer_blocks[0]
    attn, lnp = blk.attn1, blk.ln_params()[0]
    ap, am = attn.packed(), attn.mx_packed()
    tokens = B * T * P
    g = torch.Generator(device=DEV).manual_seed(D)
    t = (torch.randn(tokens, D, device=DEV, generator=g) * 1.3).half()
    geo = dict(B=B, T=T, P=P, heads=heads, ld=3 * D, k_off=D, v_off=2 * D, scale=attn.scale)
    if not A._folded(ap["qkv"], tokens, D, D):
        print(f"(width {D}: the fp16 q|k|v projection is not folded at this shape - its rows include a LayerNorm pass)")
    assert ops.linear_mxfp8_ok(tokens, 3 * D, D) and ops.linear_mxfp8_ok(tokens, D, D, residual=True) and ops.temporal_attn_mxfp8_ok(B, T, P, heads, 3 * D)
    st = ops.row_stats(t, lnp[2])
    o16 = torch.empty((tokens, D), dtype=torch.float16, device=DEV)
    state = dict(qkv=A.ln_linear(t, ap["qkv"], lnp, stats=st), a=ops.layer_norm_mxfp8(t, *lnp))
    state["omx"] = ops.temporal_attn_mxfp8(state["qkv"], **geo)
    ops.temporal_attn(state["qkv"], o16, ldo=D, **geo)

    def f16_layer(stats):
        def run():
            qkv = A.ln_linear(t, ap["qkv"], lnp, stats=stats)
            ops.temporal_attn(qkv, o16, ldo=D, **geo)
            ops.linear(o16, ap["wo"], ap["bo"], residual=t)
        return run

    def mx_layer():
        a = ops.layer_norm_mxfp8(t, *lnp)
        qkv = ops.linear_mxfp8(a, am["wqkv"], am["zero"], K=D)
        o = ops.temporal_attn_mxfp8(qkv, **geo)
        ops.linear_mxfp8(o, am["wo"], am["bo"], K=D, residual=t)

    return dict(f16_layer=f16_layer(st), mx_layer=mx_layer, f16_layer_again=f16_layer(st), f16_layer_own_stats=f16_layer(None),
                f16_pre=lambda: ops.row_stats(t, lnp[2]), mx_pre=lambda: ops.layer_norm_mxfp8(t, *lnp),
                f16_qkv=lambda: A.ln_linear(t, ap["qkv"], lnp, stats=st), mx_qkv=lambda: ops.linear_mxfp8(state["a"], am["wqkv"], am["zero"], K=D),
                f16_attn=lambda: ops.temporal_attn(state["qkv"], o16, ldo=D, **geo), mx_attn=lambda: ops.temporal_attn_mxfp8(state["qkv"], **geo),
                f16_out=lambda: ops.linear(o16, ap["wo"], ap["bo"], residual=t), mx_out=lambda: ops.linear_mxfp8(state["omx"], am["wo"], am["bo"], K=D, residual=t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-scale", type=float, default=1.0, help="scales P (rounded to a multiple of 64)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    ops.require_gpu()
    out = []
    order = ("f16_layer", "mx_layer", "f16_layer_again", "f16_layer_own_stats", "f16_pre", "mx_pre", "f16_qkv", "mx_qkv", "f16_attn", "mx_attn", "f16_out", "mx_out")
    print("| width | rows | what | fp16 ms | MXFP8 ms | fp16 / MXFP8 | clock / power |")
    print("|---|---|---|---|---|---|---|")
    for P, D in LEVELS:
        P = max(64, int(P * a.rows_scale) // 64 * 64)
        with torch.no_grad():
            fns = level(P, D)
            for k in order:                        # every shape of the timed window, warmed up
                timed(fns[k], 2)
            samples = {k: [] for k in fns}
            with Telemetry(device_index=0, period_s=0.05) as tm:
                for _ in range(a.rounds):
                    for k in order:
                        samples[k].append(timed(fns[k], a.iters))
        med = {k: statistics.median(v) for k, v in samples.items()}
        rows = B * T * P
        fl_qkv, fl_out = 2.0 * rows * D * 3 * D, 2.0 * rows * D * D
        tel = tm.summary()
        spread = abs(med["f16_layer"] - med["f16_layer_again"]) / min(med["f16_layer"], med["f16_layer_again"])
        f16 = max(med["f16_layer"], med["f16_layer_again"])
        gain = min(med["f16_layer"], med["f16_layer_again"]) / med["mx_layer"] - 1.0
        out.append(dict(rows=rows, P=P, dim=D, ms=med, samples=samples, fp16_spread=spread, mx_gain_over_faster_fp16=gain, telemetry=tel))
        sclk, pw = (tel.get("sclk_mhz") or {}).get("mean"), (tel.get("power_w") or {}).get("mean")
        tf = lambda fl, ms: f"{fl / ms / 1e9:.0f} TFLOP/s"
        print(f"| {D} | {rows} | layer (statistics handed in) | {med['f16_layer']:.3f} / {med['f16_layer_again']:.3f} (spread {100 * spread:.1f} %) | {med['mx_layer']:.3f} | "
              f"{f16 / med['mx_layer']:.2f}x .. {min(med['f16_layer'], med['f16_layer_again']) / med['mx_layer']:.2f}x | {sclk and round(sclk)} MHz / {pw and round(pw)} W |")
        print(f"| {D} | {rows} | layer, fp16 with its own statistics pass | {med['f16_layer_own_stats']:.3f} | {med['mx_layer']:.3f} | {med['f16_layer_own_stats'] / med['mx_layer']:.2f}x | |")
        print(f"| {D} | {rows} | row statistics / LayerNorm + quantiser | {med['f16_pre']:.3f} | {med['mx_pre']:.3f} | {med['f16_pre'] / med['mx_pre']:.2f}x | |")
        print(f"| {D} | {rows} | q\\|k\\|v, N = {3 * D}, K = {D} | {med['f16_qkv']:.3f} ({tf(fl_qkv, med['f16_qkv'])}) | {med['mx_qkv']:.3f} ({tf(fl_qkv, med['mx_qkv'])}) | "
              f"{med['f16_qkv'] / med['mx_qkv']:.2f}x | |")
        print(f"| {D} | {rows} | attention kernel | {med['f16_attn']:.3f} | {med['mx_attn']:.3f} | {med['f16_attn'] / med['mx_attn']:.2f}x | |")
        print(f"| {D} | {rows} | to_out + residual, N = K = {D} | {med['f16_out']:.3f} ({tf(fl_out, med['f16_out'])}) | {med['mx_out']:.3f} ({tf(fl_out, med['mx_out'])}) | "
              f"{med['f16_out'] / med['mx_out']:.2f}x | |")
        print(f"  -> width {D}: MX layer faster than the faster fp16 series by {100 * gain:.1f} %, fp16 spread {100 * spread:.1f} %: "
              f"{'MX' if gain > spread else 'SKIP (keeps fp16)'}")
        sys.stdout.flush()
        del fns
        torch.cuda.empty_cache()
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
