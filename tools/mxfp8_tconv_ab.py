"""Per-width A/B of one TemporalConvBlock, MXFP8 (VCX_TCONV_MXFP8 route) against fp16 (the default route), isolated, with clock / power
telemetry beside every figure (tools/telemetry.py).  Writes the table of profiles/mxfp8_tconv.md to stdout.

    python tools/mxfp8_tconv_ab.py [--rows-scale 1.0] [--rounds 3] [--iters 3]

Per level (width 320 / 640 / 1280 at the row counts of 576x1024x25: B = 2 videos x T = 25 frames x P = 9216 / 2304 / 576 pixels): the
whole block (four GroupNorm + SiLU applies and four (3,1,1) convolutions, moments travelling, residual on the last) through
TemporalConvBlock.forward on either route, and one apply pass and one convolution of either route timed apart.  Interleaved rounds,
median."""
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
from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U  # noqa: E402
from viewcrafter_amd.packing import pack_conv, pack_conv_t3_mxfp8  # noqa: E402

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


def level(P, C):
    torch.manual_seed(C)
    blk = U.TemporalConvBlock(C).eval()
    with torch.no_grad():
        for seq in (blk.conv1, blk.conv2, blk.conv3, blk.conv4):
            seq[0].weight.copy_(1.0 + 0.2 * torch.randn(C))
            seq[0].bias.copy_(0.1 * torch.randn(C))
            seq[-1].weight.copy_(torch.randn(C, C, 3, 1, 1) * (3 * C) ** -0.5)
            seq[-1].bias.copy_(0.1 * torch.randn(C))
    blk = blk.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(C)
    x = (torch.randn(B, T, P, C, device=DEV, generator=g) * 1.3).half()
    gn, conv = blk.conv2[0], blk.conv2[-1]
    gw, gb = gn.weight.detach().float(), gn.bias.detach().float()
    w16, wmx, bias = pack_conv(conv.weight.detach()).half(), pack_conv_t3_mxfp8(conv.weight.detach()), conv.bias.detach().float()
    stats = ops.group_norm_stats(x.view(B, T * P, C))
    state = dict(a16=ops.group_norm(x.view(B, T * P, C), gw, gb, gn.eps, True, stats=stats), amx=ops.group_norm_mxfp8(x.view(B, T * P, C), gw, gb, gn.eps, True, stats=stats))
    cs = ops.colstats_buffer(B * T * P, C, DEV) if (T * P) % 64 == 0 else None

    def block(flag):
        def run():
            U.TCONV_MXFP8 = flag
            with torch.no_grad():
                blk(x, want_colstats=P % 64 == 0)
        return run

    return dict(f16_block=block(False), mx_block=block(True),
                f16_apply=lambda: ops.group_norm(x.view(B, T * P, C), gw, gb, gn.eps, True, stats=stats),
                mx_apply=lambda: ops.group_norm_mxfp8(x.view(B, T * P, C), gw, gb, gn.eps, True, stats=stats),
                f16_conv=lambda: ops.temporal_conv3(state["a16"].view(B, T, P, C), w16, bias, **(dict(colstats=cs) if cs is not None else {})),
                mx_conv=lambda: ops.temporal_conv3_mxfp8(state["amx"], wmx, bias, B=B, T=T, P=P, cin=C, colstats=cs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-scale", type=float, default=1.0, help="scales P (rounded to a multiple of 64)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    ops.require_gpu()
    was = U.TCONV_MXFP8, U.TCONV_MXFP8_SKIP_DIMS
    U.TCONV_MXFP8_SKIP_DIMS = frozenset()
    out = []
    order = ("f16_block", "mx_block", "f16_apply", "mx_apply", "f16_conv", "mx_conv")
    try:
        for P, C in LEVELS:
            P = max(64, int(P * a.rows_scale) // 64 * 64)
            fns = level(P, C)
            samples = {k: [] for k in fns}
            with Telemetry(device_index=0, period_s=0.05) as tm:
                for _ in range(a.rounds):
                    for k in order:
                        samples[k].append(timed(fns[k], a.iters))
            med = {k: statistics.median(v) for k, v in samples.items()}
            rows = B * T * P
            fl = 2.0 * rows * C * 3 * C
            tel = tm.summary()
            out.append(dict(rows=rows, P=P, dim=C, ms=med, tflops=dict(f16_conv=fl / med["f16_conv"] / 1e9, mx_conv=fl / med["mx_conv"] / 1e9), telemetry=tel))
            sclk, pw = (tel.get("sclk_mhz") or {}).get("mean"), (tel.get("power_w") or {}).get("mean")
            print(f"| {C} | {rows} | block | {med['f16_block']:.3f} | {med['mx_block']:.3f} | {med['f16_block'] / med['mx_block']:.2f}x | {sclk and round(sclk)} MHz / {pw and round(pw)} W |")
            print(f"| {C} | {rows} | GroupNorm + SiLU apply | {med['f16_apply']:.3f} | {med['mx_apply']:.3f} | {med['f16_apply'] / med['mx_apply']:.2f}x | |")
            print(f"| {C} | {rows} | convolution K = 3 x {C} (+ moments) | {med['f16_conv']:.3f} ({fl / med['f16_conv'] / 1e9:.0f} TFLOP/s) | "
                  f"{med['mx_conv']:.3f} ({fl / med['mx_conv'] / 1e9:.0f} TFLOP/s) | {med['f16_conv'] / med['mx_conv']:.2f}x | |")
            sys.stdout.flush()
            del fns
            torch.cuda.empty_cache()
    finally:
        U.TCONV_MXFP8, U.TCONV_MXFP8_SKIP_DIMS = was
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
