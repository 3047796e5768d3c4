"""Per-block A/B of one ResBlock, MXFP8 (VCX_RESCONV_MXFP8 route) against fp16 (the default route), isolated, with clock / power telemetry
beside every figure (tools/telemetry.py).  Writes the tables of profiles/mxfp8_resconv.md to stdout.

    python tools/mxfp8_resconv_ab.py [--rounds 3] [--iters 3] [--only 320,640]

The blocks are those of 576x1024x25 with classifier-free guidance (n = 2 videos x 25 frames) at every level: identity-skip, skip-conv and
split-concat (up path, [h | skip] read in place where the frame is whole 64-row strips) blocks at the grids 72x128 / 36x64 / 18x32 / 9x16.
Per block: ResBlock.forward (without its temporal block) on the fp16 route, on the MX route with the second convolution kept on the
folded fp16 kernel (RESCONV_MXFP8_KEEP_FOLD = 1) and with it on MX behind a separate skip convolution (= 0; the same thing for an
identity-skip block), and the first convolution alone (embedding addend + moments) on either engine.  Interleaved rounds, median."""
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
from viewcrafter_amd.packing import pack_conv, pack_conv3x3_mxfp8  # noqa: E402

DEV = "cuda"
B, T, EMB = 2, 25, 1280
# (H, W, c1, c2, cout): c2 = 0: one input tensor; c2 > 0: the up path's [h | skip]
BLOCKS = [
    (72, 128, 320, 0, 320), (72, 128, 640, 320, 320), (72, 128, 320, 320, 320),
    (36, 64, 640, 0, 640), (36, 64, 320, 0, 640), (36, 64, 1280, 640, 640), (36, 64, 640, 640, 640), (36, 64, 640, 320, 640),
    (18, 32, 1280, 0, 1280), (18, 32, 640, 0, 1280), (18, 32, 1280, 1280, 1280), (18, 32, 1280, 640, 1280),
    (9, 16, 1280, 0, 1280), (9, 16, 1280, 1280, 1280),
]


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


def colstats_of(x):
    """(mean, M2) per 64-row strip and column of x [M, C]: the moments the producing layer's epilogue would have written"""
    M, C = x.shape
    xs = x.float().view(M // 64, 64, C)
    mean = xs.mean(1)
    return torch.stack([mean, ((xs - mean.unsqueeze(1)) ** 2).sum(1)], dim=-1).contiguous()


def block(H, W, c1, c2, cout):
    cin, n = c1 + c2, B * T
    M = n * H * W
    torch.manual_seed(cin + cout)
    blk = U.ResBlock(cin, EMB, 0.0, out_channels=cout).eval()
    with torch.no_grad():
        for gn in (blk.in_layers[0], blk.out_layers[0]):
            gn.weight.copy_(1.0 + 0.2 * torch.randn(gn.weight.shape))
            gn.bias.copy_(0.1 * torch.randn(gn.bias.shape))
        for conv in (blk.in_layers[2], blk.out_layers[3]):
            conv.weight.copy_(torch.randn(conv.weight.shape) * (9 * conv.in_channels) ** -0.5)
            conv.bias.copy_(0.1 * torch.randn(conv.bias.shape))
    blk = blk.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(cin)
    x = (torch.randn(n, H, W, c1, device=DEV, generator=g) * 1.3).half()
    x2 = (torch.randn(n, H, W, c2, device=DEV, generator=g) * 0.8).half() if c2 else None
    emb = torch.randn(B, EMB, device=DEV, generator=g).half()
    whole = (H * W) % 64 == 0
    cs_in = colstats_of(torch.cat([x, x2], dim=-1).view(M, cin)) if (c2 and whole) else None
    conv1, gn1 = blk.in_layers[2], blk.in_layers[0]
    gw, gb = gn1.weight.detach().float(), gn1.bias.detach().float()
    xc = x if x2 is None else torch.cat([x, x2], dim=-1).contiguous()
    stats = ops.group_norm_stats(xc.view(n, H * W, cin))
    a16 = ops.group_norm(xc.view(n, H * W, cin), gw, gb, gn1.eps, True, stats=stats)
    amx = ops.group_norm_mxfp8(xc.view(n, H * W, cin), gw, gb, gn1.eps, True, stats=stats)
    del xc
    w16, wmx, bias = pack_conv(conv1.weight.detach()).half(), tuple(t.to(DEV) for t in pack_conv3x3_mxfp8(conv1.weight.detach())), conv1.bias.detach().float()
    rowadd = torch.randn(B, cout, device=DEV, generator=g)
    cs = ops.colstats_buffer(M, cout, DEV) if whole else None

    def run(flag, keep):
        def f():
            U.RESCONV_MXFP8, U.RESCONV_MXFP8_KEEP_FOLD = flag, keep
            with torch.no_grad():
                blk(x, emb, batch_size=B, want_colstats=whole, colstats=cs_in, x2=x2)
        return f

    return dict(f16_block=run(False, True), mx_block_fold=run(True, True), mx_block_nofold=run(True, False),
                f16_conv=lambda: ops.conv2d(a16.view(n, H, W, cin), w16, bias, kh=3, kw=3, rowadd=rowadd, rowadd_div=T * H * W, colstats=cs),
                mx_conv=lambda: ops.conv3x3_mxfp8(amx, wmx, bias, n=n, H=H, W=W, cin=cin, rowadd=rowadd, rowadd_div=T * H * W, colstats=cs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated out_channels to run")
    a = ap.parse_args()
    only = {int(v) for v in a.only.split(",") if v.strip()}
    ops.require_gpu()
    was = U.RESCONV_MXFP8, U.RESCONV_MXFP8_SKIP_DIMS, U.RESCONV_MXFP8_KEEP_FOLD
    U.RESCONV_MXFP8_SKIP_DIMS = frozenset()
    out = []
    order = ("f16_block", "mx_block_fold", "mx_block_nofold", "f16_conv", "mx_conv")
    try:
        for H, W, c1, c2, cout in BLOCKS:
            if only and cout not in only:
                continue
            fns = block(H, W, c1, c2, cout)
            samples = {k: [] for k in fns}
            with Telemetry(device_index=0, period_s=0.05) as tm:
                for _ in range(a.rounds):
                    for k in order:
                        samples[k].append(timed(fns[k], a.iters))
            med = {k: statistics.median(v) for k, v in samples.items()}
            rows, cin = B * T * H * W, c1 + c2
            kind = "identity" if (c2 == 0 and c1 == cout) else "skip conv" if c2 == 0 else "split concat"
            fl = 2.0 * rows * cout * 9 * cin
            tel = tm.summary()
            out.append(dict(grid=[H, W], rows=rows, c1=c1, c2=c2, cout=cout, kind=kind, ms=med, samples=samples, telemetry=tel))
            sclk, pw = (tel.get("sclk_mhz") or {}).get("mean"), (tel.get("power_w") or {}).get("mean")
            name = f"{c1}|{c2}" if c2 else f"{c1}"
            print(f"| {H}x{W} | {name} -> {cout} | {kind} | block | {med['f16_block']:.3f} | {med['mx_block_fold']:.3f} ({med['f16_block'] / med['mx_block_fold']:.2f}x) | "
                  f"{med['mx_block_nofold']:.3f} ({med['f16_block'] / med['mx_block_nofold']:.2f}x) | {sclk and round(sclk)} MHz / {pw and round(pw)} W |")
            print(f"| {H}x{W} | {name} -> {cout} | {kind} | conv1 K = 9 x {cin} | {med['f16_conv']:.3f} ({fl / med['f16_conv'] / 1e9:.0f} TFLOP/s) | "
                  f"{med['mx_conv']:.3f} ({fl / med['mx_conv'] / 1e9:.0f} TFLOP/s) ({med['f16_conv'] / med['mx_conv']:.2f}x) | | |")
            sys.stdout.flush()
            del fns
            torch.cuda.empty_cache()
    finally:
        U.RESCONV_MXFP8, U.RESCONV_MXFP8_SKIP_DIMS, U.RESCONV_MXFP8_KEEP_FOLD = was
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
