"""Per-block A/B of the ResBlocks with a skip convolution: fp16 (the default route), VCX_RESCONV_MXFP8=1 as shipped, and the same plus
VCX_RESCONV_MXFP8_TAIL=1 (the skip convolution as a K tail of the MX second convolution), isolated, with clock / power telemetry beside
every figure (tools/telemetry.py).  Writes the tables of profiles/mxfp8_resconv_tail.md to stdout.

    python tools/mxfp8_resconv_tail_ab.py [--rounds 5] [--iters 3] [--only 320,640]

The blocks are the skip-conv and split-concat rows of tools/mxfp8_resconv_ab.py: 576x1024x25 with classifier-free guidance (n = 2 videos x
25 frames) at the grids 72x128 / 36x64 / 18x32 / 9x16.  Per block: ResBlock.forward (without its temporal block) on the three routes, the
quantising GroupNorm apply with and without its raw second output, and the tailed convolution alone.  The baseline of every figure is the
same tree with the new switch off.  Interleaved rounds in one process, median; `spread` is (max - min) / median of the shipped MX route's
rounds - a gain inside it is not a gain."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.mxfp8_resconv_ab import B, BLOCKS, DEV, EMB, T, colstats_of, timed  # noqa: E402
from tools.telemetry import Telemetry  # noqa: E402
from viewcrafter_amd import ops  # noqa: E402
from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U  # noqa: E402
from viewcrafter_amd.packing import pack_conv3x3_tail_mxfp8  # noqa: E402


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
    inplace = cs_in is not None          # the concat is read in place where its moments exist (ResBlock._plan), else materialised once
    gn1 = blk.in_layers[0]
    gw, gb = gn1.weight.detach().float(), gn1.bias.detach().float()
    xc = x if x2 is None else torch.cat([x, x2], dim=-1).contiguous()
    stats = ops.group_norm_stats(xc.view(n, H * W, cin))
    if inplace:
        nx, nx2 = x.view(n, H * W, c1), x2.view(n, H * W, c2)
        del xc
    else:
        nx, nx2 = xc.view(n, H * W, cin), None
    a2 = ops.quant_mxfp8((torch.randn(M, cout, device=DEV, generator=g)).half())
    _, xq = ops.group_norm_mxfp8_raw(nx, gw, gb, gn1.eps, True, stats=stats, x2=nx2)
    w2s = tuple(t.to(DEV) for t in pack_conv3x3_tail_mxfp8(blk.out_layers[3].weight.detach(), blk.skip_connection.weight.detach()))
    b2s = (blk.out_layers[3].bias + blk.skip_connection.bias).detach().float().contiguous()
    cs = ops.colstats_buffer(M, cout, DEV) if whole else None

    def run(flag, tail):
        def f():
            U.RESCONV_MXFP8, U.RESCONV_MXFP8_KEEP_FOLD, U.RESCONV_MXFP8_TAIL = flag, False, tail
            with torch.no_grad():
                blk(x, emb, batch_size=B, want_colstats=whole, colstats=cs_in, x2=x2)
        return f

    return dict(f16_block=run(False, False), mx_block=run(True, False), tail_block=run(True, True),
                norm=lambda: ops.group_norm_mxfp8(nx, gw, gb, gn1.eps, True, stats=stats, x2=nx2),
                norm_raw=lambda: ops.group_norm_mxfp8_raw(nx, gw, gb, gn1.eps, True, stats=stats, x2=nx2),
                tail_conv=lambda: ops.conv3x3_tail_mxfp8(a2, xq, w2s, b2s, n=n, H=H, W=W, cin=cout, ct=cin, colstats=cs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated out_channels to run")
    a = ap.parse_args()
    only = {int(v) for v in a.only.split(",") if v.strip()}
    ops.require_gpu()
    was = U.RESCONV_MXFP8, U.RESCONV_MXFP8_SKIP_DIMS, U.RESCONV_MXFP8_KEEP_FOLD, U.RESCONV_MXFP8_TAIL
    U.RESCONV_MXFP8_SKIP_DIMS = frozenset()
    out = []
    order = ("f16_block", "mx_block", "tail_block", "norm", "norm_raw", "tail_conv")
    try:
        for H, W, c1, c2, cout in BLOCKS:
            if (c2 == 0 and c1 == cout) or (only and cout not in only):          # identity-skip blocks have no skip convolution
                continue
            fns = block(H, W, c1, c2, cout)
            samples = {k: [] for k in fns}
            with Telemetry(device_index=0, period_s=0.05) as tm:
                for _ in range(a.rounds):
                    for k in order:
                        samples[k].append(timed(fns[k], a.iters))
            med = {k: statistics.median(v) for k, v in samples.items()}
            spread = (max(samples["mx_block"]) - min(samples["mx_block"])) / med["mx_block"]
            rows, cin = B * T * H * W, c1 + c2
            kind = "skip conv" if c2 == 0 else "split concat" if (H * W) % 64 == 0 else "split concat (materialised)"
            fl = 2.0 * rows * cout * (9 * cout + cin)
            tel = tm.summary()
            out.append(dict(grid=[H, W], rows=rows, c1=c1, c2=c2, cout=cout, kind=kind, ms=med, samples=samples, spread=spread, telemetry=tel))
            sclk, pw = (tel.get("sclk_mhz") or {}).get("mean"), (tel.get("power_w") or {}).get("mean")
            name = f"{c1}\\|{c2}" if c2 else f"{c1}"
            print(f"| {H}x{W} | {name} -> {cout} | {kind} | {med['f16_block']:.3f} | {med['mx_block']:.3f} | {med['tail_block']:.3f} | "
                  f"{med['mx_block'] / med['tail_block']:.2f}x | {100 * spread:.1f} % | {med['norm']:.3f} | {med['norm_raw']:.3f} | "
                  f"{med['tail_conv']:.3f} ({fl / med['tail_conv'] / 1e9:.0f} TFLOP/s) | {sclk and round(sclk)} MHz / {pw and round(pw)} W |")
            sys.stdout.flush()
            del fns
            torch.cuda.empty_cache()
    finally:
        U.RESCONV_MXFP8, U.RESCONV_MXFP8_SKIP_DIMS, U.RESCONV_MXFP8_KEEP_FOLD, U.RESCONV_MXFP8_TAIL = was
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
