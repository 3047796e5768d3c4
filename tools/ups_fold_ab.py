"""Per-layer A/B of the folded upsample convolution (ops.conv2d_ups_folded, four 2x2 weight sets) against the nine-tap ups = 1 call, same
process: the three Upsample layers of the default workload (576x1024x25, CFG as one B = 2 forward: 50 frames), each with the column-moment
epilogue it has in the graph.  Legs in the order fold, parent, parent, fold; HIP events around a leg, tools/telemetry.py's mean graphics
clock beside it.  A layer the route refuses (vcx_gemm_route) is timed on the nine-tap call alone.
    python tools/ups_fold_ab.py [--calls 40] [--warmup 5] [--plain]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LAYERS = [("level 1 -> 0, source 36x64, 640 -> 640", 50, 36, 64, 640, 640), ("level 2 -> 1, source 18x32, 1280 -> 1280", 50, 18, 32, 1280, 1280),
          ("level 3 -> 2, source 9x16, 1280 -> 1280", 50, 9, 16, 1280, 1280)]


def leg(run, calls, warmup):
    from telemetry import Telemetry
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    with Telemetry(period_s=0.02) as tm:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(calls):
            run()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
    s = tm.summary(t0, t1)
    return a.elapsed_time(b) / calls, (s.get("sclk_mhz") or {}).get("mean") or float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--plain", action="store_true", help="without the column-moment epilogue")
    args = ap.parse_args()
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv, pack_conv_ups_folded
    ops.require_gpu()
    os.environ["VCX_GEMM_PLAN_TRACE"] = "1"
    print("| layer | fold ms (1st / 2nd leg) | nine-tap ms (1st / 2nd leg) | best fold / best nine-tap | nine-tap spread | sclk MHz per leg | TF/s launched (fold / nine-tap) |")
    print("|---|---|---|---|---|---|---|")
    for name, n, H, W, cin, cout in LAYERS:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((n, H, W, cin), generator=g, device="cuda").half()
        w = (torch.randn((cout, cin, 3, 3), generator=g, device="cuda") * (9 * cin) ** -0.5).half()
        b = torch.randn((cout,), generator=g, device="cuda")
        w9, wf = pack_conv(w), pack_conv_ups_folded(w)
        M = n * 4 * H * W
        want_cs = not args.plain and ops.colstats_ok(M, 4 * H * W, cin, cout, in_rows=n * H * W)
        cs = ops.colstats_buffer(M, cout, "cuda") if want_cs else None
        out = torch.empty((M, cout), dtype=torch.float16, device="cuda")
        kw = dict(out=out, ldc=cout, **(dict(colstats=cs) if want_cs else {}))
        nine = lambda: ops.conv2d(x, w9, b, kh=3, kw=3, ups=1, **kw)
        fold = lambda: ops.conv2d_ups_folded(x, wf, b, **kw)
        takes = ops.conv2d_ups_folded_ok(n, H, W, cin, cout, colstats=want_cs)
        print(f"# {name}: plans (stderr) of one call each, fold {'taken' if takes else 'REFUSED by the route'}, column moments {'on' if want_cs else 'off'}", flush=True)
        nine()
        if takes:
            fold()
        torch.cuda.synchronize()
        del os.environ["VCX_GEMM_PLAN_TRACE"]
        order = [fold, nine, nine, fold] if takes else [nine, nine]
        res = [leg(r, args.calls, args.warmup) for r in order]
        os.environ["VCX_GEMM_PLAN_TRACE"] = "1"
        clk = ", ".join(f"{c:.0f}" for _, c in res)
        f9 = 2.0 * M * cout * 9 * cin
        if takes:
            (f1, _), (p1, _), (p2, _), (f2, _) = res
            print(f"| {name} | {f1:.3f} / {f2:.3f} | {p1:.3f} / {p2:.3f} | {min(f1, f2) / min(p1, p2):.3f} | {abs(p1 - p2):.3f} ms | {clk} | "
                  f"{f9 * 4 / 9 / min(f1, f2) / 1e9:.0f} / {f9 / min(p1, p2) / 1e9:.0f} |", flush=True)
        else:
            (p1, _), (p2, _) = res
            print(f"| {name} | refused | {p1:.3f} / {p2:.3f} | - | {abs(p1 - p2):.3f} ms | {clk} | - / {f9 / min(p1, p2) / 1e9:.0f} |", flush=True)
        del x, w, w9, wf, out, cs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
