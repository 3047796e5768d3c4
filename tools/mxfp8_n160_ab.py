"""Isolated A/B of the MXFP8 GEMM kernel's two tile configurations at the 320-wide level (profiles/mxfp8_n160.md): every problem is timed on
up to three builds in ONE process, interleaved round by round (after one unrecorded warm-up round), with the clock sampled beside every
measurement (tools/telemetry.py):

    parent   another build of the library (--parent path/to/libvcx.so, e.g. the parent commit's; any ABI - only the three MXFP8 launchers
             are called, whose signatures have not changed since ABI 14)
    cfg0     this tree's library under VCX_GEMM_MX_CFG=0 (128 x 128 tiles everywhere: must be level with parent)
    cfg1     this tree's library under VCX_GEMM_MX_CFG=1 (128 x 160 tiles)

The knob is read once per loaded library, so cfg0 and cfg1 are two private copies of libvcx.so loaded side by side, each asked for its
configuration once while the environment variable holds its value.  Outputs are compared bit for bit across the builds.

    python tools/mxfp8_n160_ab.py [--parent other/libvcx.so] [--rounds 7] [--iters 20] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from ctypes import c_int, c_int64, c_void_p

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BIAS, ROWADD, RES, COLSTATS = 1, 4, 8, 0x200


def load(path, knob):
    if knob is None:
        os.environ.pop("VCX_GEMM_MX_CFG", None)
    else:
        os.environ["VCX_GEMM_MX_CFG"] = knob
    L = ctypes.CDLL(path)
    L.vcx_last_error.restype = ctypes.c_char_p
    L.vcx_gemm_mxfp8.argtypes = [c_void_p] * 8 + [c_int64] * 5 + [c_int, c_void_p]
    L.vcx_conv_t3_mxfp8.argtypes = [c_void_p] * 8 + [c_int64] * 8 + [c_int, c_void_p]
    L.vcx_conv3x3_mxfp8.argtypes = [c_void_p] * 9 + [c_int64] * 10 + [c_int, c_void_p]
    if hasattr(L, "vcx_gemm_mxfp8_cfg"):
        L.vcx_gemm_mxfp8_cfg.argtypes = [c_int64, c_int, c_int]
        got = L.vcx_gemm_mxfp8_cfg(320, BIAS, 0)          # the first use: the knob is read here
        assert got == (1 if knob is None else int(knob)), (path, knob, got)
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from telemetry import Telemetry
    from viewcrafter_amd import _lib, ops
    ops.require_gpu()
    tmp = tempfile.mkdtemp(prefix="vcx_n160_")
    libs = {}
    if args.parent:
        libs["parent"] = load(os.path.abspath(args.parent), None)
    for name, knob in (("cfg0", "0"), ("cfg1", "1")):
        copy = os.path.join(tmp, f"libvcx_{name}.so")
        shutil.copyfile(_lib.LIB_PATH, copy)
        libs[name] = load(copy, knob)
    os.environ.pop("VCX_GEMM_MX_CFG", None)
    dev = "cuda"
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(5)

    def mx(rows, K):
        return ops.quant_mxfp8(torch.randn((rows, K), generator=g, device=dev, dtype=torch.float16))

    def problem(kind, dims, cin, N, flags):
        """-> (label, call(L, out, cs) -> rc, M, FLOP)"""
        kp = (cin + 127) // 128 * 128
        taps = {"linear": 1, "t3": 3, "c9": 9}[kind]
        if kind == "linear":
            M = dims[0]
        else:
            M = dims[0] * dims[1] * dims[2]
        a, w = mx(M, cin), mx(N, taps * kp)
        bias = torch.randn((N,), generator=g, device=dev)
        res = torch.randn((M, N), generator=g, device=dev, dtype=torch.float16) if flags & RES else None
        rowadd = torch.randn((1, N), generator=g, device=dev) if flags & ROWADD else None
        p = lambda t: None if t is None else t.data_ptr()
        if kind == "linear":
            call = lambda L, out, cs: L.vcx_gemm_mxfp8(a[0].data_ptr(), a[1].data_ptr(), w[0].data_ptr(), w[1].data_ptr(), out.data_ptr(), None, bias.data_ptr(), p(res),
                                                       M, N, cin, N, N, flags, stream)
        elif kind == "t3":
            B, T, P = dims
            call = lambda L, out, cs: L.vcx_conv_t3_mxfp8(a[0].data_ptr(), a[1].data_ptr(), w[0].data_ptr(), w[1].data_ptr(), out.data_ptr(), bias.data_ptr(), p(res), p(cs),
                                                          B, T, P, cin, N, N, N, N, flags, stream)
        else:
            n, H, W = dims
            call = lambda L, out, cs: L.vcx_conv3x3_mxfp8(a[0].data_ptr(), a[1].data_ptr(), w[0].data_ptr(), w[1].data_ptr(), out.data_ptr(), bias.data_ptr(), p(rowadd),
                                                          p(res), p(cs), n, H, W, cin, N, N, N, N, N, M, flags, stream)
        names = "+".join(n for n, f in (("rowadd", ROWADD), ("residual", RES), ("colstats", COLSTATS)) if flags & f) or "bias"
        return f"{kind} {'x'.join(map(str, dims))} {cin}->{N} {names}", call, M, 2.0 * M * N * taps * cin

    P0 = 72 * 128
    problems = [("c9", (25, 72, 128), 320, 320, BIAS | ROWADD | COLSTATS), ("c9", (25, 72, 128), 640, 320, BIAS | ROWADD | COLSTATS),
                ("c9", (25, 72, 128), 960, 320, BIAS | ROWADD | COLSTATS), ("c9", (25, 72, 128), 320, 320, BIAS | RES),
                ("t3", (1, 25, P0), 320, 320, BIAS | COLSTATS), ("t3", (1, 25, P0), 320, 320, BIAS | RES),
                ("linear", (2 * 25 * P0,), 1280, 320, BIAS | RES), ("linear", (2 * 25 * P0,), 320, 320, BIAS | RES), ("linear", (2 * 25 * P0,), 320, 960, BIAS)]
    results = []
    for spec in problems:
        label, call, M, flops = problem(*spec)
        N = spec[3]
        outs = {k: torch.empty((M, N), dtype=torch.float16, device=dev) for k in libs}
        css = {k: torch.zeros((M // 64, N, 2), device=dev) if spec[4] & COLSTATS else None for k in libs}
        for k, L in libs.items():          # warm-up, and the bytes
            rc = call(L, outs[k], css[k])
            assert rc == 0, (label, k, L.vcx_last_error())
        torch.cuda.synchronize()
        same = all(torch.equal(outs[k], outs["cfg0"]) and (css[k] is None or torch.equal(css[k], css["cfg0"])) for k in libs)
        times = {k: [] for k in libs}
        tm = Telemetry(period_s=0.02)
        with tm:
            for r in range(-1, args.rounds):          # round -1 is a warm-up through every build (clocks, caches) and is not recorded
                for k, L in libs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    call(L, outs[k], css[k])
                    e0.record()
                    for _ in range(args.iters):
                        call(L, outs[k], css[k])
                    e1.record()
                    torch.cuda.synchronize()
                    if r >= 0:
                        times[k].append(e0.elapsed_time(e1) / args.iters)
            time.sleep(0.05)
        tel = tm.summary()
        row = {"problem": label, "bit_equal": same, "sclk_mhz": (tel.get("sclk_mhz") or {}).get("mean"), "power_w": (tel.get("power_w") or {}).get("mean")}
        for k, v in times.items():
            row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                      "tflops": round(flops / statistics.median(v) * 1e-9, 1)}
        base = "parent" if "parent" in libs else "cfg0"
        row["cfg1_speedup_vs_" + base] = round(row[base]["median_ms"] / row["cfg1"]["median_ms"], 3)
        row[base + "_spread"] = round(row[base]["max_ms"] / row[base]["min_ms"], 3)          # slowest / fastest round of the baseline
        row["cfg1_slowest_round_beats_" + base + "_fastest"] = row["cfg1"]["max_ms"] < row[base]["min_ms"]
        if base == "parent":
            row["cfg0_vs_parent"] = round(row["parent"]["median_ms"] / row["cfg0"]["median_ms"], 3)
        results.append(row)
        print(json.dumps(row), flush=True)
        del outs, css
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
