"""Is the tile plan of vcx_gemm_f16 (csrc/gemm.hip plan_tiles: whole rounds of 256-row tiles, the remaining rows on a smaller
configuration chosen by a cost table) the best choice for every problem of the forward?  Times each problem of
profiles/gemm_shapes.json (the recorded descriptors: no model build) under the product dispatch and under each forced tile
configuration (knob GEMM_CFG = 0 .. 6: 128x128, 128x160, 256x256, 256x320, and the 64-row tail configurations 64x128, 64x64,
64x128 for GEGLU - a forced configuration also means the tiled engine where the product takes the weight-stationary kernel),
interleaved, min over rounds, and prints the plan's choice (segments cfg:rows) next to them.

    python tools/gemm_cfg_scan.py [--rounds 3] [--iters 5] [--min-total-ms 0.3] [--cfgs -1,0,1] [--json out.json]

VCX_LIB=path/to/libvcx.so times another build of the library (the parent commit's, for a same-box A/B of the product dispatch).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
if os.environ.get("VCX_LIB"):      # repo-relative or absolute; works because _lib.lib() reads the module global LIB_PATH at its first call, which is after this
    from viewcrafter_amd import _lib
    _lib.LIB_PATH = os.path.join(ROOT, os.environ["VCX_LIB"])
from viewcrafter_amd import ops  # noqa: E402
from gemm_shapes import FIELDS, _time, make_problem  # noqa: E402
from telemetry import Telemetry  # noqa: E402

CFG_NAME = {-1: "product", 0: "128x128", 1: "128x160", 2: "256x256", 3: "256x320", 4: "64x128", 5: "64x64", 6: "64x128g"}
ALL = (-1, 0, 1, 2, 3, 4, 5, 6)


def plan_of(run):
    """The plan's segments for one call, "cfg:rows+cfg:rows", from the library's trace on stderr (VCX_GEMM_PLAN_TRACE); "-" where
    the product does not take the tiled engine (weight-stationary kernels) or the library has no trace."""
    import re
    import tempfile
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["VCX_GEMM_PLAN_TRACE"] = "1"
        try:
            run()
            torch.cuda.synchronize()
        finally:
            os.environ.pop("VCX_GEMM_PLAN_TRACE", None)
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        segs = re.findall(r"cfg (\d+) rows \d+\+(\d+) grid (\d+)", tmp.read().decode("utf-8", "replace"))
    return "+".join(f"{c}:{r}/{g}" for c, r, g in segs) or "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=os.path.join(ROOT, "profiles", "gemm_shapes.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--min-total-ms", type=float, default=0.3, help="skip problems whose count x ms is below this")
    ap.add_argument("--cfgs", default=",".join(str(c) for c in ALL), help="configurations to time (-1 = the product dispatch)")
    ap.add_argument("--json", default=None, help="write the per-problem times here")
    args = ap.parse_args()
    want = tuple(int(c) for c in args.cfgs.split(","))
    records = []
    rows = json.load(open(args.shapes))["rows"]
    print(f"# {len(rows)} problems from {args.shapes}; ms per call, min over {args.rounds} interleaved rounds of {args.iters} launches")
    print(f"{'cnt':>4} {'M':>8} {'N':>6} {'K':>6} {'mode':>4} {'flags':>5} " + " ".join(f"{CFG_NAME[c]:>8}" for c in want) + "   best     gain x cnt  plan (cfg:rows/grid)")
    tot_prod = tot_best = 0.0
    for r in rows:
        if r["total_ms"] < args.min_total_ms or r["mode"] == 2:
            continue
        key = tuple(r[f] for f in FIELDS)
        run = make_problem(key)
        geglu = bool(r["flags"] & 16)
        cfgs = [c for c in want if c in ((-1, 0, 2, 6) if geglu else (-1, 0, 1, 2, 3, 4, 5))]
        plan = plan_of(run) if -1 in cfgs else "-"
        best = {c: float("inf") for c in cfgs}
        with Telemetry(device_index=0, period_s=0.02) as tm:      # the clock beside the number: boxes and minutes differ
            for _ in range(args.rounds):
                for c in cfgs:
                    prev = ops.tune_set("GEMM_CFG", c)
                    try:
                        best[c] = min(best[c], _time(run, args.iters))
                    except Exception as e:      # a configuration this epilogue is not instantiated for
                        best[c] = float("nan")
                        print(f"#   {r['M']}x{r['N']}x{r['K']} flags {r['flags']} cfg {c}: {type(e).__name__}", file=sys.stderr)
                    finally:
                        ops.tune_set("GEMM_CFG", prev)
        sclk = ((tm.summary() or {}).get("sclk_mhz") or {}).get("mean")
        del run
        if -1 not in best:
            continue
        torch.cuda.empty_cache()
        ok = {c: v for c, v in best.items() if v == v}
        cb = min(ok, key=ok.get)
        gain = (best[-1] - ok[cb]) * r["count"]
        tot_prod += best[-1] * r["count"]
        tot_best += ok[cb] * r["count"]
        cells = " ".join(f"{best.get(c, float('nan')):8.3f}" if c in best else f"{'-':>8}" for c in want)
        records.append(dict(M=r["M"], N=r["N"], K=r["K"], mode=r["mode"], flags=r["flags"], count=r["count"], plan=plan, sclk_mhz=sclk, ms={str(c): v for c, v in best.items()}))
        mark = "  <--" if cb != -1 and best[-1] > 1.03 * ok[cb] else ""
        print(f"{r['count']:4d} {r['M']:8d} {r['N']:6d} {r['K']:6d} {r['mode']:4d} {r['flags']:5d} {cells}   {CFG_NAME[cb]:>8} {gain:7.3f}{mark}  {plan}  {f'{sclk:.0f} MHz' if sclk else ''}")
    print(f"# product dispatch {tot_prod:.2f} ms, per-problem best {tot_best:.2f} ms: {tot_prod - tot_best:.2f} ms per forward pair to gain from a perfect rule")
    if args.json:
        json.dump(dict(lib=os.environ.get("VCX_LIB", "viewcrafter_amd/libvcx.so"), product_ms=tot_prod, rows=records), open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
