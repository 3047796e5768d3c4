"""A/B of the spatial self-attention chain of one SpatialTransformer block - row statistics, projections, (pool,) attention kernel; up to, not
including, to_out - with VCX_SATTN_KV_POOL off against mean / nearest, in one process, rounds interleaved (off - mean - nearest - off again:
the two off series give the off route's own spread on this box), with clock / power telemetry beside every figure (tools/telemetry.py).
Writes the isolated tables of profiles/sattn_kv_pool.md to stdout.

    python tools/sattn_kv_pool_ab.py [--rounds 5] [--iters 10] [--levels 0,1]

Level 0: 2 videos x 25 frames of 72 x 128 tokens, D = 320 (9216 queries, 2304 pooled keys); level 1: 36 x 64 tokens, D = 640 (2304 / 576) - the
two levels of 576x1024x25 that can pool.  The parts are timed apart, and the pool kernel alone against layer_norm + avgpool2x2, the two
launches it is defined as."""
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
from viewcrafter_amd.lvdm.modules import attention as A  # noqa: E402

DEV = "cuda"
B, T = 2, 25
LEVELS = [(72, 128, 320), (36, 64, 640)]


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


def level(H, W, D):
    torch.manual_seed(D)
    heads, n, N, Np = D // 64, B * T, H * W, (H // 2) * (W // 2)
    st = A.SpatialTransformer(D, heads, 64, depth=1, context_dim=1024, use_checkpoint=False, use_linear=True, image_cross_attention=True).eval()
    with torch.no_grad():
        for m in st.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.2 * torch.randn(D))
                m.bias.copy_(0.1 * torch.randn(D))
    st = st.to(DEV)
    blk = st.transformer_blocks[0]
    lnp = blk.ln_params()[0]
    a1, pp = blk.attn1.packed(), blk.attn1.kv_pool_packed()
    tokens = n * N
    g = torch.Generator(device=DEV).manual_seed(D)
    t = (torch.randn(tokens, D, device=DEV, generator=g) * 1.3).half()
    alpha = math.sqrt(blk.attn1.scale * ops.LOG2E)
    for what, pj, tr in (("q|k", a1["qk"], False), ("V^T", a1["v"], True), ("q", pp["q"], False)):
        if not A._folded(pj, tokens, D, D, transposed=tr):
            print(f"(width {D}: the {what} projection is not folded at this shape - its rows include a LayerNorm pass)")
    o = torch.empty((tokens, D), dtype=torch.float16, device=DEV)

    def off():
        stt = ops.row_stats(t, lnp[2])
        qk = A.ln_linear(t, a1["qk"], lnp, alpha=alpha, stats=stt)
        vt = A.ln_linear_t(t, a1["v"], lnp, stats=stt)
        ops.flash_attn(qk, qk[:, D:], vt, o, n_groups=n, heads=heads, nq=N, nk=N, kv_rows=N, kv_div=1, ldq=2 * D, ldk=2 * D, ldvt=tokens, ldo=D,
                       scale=blk.attn1.scale, log2_logits=True)

    def pooled(mode):
        def run():
            prev, A.SATTN_KV_POOL = A.SATTN_KV_POOL, mode
            try:
                A._sattn_kv_pool(blk, lnp, t, A._self_attn_geometry(n, heads, N, N, D, (H // 2, W // 2)), None, (H, W))
            finally:
                A.SATTN_KV_POOL = prev
        return run

    # the parts, on operands made once
    st1 = ops.row_stats(t, lnp[2])
    qk = A.ln_linear(t, a1["qk"], lnp, alpha=alpha, stats=st1)
    vt = A.ln_linear_t(t, a1["v"], lnp, stats=st1)
    q = A.ln_linear(t, pp["q"], lnp, alpha=alpha, stats=st1)
    p = ops.layer_norm_pool2x2(t, *lnp, n, H, W, ops.POOL_MEAN)
    k = ops.linear(p, pp["wk"], None, alpha=alpha)
    vtp = ops.gemm(pp["wv"], p, M=D, N=n * Np, K=D, lda=D)
    geo_off = dict(n_groups=n, heads=heads, nq=N, nk=N, kv_rows=N, kv_div=1, ldq=2 * D, ldk=2 * D, ldvt=tokens, ldo=D, scale=1.0, log2_logits=True)
    geo_on = dict(n_groups=n, heads=heads, nq=N, nk=Np, kv_rows=Np, kv_div=1, ldq=D, ldk=D, ldvt=n * Np, ldo=D, scale=1.0, log2_logits=True)
    fns = dict(off=off, mean=pooled("mean"), nearest=pooled("nearest"), off_again=off,
               stats=lambda: ops.row_stats(t, lnp[2]),
               off_qk=lambda: A.ln_linear(t, a1["qk"], lnp, alpha=alpha, stats=st1), off_vt=lambda: A.ln_linear_t(t, a1["v"], lnp, stats=st1),
               off_attn=lambda: ops.flash_attn(qk, qk[:, D:], vt, o, **geo_off),
               on_q=lambda: A.ln_linear(t, pp["q"], lnp, alpha=alpha, stats=st1),
               on_pool_mean=lambda: ops.layer_norm_pool2x2(t, *lnp, n, H, W, ops.POOL_MEAN),
               on_pool_nearest=lambda: ops.layer_norm_pool2x2(t, *lnp, n, H, W, ops.POOL_NEAREST),
               on_k=lambda: ops.linear(p, pp["wk"], None, alpha=alpha), on_vt=lambda: ops.gemm(pp["wv"], p, M=D, N=n * Np, K=D, lda=D),
               on_attn=lambda: ops.flash_attn(q, k, vtp, o, **geo_on),
               two_launches=lambda: ops.avgpool2x2(ops.layer_norm(t, *lnp).view(n, H, W, D)))
    return fns, tokens, n * Np


PARTS = (("stats", "row statistics (both routes)"), ("off_qk", "off: q\\|k, N = 2 D"), ("off_vt", "off: V^T, N = tokens"), ("off_attn", "off: attention, nk = nq"),
         ("on_q", "on: q, N = D"), ("on_pool_mean", "on: LayerNorm + pool, mean"), ("on_pool_nearest", "on: LayerNorm + pool, nearest"),
         ("on_k", "on: k of the pooled rows"), ("on_vt", "on: V^T of the pooled rows"), ("on_attn", "on: attention, nk = nq / 4"),
         ("two_launches", "layer_norm + avgpool2x2 (what the mean pool kernel replaces)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--levels", default="0,1")
    a = ap.parse_args()
    ops.require_gpu()
    out = []
    for li in (int(v) for v in a.levels.split(",") if v):
        H, W, D = LEVELS[li]
        with torch.no_grad():
            fns, tokens, prows = level(H, W, D)
            order = list(fns)
            for k in order:                        # every shape of the timed window, warmed up
                timed(fns[k], 2)
            samples = {k: [] for k in fns}
            with Telemetry(device_index=0, period_s=0.05) as tm:
                for _ in range(a.rounds):
                    for k in order:
                        samples[k].append(timed(fns[k], a.iters))
        med = {k: statistics.median(v) for k, v in samples.items()}
        tel = tm.summary()
        lo, hi = sorted((med["off"], med["off_again"]))
        spread = (hi - lo) / lo
        sclk, pw = (tel.get("sclk_mhz") or {}).get("mean"), (tel.get("power_w") or {}).get("mean")
        print(f"\n### {B * T} frames of {H} x {W} tokens, D = {D} ({tokens} rows, {prows} pooled rows); {sclk and round(sclk)} MHz / {pw and round(pw)} W\n")
        print("| what | ms | against off |")
        print("|---|---|---|")
        print(f"| self-attention chain, switch off (two series) | {med['off']:.3f} / {med['off_again']:.3f} (spread {100 * spread:.1f} %) | |")
        for mode in ("mean", "nearest"):
            gain = lo - med[mode]
            verdict = "a gain" if gain > hi - lo else "inside the off route's spread"
            print(f"| self-attention chain, {mode} | {med[mode]:.3f} | {lo / med[mode]:.2f}x, -{gain:.3f} ms a call: {verdict} |")
        for k, what in PARTS:
            print(f"| {what} | {med[k]:.3f} | |")
        out.append(dict(H=H, W=W, dim=D, rows=tokens, pooled_rows=prows, ms=med, samples=samples, off_spread=spread, telemetry=tel))
        sys.stdout.flush()
        del fns
        torch.cuda.empty_cache()
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
