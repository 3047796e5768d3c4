"""Per-width A/B of the two attentions of one SpatialTransformer block (LayerNorm -> q|k, V^T -> self-attention -> to_out + residual ->
LayerNorm -> q -> text (+) image cross-attention -> to_out + residual), MXFP8 (VCX_SATTN_MXFP8 route) against fp16 (the default route),
isolated, with clock / power telemetry beside every figure (tools/telemetry.py).  Writes the table of profiles/mxfp8_sattn.md to stdout.

    python tools/mxfp8_sattn_ab.py [--rows-scale 1.0] [--rounds 5] [--iters 10] [--widths 320,640,1280]

Per level (width 320 / 640 / 1280 at the row counts of 576x1024x25: 2 videos x 25 frames of 9216 / 2304 / 576 tokens; 77 text keys and 256
image keys per video): both attentions on either route, and the parts timed apart.  The fp16 route is timed with the row statistics
handed in (in the model the GEMM that writes the token stream supplies them where ops.rowstats_ok holds - the form that is kindest to
fp16, and the one the skip rule compares against) and with its own statistics passes.  Every variant is warmed up, rounds are interleaved
(fp16 - MX - fp16 again: the two fp16 series give the fp16 route's own spread on this box), median over the rounds."""
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
B, T, CDIM, N_IMG = 2, 25, 1024, 256
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


def level(N, D):
    torch.manual_seed(D)
    heads, n = D // 64, B * T
    st = A.SpatialTransformer(D, heads, 64, depth=1, context_dim=CDIM, use_checkpoint=False, use_linear=True, image_cross_attention=True).eval()
    with torch.no_grad():
        for m in st.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.2 * torch.randn(D))
                m.bias.copy_(0.1 * torch.randn(D))
    st = st.to(DEV)
    blk = st.transformer_blocks[0]
    ln = blk.ln_params()
    a1, a2, m1, m2 = blk.attn1.packed(), blk.attn2.packed(), blk.attn1.mx_packed(), blk.attn2.mx_packed()
    tokens = n * N
    g = torch.Generator(device=DEV).manual_seed(D)
    t = (torch.randn(tokens, D, device=DEV, generator=g) * 1.3).half()
    txt = torch.zeros((B, 80, CDIM), dtype=torch.float16, device=DEV)
    txt[:, :77] = torch.randn(B, 77, CDIM, device=DEV, generator=g).half()
    img = torch.randn(B * N_IMG, CDIM, device=DEV, generator=g).half()
    kv = st.project_context(dict(txt=txt.view(B * 80, CDIM), img=img, n_img=N_IMG, per_frame=False))[0]
    geo1, geo2 = A._self_attn_geometry(n, heads, N, N, D), A._cross_attn_geometry(kv, n, heads, N, D, T)
    ctx = (kv.k_txt, kv.vt_txt, kv.k_img, kv.vt_img)
    assert (ops.linear_mxfp8_ok(tokens, 2 * D, D) and ops.linear_t_mxfp8_ok(tokens, D, D) and ops.linear_mxfp8_ok(tokens, D, D, residual=True)
            and ops.flash_attn_mxfp8_ok(**geo1) and ops.flash_attn_dual_mxfp8_ok(**geo2))
    for what, pj, tr in (("q|k", a1["qk"], False), ("V^T", a1["v"], True), ("q2", a2["q"], False)):
        if not A._folded(pj, tokens, D, D, transposed=tr):
            print(f"(width {D}: the fp16 {what} projection is not folded at this shape - its rows include a LayerNorm pass)")
    al1, al2 = math.sqrt(blk.attn1.scale * ops.LOG2E), blk.attn2.scale * ops.LOG2E
    st1 = ops.row_stats(t, ln[0][2])
    o16, o216 = (torch.empty((tokens, D), dtype=torch.float16, device=DEV) for _ in range(2))
    s = dict(qk=A.ln_linear(t, a1["qk"], ln[0], alpha=al1, stats=st1), vt=A.ln_linear_t(t, a1["v"], ln[0], stats=st1), an=ops.layer_norm_mxfp8(t, *ln[0]),
             q2=A.ln_linear(t, a2["q"], ln[1], alpha=al2, stats=st1))
    s["omx"] = ops.flash_attn_mxfp8(s["qk"], s["qk"][:, D:], s["vt"], **geo1)
    s["o2mx"] = ops.flash_attn_dual_mxfp8(s["q2"], kv.k_txt, kv.vt_txt, kv.k_img, kv.vt_img, **geo2)
    f16_self = lambda: ops.flash_attn(s["qk"], s["qk"][:, D:], s["vt"], o16, ldo=D, scale=1.0, log2_logits=True, **geo1)
    f16_cross = lambda: ops.flash_attn_dual(s["q2"], kv.k_txt, kv.vt_txt, kv.k_img, kv.vt_img, o216, ldo=D, scale=1.0, log2_logits=True, **geo2)
    f16_self(), f16_cross()

    def f16_layer(handed_in):
        def run():
            sa = st1 if handed_in else ops.row_stats(t, ln[0][2])
            qk = A.ln_linear(t, a1["qk"], ln[0], alpha=al1, stats=sa)
            vt = A.ln_linear_t(t, a1["v"], ln[0], stats=sa)
            ops.flash_attn(qk, qk[:, D:], vt, o16, ldo=D, scale=1.0, log2_logits=True, **geo1)
            t1 = ops.linear(o16, a1["wo"], a1["bo"], residual=t)
            q2 = A.ln_linear(t1, a2["q"], ln[1], alpha=al2, stats=st1 if handed_in else None)      # (timing: any statistics do)
            ops.flash_attn_dual(q2, kv.k_txt, kv.vt_txt, kv.k_img, kv.vt_img, o216, ldo=D, scale=1.0, log2_logits=True, **geo2)
            ops.linear(o216, a2["wo"], a2["bo"], residual=t1)
        return run

    def mx_layer():
        t1 = A._to_out(A._sattn_mx(blk, ln[0], t, geo1, None, None), m1, t, True)           # a block's two attentions on the MX route, as SpatialTransformer.forward runs them
        q2 = ops.linear_mxfp8(ops.layer_norm_mxfp8(t1, *ln[1]), m2["wq"], m2["zero"], K=D)
        A._to_out(A._attend(q2, ctx, geo2, blk.attn2.scale, True), m2, t1, True)

    return dict(f16_layer=f16_layer(True), mx_layer=mx_layer, f16_layer_again=f16_layer(True), f16_layer_own_stats=f16_layer(False),
                f16_pre=lambda: ops.row_stats(t, ln[0][2]), mx_pre=lambda: ops.layer_norm_mxfp8(t, *ln[0]),
                f16_qk=lambda: A.ln_linear(t, a1["qk"], ln[0], alpha=al1, stats=st1), mx_qk=lambda: ops.linear_mxfp8(s["an"], m1["wqk"], m1["zero"], K=D),
                f16_vt=lambda: A.ln_linear_t(t, a1["v"], ln[0], stats=st1), mx_vt=lambda: ops.linear_t_mxfp8(s["an"], m1["wv"], K=D),
                f16_self=f16_self, mx_self=lambda: ops.flash_attn_mxfp8(s["qk"], s["qk"][:, D:], s["vt"], **geo1),
                f16_out=lambda: ops.linear(o16, a1["wo"], a1["bo"], residual=t), mx_out=lambda: ops.linear_mxfp8(s["omx"], m1["wo"], m1["bo"], K=D, residual=t),
                f16_q2=lambda: A.ln_linear(t, a2["q"], ln[1], alpha=al2, stats=st1), mx_q2=lambda: ops.linear_mxfp8(s["an"], m2["wq"], m2["zero"], K=D),
                f16_cross=f16_cross, mx_cross=lambda: ops.flash_attn_dual_mxfp8(s["q2"], kv.k_txt, kv.vt_txt, kv.k_img, kv.vt_img, **geo2))


PARTS = (("pre", "row statistics / LayerNorm + quantiser (one of two)", 0), ("qk", "q\\|k, N = 2 D, K = D", 2), ("vt", "V^T, M = D, N = tokens", 1),
         ("self", "self-attention kernel", 0), ("out", "to_out + residual, N = K = D (one of two)", 1), ("q2", "q of the cross-attention, N = K = D", 1),
         ("cross", "text (+) image cross-attention kernel", 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-scale", type=float, default=1.0, help="scales the tokens per frame (rounded to a multiple of 64)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--widths", default="320,640,1280")
    a = ap.parse_args()
    ops.require_gpu()
    widths = {int(v) for v in a.widths.split(",") if v}
    out = []
    order = ("f16_layer", "mx_layer", "f16_layer_again", "f16_layer_own_stats") + tuple(f"{r}_{k}" for k, _, _ in PARTS for r in ("f16", "mx"))
    print("| width | rows | what | fp16 ms | MXFP8 ms | fp16 / MXFP8 | clock / power |")
    print("|---|---|---|---|---|---|---|")
    for N, D in LEVELS:
        if D not in widths:
            continue
        N = max(64, int(N * a.rows_scale) // 64 * 64)
        with torch.no_grad():
            fns = level(N, D)
            for k in order:                        # every shape of the timed window, warmed up
                timed(fns[k], 2)
            samples = {k: [] for k in fns}
            with Telemetry(device_index=0, period_s=0.05) as tm:
                for _ in range(a.rounds):
                    for k in order:
                        samples[k].append(timed(fns[k], a.iters))
        med = {k: statistics.median(v) for k, v in samples.items()}
        rows = B * T * N
        tel = tm.summary()
        lo, hi = sorted((med["f16_layer"], med["f16_layer_again"]))
        spread, gain = (hi - lo) / lo, lo / med["mx_layer"] - 1.0
        out.append(dict(rows=rows, tokens_per_frame=N, dim=D, ms=med, samples=samples, fp16_spread=spread, mx_gain_over_faster_fp16=gain, telemetry=tel))
        sclk, pw = (tel.get("sclk_mhz") or {}).get("mean"), (tel.get("power_w") or {}).get("mean")
        print(f"| {D} | {rows} | both attentions (statistics handed in) | {med['f16_layer']:.3f} / {med['f16_layer_again']:.3f} (spread {100 * spread:.1f} %) | "
              f"{med['mx_layer']:.3f} | {hi / med['mx_layer']:.3f}x .. {lo / med['mx_layer']:.3f}x | {sclk and round(sclk)} MHz / {pw and round(pw)} W |")
        print(f"| {D} | {rows} | both attentions, fp16 with its own statistics passes | {med['f16_layer_own_stats']:.3f} | {med['mx_layer']:.3f} | "
              f"{med['f16_layer_own_stats'] / med['mx_layer']:.3f}x | |")
        for k, what, nd in PARTS:
            f, m = med[f"f16_{k}"], med[f"mx_{k}"]
            tf = lambda ms: f" ({2.0 * rows * D * nd * D / ms / 1e9:.0f} TFLOP/s)" if nd else ""
            print(f"| {D} | {rows} | {what} | {f:.3f}{tf(f)} | {m:.3f}{tf(m)} | {f / m:.2f}x | |")
        print(f"  -> width {D}: MX faster than the faster fp16 series by {100 * gain:.1f} %, fp16 spread {100 * spread:.1f} %: "
              f"{'MX' if gain > spread else 'SKIP (keeps fp16)'}")
        sys.stdout.flush()
        del fns
        torch.cuda.empty_cache()
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
