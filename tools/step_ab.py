"""Same-box, same-process A/B of one DDIM step (bench.py's own step: shared CFG prefix, DDIM update) under host-side switches and library
knobs, variants interleaved round by round.  Prints ms per step and the per-family HIP-event times of every round.

    python tools/step_ab.py [--rounds 3] [--steps 3] [--lib other/libvcx.so] [--workload ...] variant [variant ...]

A variant is  name:key=value,key=value  with keys
    gnfold   0 | 1   TemporalTransformer.norm folded into proj_in (viewcrafter_amd/lvdm/modules/attention.py GN_FOLD)
    gnspatial 0 | 1 | 2  ... and SpatialTransformer.norm at level 0 (GN_FOLD_SPATIAL); 2 = at every width with a one-plan per-unit route
    lnff     0 | 1 | 2   LayerNorm folded into the GEGLU projection (FOLD_LAYERNORM_FF); 2 = only at C >= 640 (levels 1-3)
    xattn    1 | 2   resident cross-attention kernel: second form | first form (knob XATTN_RESIDENT)
    ws       1 | 0   weight-stationary K = 320 kernel (knob GEMM_WS)
    lnrs     1 | 0   LayerNorm statistics from the producing layer's epilogue (VCX_GEMM_ROWSTATS; ops.LN_ROWSTATS)
    upsfold  1 | 0   Upsample convolutions as four 2x2 weight sets on the source grid (ops.UPS_FOLD; 0 = the nine-tap ups = 1 call)
    ffout    1 | 0   a transformer's ff.net[2] + proj_out as one GEMM with a K tail (attention.FF_OUT_FOLD)
    ffskip   widths joined by '+' that keep two calls (attention.FF_OUT_FOLD_SKIP_DIMS), e.g. ffskip=1280 or ffskip=640+1280
    tattn    0 | 1   temporal attention on the MXFP8 route (attention.TATTN_MXFP8; off by default)
    tattnskip widths joined by '+' that keep fp16 with tattn=1 (attention.TATTN_MXFP8_SKIP_DIMS), e.g. tattnskip=320; tattnskip= for none
    sattn    0 | 1   spatial attention on the MXFP8 route (attention.SATTN_MXFP8; off by default)
    sattnskip widths joined by '+' that keep fp16 with sattn=1 (attention.SATTN_MXFP8_SKIP_DIMS), e.g. sattnskip=320; sattnskip= for none
    kvpool   0 | mean | nearest   spatial self-attention over 2x2-pooled keys and values (attention.SATTN_KV_POOL; off by default), with
             kvpoolmin = tokens a frame from which a level pools (attention.SATTN_KV_POOL_MIN_TOKENS, default 4096: level 0 of 576x1024 only),
             e.g.  off:kvpool=0  mean:kvpool=mean  mean2:kvpool=mean,kvpoolmin=2048
    ff / tconv / resconv  0 | 1   the feed-forward pair / TemporalConvBlock / ResBlock convolutions on the MXFP8 route (attention.FF_MXFP8,
             openaimodel3d.TCONV_MXFP8 / RESCONV_MXFP8; off by default), with ffmxskip / tconvskip / resconvskip = widths joined by '+' that keep
             fp16 (the *_SKIP_DIMS lists; `tconvskip=` for none)
    restail  0 | 1   with resconv=1: a ResBlock's skip convolution as a K tail of its MXFP8 second convolution (openaimodel3d.RESCONV_MXFP8_TAIL;
             off by default), e.g.  mx:resconv=1  tail:resconv=1,restail=1
    fcache   N       feature cache (viewcrafter_amd/feature_cache.py): timed step i is a full forward iff i % N == 0, shallow otherwise (the
             warm-up step fills the slot); 0 / 1 / absent = no cache object.  fcdepth = d (default 0)
e.g.   base:gnfold=0,xattn=2  gnfold:gnfold=1,xattn=2  xattn2:gnfold=0,xattn=1  all:gnfold=1,xattn=1
--lib runs everything on another build of the library of the SAME ABI (e.g. tools/_abl/libvcx_gelu_select.so, built by
tools/build_abl.sh): a library-level change is then compared across two invocations on the same box."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="+")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--workload", default="ViewCrafter_25_576x1024x25")
    args = ap.parse_args()
    from viewcrafter_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from bench import WORKLOADS, synth_conditioning
    from viewcrafter_amd import ops
    from viewcrafter_amd.builder import build_diffusion_model, randomize_parameters
    from viewcrafter_amd.feature_cache import FeatureCache
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from viewcrafter_amd.lvdm.modules import attention
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d
    ops.require_gpu()
    print(f"library: {_lib.LIB_PATH}", flush=True)
    cfg_name, T, h, w = WORKLOADS[args.workload]
    torch.manual_seed(123)
    model = build_diffusion_model(os.path.join(ROOT, "configs", cfg_name), device="cuda", conditioners="identity")
    randomize_parameters(model, seed=0)
    x0, cond, uc = synth_conditioning(T, h, w, "cuda", seed=123)
    fs = torch.tensor([10], device="cuda")
    sampler = DDIMSampler(model)
    sampler.make_schedule(ddim_num_steps=50, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    sampler._cfg_cache = None
    sampler.share_cfg_prefix = True
    n_sched = len(sampler.ddim_timesteps)

    def one_step(x, i, fcache=None, interval=0):
        index = n_sched - 1 - (i % n_sched)
        ts = torch.full((1,), int(sampler.ddim_timesteps[index]), device="cuda", dtype=torch.long)
        kw = {}
        if fcache is not None:
            fcache.set_mode("full" if i % interval == 0 else "shallow")
            kw["feature_cache"] = fcache
        x, _ = sampler.p_sample_ddim(x, cond, ts, index=index, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, fs=fs,
                                     guidance_rescale=0.7, cfg_img=None, unconditional_conditioning_img_nonetext=None, **kw)
        return x

    variants = []
    for v in args.variants:
        name, _, kv = v.partition(":")
        variants.append((name, dict(item.split("=") for item in kv.split(",") if item)))

    default_ffskip = attention.FF_OUT_FOLD_SKIP_DIMS
    default_tattn = attention.TATTN_MXFP8, attention.TATTN_MXFP8_SKIP_DIMS
    default_sattn = attention.SATTN_MXFP8, attention.SATTN_MXFP8_SKIP_DIMS
    default_kvpool = attention.SATTN_KV_POOL, attention.SATTN_KV_POOL_MIN_TOKENS

    mx_switches = {"ff": (attention, "FF_MXFP8", "ffmxskip"), "tconv": (openaimodel3d, "TCONV_MXFP8", "tconvskip"),
                   "resconv": (openaimodel3d, "RESCONV_MXFP8", "resconvskip")}
    default_mx = {k: (getattr(mod, name), getattr(mod, name + "_SKIP_DIMS")) for k, (mod, name, _) in mx_switches.items()}
    default_restail = openaimodel3d.RESCONV_MXFP8_TAIL

    def apply(settings):
        for k, (mod, name, skip) in mx_switches.items():
            setattr(mod, name, settings[k] != "0" if k in settings else default_mx[k][0])
            setattr(mod, name + "_SKIP_DIMS", frozenset(int(v) for v in settings[skip].split("+") if v) if skip in settings else default_mx[k][1])
        openaimodel3d.RESCONV_MXFP8_TAIL = settings["restail"] != "0" if "restail" in settings else default_restail
        attention.GN_FOLD = settings.get("gnfold", "1") != "0"
        attention.GN_FOLD_SPATIAL = {"0": 0, "2": 2}.get(settings.get("gnspatial", "1"), 1)
        lnff, lnff_min = settings.get("lnff", "2") != "0", (640 if settings.get("lnff", "2") == "2" else 0)      # 2 (the product): levels 1-3 only (C >= 640)
        if lnff != attention.FOLD_LAYERNORM_FF or lnff_min != attention.FOLD_LAYERNORM_FF_MIN_DIM:
            attention.FOLD_LAYERNORM_FF, attention.FOLD_LAYERNORM_FF_MIN_DIM = lnff, lnff_min
            for m in model.modules():
                if isinstance(m, attention.FeedForward):
                    m._drop_packed()
        ops.tune_set("XATTN_RESIDENT", int(settings.get("xattn", "1")))
        ops.tune_set("GEMM_WS", int(settings.get("ws", "1")))
        ops.LN_ROWSTATS = settings.get("lnrs", "1") != "0"
        ops.UPS_FOLD = settings.get("upsfold", "1") != "0"
        attention.FF_OUT_FOLD = settings.get("ffout", "1") != "0"
        if "ffskip" in settings:
            attention.FF_OUT_FOLD_SKIP_DIMS = frozenset(int(v) for v in settings["ffskip"].split("+") if v)
        else:
            attention.FF_OUT_FOLD_SKIP_DIMS = default_ffskip
        attention.TATTN_MXFP8 = settings["tattn"] != "0" if "tattn" in settings else default_tattn[0]
        attention.TATTN_MXFP8_SKIP_DIMS = frozenset(int(v) for v in settings["tattnskip"].split("+") if v) if "tattnskip" in settings else default_tattn[1]
        attention.SATTN_MXFP8 = settings["sattn"] != "0" if "sattn" in settings else default_sattn[0]
        attention.SATTN_MXFP8_SKIP_DIMS = frozenset(int(v) for v in settings["sattnskip"].split("+") if v) if "sattnskip" in settings else default_sattn[1]
        attention.SATTN_KV_POOL = attention._parse_kv_pool(settings["kvpool"]) if "kvpool" in settings else default_kvpool[0]
        attention.SATTN_KV_POOL_MIN_TOKENS = int(settings["kvpoolmin"]) if "kvpoolmin" in settings else default_kvpool[1]

    def run(settings, steps, profile):
        apply(settings)
        torch.manual_seed(7)                         # the eta = 1 noise of every run is the same draw
        x = x0.clone()
        interval = int(settings.get("fcache", "0"))
        fcache = FeatureCache(depth=int(settings.get("fcdepth", "0"))) if interval >= 2 else None
        with torch.no_grad():
            x = one_step(x, 0, fcache, interval)     # packs / caches of this variant (and the feature cache's first full forward)
            torch.cuda.synchronize()
            if profile:
                ops.profile_begin(1 << 16)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(1, 1 + steps):
                x = one_step(x, i, fcache, interval)
            e1.record()
            torch.cuda.synchronize()
            prof = ops.profile_end() if profile else None
        assert torch.isfinite(x).all()
        return e0.elapsed_time(e1) / steps, prof, x

    finals = {}
    for name, st in variants:                        # warm-up of every variant
        run(st, 1, False)
    from tools.telemetry import Telemetry
    with Telemetry(device_index=0, period_s=0.05) as tm:
        for r in range(args.rounds):
            for name, st in variants:
                ms, prof, x = run(st, args.steps, True)
                fam = {k: round(v["ms"] / args.steps, 2) for k, v in prof.items()}
                print(f"round {r} {name:10s} {ms:8.2f} ms/step  {fam}  launches {sum(v['launches'] for v in prof.values()) // args.steps}", flush=True)
                finals[name] = x
    tel = tm.summary()
    print("telemetry over the rounds: " + ", ".join(f"{k} {v}" for k, v in tel.items() if k in ("sclk_mhz", "power_w", "source", "samples")), flush=True)
    names = list(finals)
    for n in names[1:]:
        a, b = finals[names[0]].float(), finals[n].float()
        print(f"latent after {1 + args.steps} steps: {n} vs {names[0]}: rel-L2 {float((a - b).norm() / b.norm()):.3e}")


if __name__ == "__main__":
    main()
