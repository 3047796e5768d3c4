"""The feature cache (VCX_FEATURE_CACHE / VCX_FEATURE_CACHE_DEPTH, viewcrafter_amd/feature_cache.py) on one box, synthetic weights: what a
full and a shallow step cost, what a video costs at N in {2, 3, 5}, and how far the cached latent is from the uncached one.

    python tools/feature_cache_ab.py [--out profiles/feature_cache.md] [--rounds 3] [--steps 50] [--converged 200] [--parts steps,videos,accuracy]

  steps     576 x 1024 x 25: ms of one DDIM step (the benchmark's step: shared CFG prefix + update kernel) - plain (no cache object: the
            parent commit's launch sequence; this change does not touch the library, so the same build serves both), full with a cache
            object, shallow at d in {0, 1, 2} - interleaved round by round in one process, graphics clock and socket power beside every
            number (tools/telemetry.py);
  videos    whole sample() calls of --steps steps, 576 x 1024 x 25 and 320 x 512 x 16, eager and graph replay, cache off and N in {2, 3, 5}
            at d = 0, and one line VCX_SAMPLER=dpmpp2m with 20 steps;
  accuracy  320 x 512 x 16, eta 0, one fixed x_T: final-latent rel-L2 of every (N, d) against the uncached run of the same step count and
            against DDIM-<converged> (the table of profiles/dpmpp2m.md).  INDICATIVE ONLY: synthetic weights say nothing about a checkpoint.
Writes the markdown tables to --out (and prints them)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"576x1024x25": ("inference_pvd_1024.yaml", 25, 72, 128), "320x512x16": ("inference_pvd_512.yaml", 16, 40, 64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_cache.md"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--converged", type=int, default=200)
    ap.add_argument("--parts", default="steps,videos,accuracy")
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    from bench import synth_conditioning
    from tools.telemetry import Telemetry
    from viewcrafter_amd import ops
    from viewcrafter_amd.builder import build_diffusion_model, randomize_parameters
    from viewcrafter_amd.feature_cache import FeatureCache
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    ops.require_gpu()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def load(size):
        cfg, T, h, w = SIZES[size]
        torch.manual_seed(123)
        model = build_diffusion_model(os.path.join(ROOT, "configs", cfg), device="cuda", conditioners="identity")
        randomize_parameters(model, seed=0)
        return model, (T, h, w), synth_conditioning(T, h, w, "cuda", seed=123)

    def timed(fn):
        """(result, ms, 'sclk MHz / W') of fn() between two HIP events, with the telemetry of the region"""
        tm = Telemetry(period_s=0.02)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with tm:
            t0 = time.perf_counter()
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            s = tm.summary(t0, time.perf_counter())
        clk, pw = (s.get("sclk_mhz") or {}).get("mean"), (s.get("power_w") or {}).get("mean")
        return out, e0.elapsed_time(e1), f"{clk if clk is not None else '?'} MHz / {pw if pw is not None else '?'} W"

    def sample(model, thw, inputs, S, env, sampler="ddim", graph=False):
        T, h, w = thw
        x_T, cond, uc = inputs
        for k in ("VCX_FEATURE_CACHE", "VCX_FEATURE_CACHE_DEPTH"):
            os.environ.pop(k, None)
        os.environ.update(env)
        os.environ["VCX_SAMPLER"] = sampler
        unet = model.model.diffusion_model
        unet.use_hip_graph = graph

        def go():
            with torch.no_grad():
                return DDIMSampler(model).sample(S=S, conditioning=cond, batch_size=1, shape=[4, T, h, w], verbose=False,
                                                 unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=0.0,
                                                 fs=torch.tensor([10], device="cuda"), timestep_spacing="uniform_trailing", guidance_rescale=0.7,
                                                 x_T=x_T.clone(), cfg_img=None, unconditional_conditioning_img_nonetext=None)[0]
        try:
            out, ms, tele = timed(go)
        finally:
            unet.use_hip_graph = False
        assert torch.isfinite(out).all(), env
        return out, ms, tele

    say("# Feature cache (`VCX_FEATURE_CACHE`): what was measured, and what was not")
    say()
    say("Written by `tools/feature_cache_ab.py`.  One MI355X, one box, **synthetic weights** (`randomize_parameters(seed=0)`), CFG 7.5 through the")
    say("shared prefix, guidance rescale 0.7, `uniform_trailing`.  Nothing here says anything about a trained checkpoint or about video quality.")

    if "steps" in parts:
        model, thw, (x0, cond, uc) = load("576x1024x25")
        sampler = DDIMSampler(model)
        sampler.make_schedule(ddim_num_steps=50, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
        fs = torch.tensor([10], device="cuda")
        K = 3

        def step(x, i, **kw):
            index = 49 - (i % 50)
            ts = torch.full((1,), int(sampler.ddim_timesteps[index]), device="cuda", dtype=torch.long)
            return sampler.p_sample_ddim(x, cond, ts, index=index, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, fs=fs,
                                         guidance_rescale=0.7, cfg_img=None, unconditional_conditioning_img_nonetext=None, **kw)[0]

        def run(kind, depth):
            torch.manual_seed(7)
            with torch.no_grad():
                if kind == "plain":
                    return timed(lambda: [step(x0, i) for i in range(K)][-1])
                fc = FeatureCache(depth=depth)
                if kind == "full":
                    return timed(lambda: [step(x0, i, feature_cache=fc) for i in range(K)][-1])
                step(x0, 0, feature_cache=fc)
                fc.set_mode("shallow")
                return timed(lambda: [step(x0, i, feature_cache=fc) for i in range(1, 1 + K)][-1])
        variants = [("plain (no cache object)", "plain", 0), ("full, cache on (d = 0)", "full", 0), ("shallow d = 0", "shallow", 0),
                    ("shallow d = 1", "shallow", 1), ("shallow d = 2", "shallow", 2)]
        for _, kind, d in variants:
            run(kind, d)
        say()
        say(f"## 1. One step, 576 x 1024 x 25 (ms per step over {K} steps; graphics clock / socket power of the region)")
        say()
        say("| round | " + " | ".join(n for n, _, _ in variants) + " |")
        say("|---|" + "---|" * len(variants))
        for r in range(args.rounds):
            cells = []
            for _, kind, d in variants:
                _, ms, tele = run(kind, d)
                cells.append(f"{ms / K:.2f} ({tele})")
            say(f"| {r} | " + " | ".join(cells) + " |")
        model.model.diffusion_model.drop_feature_cache()
        del model, sampler
        torch.cuda.empty_cache()

    if "videos" in parts:
        say()
        say(f"## 2. One `sample()` call of {args.steps} steps (eta 0), d = 0: s per call, ms per step averaged over the call")
        for size in SIZES:
            model, thw, inputs = load(size)
            configs = [("off", {})] + [(f"N = {n}", {"VCX_FEATURE_CACHE": str(n)}) for n in (2, 3, 5)]
            say()
            say(f"### {size}")
            say()
            say("The graph-replay rows include the captures: a `sample()` call stacks its conditionings anew, a graph is keyed on that tensor, so every")
            say("call captures its own (one per mode and slot) - as in production, where a call is a video.")
            say()
            say("| cache | route | s per call | ms per step | clock / power |")
            say("|---|---|---|---|---|")
            for graph in (False, True):
                for name, env in configs:
                    sample(model, thw, inputs, 2 * max(int(env.get("VCX_FEATURE_CACHE", 1)), 1), env, graph=graph)       # packs, captures
                    _, ms, tele = sample(model, thw, inputs, args.steps, env, graph=graph)
                    say(f"| {name} | {'graph replay' if graph else 'eager'} | {ms / 1e3:.3f} | {ms / args.steps:.2f} | {tele} |")
            if size == "576x1024x25":
                for name, env in (("off", {}), ("N = 3", {"VCX_FEATURE_CACHE": "3"})):
                    sample(model, thw, inputs, 6, env, sampler="dpmpp2m")
                    _, ms, tele = sample(model, thw, inputs, 20, env, sampler="dpmpp2m")
                    say(f"| {name}, `VCX_SAMPLER=dpmpp2m`, 20 steps | eager | {ms / 1e3:.3f} | {ms / 20:.2f} | {tele} |")
            model.model.diffusion_model.drop_feature_cache()
            del model
            torch.cuda.empty_cache()

    if "accuracy" in parts:
        model, thw, inputs = load("320x512x16")
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
        base, _, _ = sample(model, thw, inputs, args.steps, {})
        conv, _, _ = sample(model, thw, inputs, args.converged, {})
        say()
        say(f"## 3. Final latent, 320 x 512 x 16, DDIM eta 0, {args.steps} steps - INDICATIVE ONLY (synthetic weights)")
        say()
        say(f"The uncached {args.steps}-step run is {rel(base, conv):.3e} from DDIM-{args.converged} (the row to read the last column against).")
        say()
        say(f"| N | d | rel-L2 vs the uncached {args.steps}-step run | rel-L2 vs DDIM-{args.converged} |")
        say("|---|---|---|---|")
        for n in (2, 3, 5):
            for d in (0, 1, 2):
                out, _, _ = sample(model, thw, inputs, args.steps, {"VCX_FEATURE_CACHE": str(n), "VCX_FEATURE_CACHE_DEPTH": str(d)})
                say(f"| {n} | {d} | {rel(out, base):.3e} | {rel(out, conv):.3e} |")
        out, _, _ = sample(model, thw, inputs, 20, {"VCX_FEATURE_CACHE": "3"}, sampler="dpmpp2m")
        ref20, _, _ = sample(model, thw, inputs, 20, {}, sampler="dpmpp2m")
        say()
        say(f"`VCX_SAMPLER=dpmpp2m`, 20 steps, N = 3, d = 0: {rel(out, ref20):.3e} from the uncached 20-step solver run, {rel(out, conv):.3e} from DDIM-{args.converged} "
            f"(uncached: {rel(ref20, conv):.3e}).")

    say()
    say("## Not measured")
    say()
    say("* **A real checkpoint** and **video quality**: no trained weights are available to this repository.  DeepCache's premise - deep features")
    say("  change slowly between steps - is a property of a trained denoiser; section 3 shows how this randomly initialised one behaves, no more.")
    say("* Multi-GPU runs (`VCX_GUIDANCE_PARALLEL`), `VCX_CLIPS_PER_GPU=2` and `VCX_CLIP_BATCH` with the cache: tested for bits, not timed.")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
