"""Several clips per GPU: aggregate DDIM steps/s of three ways to run them on one box (VCX_CLIP_BATCH, viewcrafter_amd/clip_batch.py).

    python tools/clip_batch_ab.py [--workload ViewCrafter_25_576x1024x25] [--rounds 3] [--steps 3] [--ks 2,3]
    python tools/clip_batch_ab.py --one-step K      # one warm-up and one timed step at k = K only (for rocprofv3 --kernel-trace --stats)

Modes, each a DDIM step of the product sampler (DDIMSampler.p_sample_ddim: one CFG forward with the shared prefix + the fused update,
eta = 1, guidance rescale 0.7) on synthetic weights and conditioning:
  sequential    one clip after the other (B = 1, 2 videos per forward)
  two streams   two clips step by step on two HIP streams (VCX_CLIPS_PER_GPU=2, interleave.py)
  batched k     k clips stacked on the batch axis, one forward of 2k videos (VCX_CLIP_BATCH=k); k above the workload's 32-bit extent
                cap (clip_batch.max_clips_per_forward) is skipped
Prints clip-steps per second (median of interleaved rounds) and the clock / power the telemetry sampled during each mode."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ViewCrafter_25_576x1024x25")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="DDIM steps per clip in one timed run")
    ap.add_argument("--ks", default="2,3")
    ap.add_argument("--one-step", type=int, default=0)
    args = ap.parse_args()
    from bench import WORKLOADS, synth_conditioning
    from tools.telemetry import Telemetry
    from viewcrafter_amd import clip_batch
    from viewcrafter_amd.builder import build_diffusion_model, randomize_parameters
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    cfg, T, h, w = WORKLOADS[args.workload]
    model = build_diffusion_model(os.path.join(ROOT, "configs", cfg), device="cuda", conditioners="identity")
    randomize_parameters(model)
    cap = clip_batch.max_clips_per_forward(model.model.diffusion_model, [1, 4, T, h, w], 2)
    ks = [args.one_step] if args.one_step else [k for k in (int(s) for s in args.ks.split(",")) if k <= cap]
    n_clips = max(ks + [2])
    clips = [synth_conditioning(T, h, w, "cuda", seed=123 + i) for i in range(n_clips)]

    def stacked(n):
        x = torch.cat([c[0] for c in clips[:n]])
        cat = torch.cat([c[1]["c_concat"][0] for c in clips[:n]])
        cond = {"c_crossattn": [torch.cat([c[1]["c_crossattn"][0] for c in clips[:n]])], "c_concat": [cat]}
        uc = {"c_crossattn": [torch.cat([c[2]["c_crossattn"][0] for c in clips[:n]])], "c_concat": [cat]}
        return x, cond, uc

    def sampler():
        s = DDIMSampler(model)
        s.make_schedule(ddim_num_steps=50, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
        return s

    def step(s, x, cond, uc, index=25):
        t = torch.full((x.shape[0],), int(s.ddim_timesteps[index]), device="cuda", dtype=torch.long)
        fs = torch.full((x.shape[0],), 10, device="cuda", dtype=torch.long)
        return s.p_sample_ddim(x, cond, t, index=index, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, fs=fs,
                               guidance_rescale=0.7)[0]

    runs = {}
    one = [(sampler(),) + stacked_one for stacked_one in ((c[0], c[1], c[2]) for c in clips)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def run_sequential():
        for s, x, c, u in one[:1]:
            for _ in range(args.steps):
                x = step(s, x, c, u)
        return args.steps

    def run_two_streams():
        xs = [one[0][1], one[1][1]]
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
        for _ in range(args.steps):
            for j in range(2):
                with torch.cuda.stream(streams[j]):
                    xs[j] = step(one[j][0], xs[j], one[j][2], one[j][3])
        for st in streams:
            torch.cuda.current_stream().wait_stream(st)
        return 2 * args.steps

    def run_batched(k):
        s, (x, c, u) = sampler(), stacked(k)

        def go():
            y = x
            for _ in range(args.steps):
                y = step(s, y, c, u)
            return k * args.steps
        return go

    if args.one_step:
        go = run_batched(args.one_step)
        with torch.no_grad():
            args.steps = 1
            go()                    # warm-up: weight packs, context K / V
            torch.cuda.synchronize()
            go()
            torch.cuda.synchronize()
        print(f"{args.workload}: one warm-up and one DDIM step at k = {args.one_step} done")
        return
    runs["sequential"] = run_sequential
    runs["two streams"] = run_two_streams
    for k in ks:
        runs[f"batched k={k}"] = run_batched(k)
    rates = {name: [] for name in runs}
    tele = {name: [] for name in runs}
    with torch.no_grad():
        for fn in runs.values():        # warm every mode once
            fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                with Telemetry(device_index=torch.cuda.current_device(), period_s=0.05) as tm:
                    e0.record()
                    n = fn()
                    e1.record()
                    torch.cuda.synchronize()
                rates[name].append(n / (e0.elapsed_time(e1) / 1e3))
                tele[name].append(tm.summary())
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    print(f"{args.workload}: aggregate clip-steps/s (DDIM step = CFG forward + update), {args.rounds} interleaved rounds of "
          f"{args.steps} steps per clip; extent cap k <= {cap}")
    print(f"| mode | clip-steps/s (median) | vs sequential | all rounds | sclk MHz (mean) | power W (mean) |")
    print("|---|---|---|---|---|---|")
    for name in runs:
        t = [s for s in tele[name] if s.get("source")]
        sclk = [s["sclk_mhz"]["mean"] for s in t if s.get("sclk_mhz")]
        pw = [s["power_w"]["mean"] for s in t if s.get("power_w")]
        sclk_s = f"{sum(sclk) / len(sclk):.0f}" if sclk else "n/a"
        pw_s = f"{sum(pw) / len(pw):.0f}" if pw else "n/a"
        print(f"| {name} | {med[name]:.3f} | {med[name] / med['sequential']:.3f} | {[round(r, 3) for r in rates[name]]} | {sclk_s} | {pw_s} |")


if __name__ == "__main__":
    main()
