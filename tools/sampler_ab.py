"""DDIM against DPM-Solver++(2M) (VCX_SAMPLER=dpmpp2m) on one box, synthetic weights: how far the final latent of a short run is from
the converged solution, and what a step costs under either sampler.

    python tools/sampler_ab.py [--rounds 3] [--timing-steps 20] [--converged 200]

Setting: configs/inference_pvd_512.yaml, latent 16 x 40 x 64 (320 x 512, 16 frames), CFG 7.5, guidance rescale 0.7, eta 0,
uniform_trailing, one fixed x_T.  Prints
  * the final-latent rel-L2 of DDIM-{20,25,50} and 2M-{15,20,25} against DDIM-<converged> (both samplers integrate the same ODE,
    so the long DDIM run stands for its solution), and 2M-<converged> against it as a consistency check;
  * ms per step of both samplers from interleaved rounds (one whole sample() call of --timing-steps steps per sampler and round).
Synthetic weights: the numbers say how the solvers behave on THIS denoiser, not what a trained checkpoint gives."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timing-steps", type=int, default=20)
    ap.add_argument("--converged", type=int, default=200)
    args = ap.parse_args()
    from bench import synth_conditioning
    from viewcrafter_amd import ops
    from viewcrafter_amd.builder import build_diffusion_model, randomize_parameters
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    ops.require_gpu()
    T, h, w = 16, 40, 64
    torch.manual_seed(123)
    model = build_diffusion_model(os.path.join(ROOT, "configs", "inference_pvd_512.yaml"), device="cuda", conditioners="identity")
    randomize_parameters(model, seed=0)
    x_T, cond, uc = synth_conditioning(T, h, w, "cuda", seed=123)
    fs = torch.tensor([10], device="cuda")

    def sample(name, S):
        os.environ["VCX_SAMPLER"] = name
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            e0.record()
            out, _ = DDIMSampler(model).sample(S=S, conditioning=cond, batch_size=1, shape=[4, T, h, w], verbose=False,
                                               unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=0.0, fs=fs,
                                               timestep_spacing="uniform_trailing", guidance_rescale=0.7, x_T=x_T.clone(),
                                               cfg_img=None, unconditional_conditioning_img_nonetext=None)
            e1.record()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), (name, S)
        return out, e0.elapsed_time(e1) / S

    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    sample("ddim", 2)                                                    # packs, caches
    sample("dpmpp2m", 3)
    ref, _ = sample("ddim", args.converged)
    print(f"final latent, rel-L2 against DDIM-{args.converged} (latent {T}x{h}x{w}, CFG 7.5, rescale 0.7, eta 0, uniform_trailing)")
    print("| sampler | steps | rel-L2 |\n|---|---|---|")
    for name, steps in (("ddim", (20, 25, 50)), ("dpmpp2m", (15, 20, 25, args.converged))):
        for S in steps:
            out, _ = sample(name, S)
            print(f"| {name} | {S} | {rel(out, ref):.3e} |", flush=True)
    print(f"\nms per step, {args.rounds} interleaved rounds of one {args.timing_steps}-step sample() call per sampler")
    print("| round | ddim | dpmpp2m |\n|---|---|---|")
    for r in range(args.rounds):
        ms = {name: sample(name, args.timing_steps)[1] for name in ("ddim", "dpmpp2m")}
        print(f"| {r} | {ms['ddim']:.2f} | {ms['dpmpp2m']:.2f} |", flush=True)


if __name__ == "__main__":
    main()
