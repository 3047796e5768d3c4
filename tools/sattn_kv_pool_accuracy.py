"""rel-L2 / PSNR against the PLAIN fp32 oracle (un-pooled attention) with VCX_SATTN_KV_POOL off, mean and nearest at two thresholds
(VCX_SATTN_KV_POOL_MIN_TOKENS 4096 / 2048), on synthetic weights: one UNet forward, and a 10-step DDIM trajectory (eta 0, CFG 7.5, guidance
rescale 0.7) of the product sampler against the oracle sampler on the oracle UNet - tools/mxfp8_accuracy.py's measurement for this switch.
Two inputs: the usual white-noise latent, and a spatially smooth one - the same noise low-passed 4x (4 x 4 box mean, bilinear back up,
rescaled to unit variance) - because neighbouring tokens that are uncorrelated are the opposite of the regime token pooling is for.
What the figures are the error OF: the approximation itself (the pooled attention is another function than the oracle's), not kernel
rounding; the pooled route against its own fp32 reference is tests/test_sattn_kv_pool_gpu.py.  Figures for profiles/sattn_kv_pool.md.

    python tools/sattn_kv_pool_accuracy.py [--steps 10] [--yaml inference_pvd_1024.yaml] [--frames 4] [--height 72] [--width 128]

Default latent 4 x 72 x 128 (576x1024, four frames: the oracle's 9216-key attention in fp32 is what bounds the frame count): 4096 pools level
0, 2048 levels 0 and 1.  At 16 x 40 x 64 (--yaml inference_pvd_512.yaml --frames 16 --height 40 --width 64) 4096 pools nothing, 2048 level 0."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"


def rel_l2(a, b):
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def psnr(a, b, peak=2.0):
    mse = float(((a.detach().double() - b.detach().double()) ** 2).mean())
    return 10 * torch.log10(torch.tensor(peak * peak / max(mse, 1e-30))).item()


def low_pass(x, f=4):
    """[b, c, t, h, w]: box mean over f x f pixels, bilinear back to h x w, rescaled to the variance it had"""
    b, c, t, h, w = x.shape
    y = x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
    y = F.interpolate(F.avg_pool2d(y, f, f), size=(h, w), mode="bilinear", align_corners=False)
    y = y * (x.std() / y.std())
    return y.view(b, t, c, h, w).permute(0, 2, 1, 3, 4).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--yaml", default="inference_pvd_1024.yaml")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--height", type=int, default=72)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--thresholds", default="4096,2048")
    a = ap.parse_args()
    from oracle import lvdm_oracle as O
    from viewcrafter_amd.builder import build_diffusion_model, randomize_parameters
    from viewcrafter_amd.config import load_yaml
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from viewcrafter_amd.lvdm.modules import attention as A
    path = os.path.join(ROOT, "configs", a.yaml)
    model = build_diffusion_model(path, device=DEV, conditioners="identity")
    randomize_parameters(model, seed=0)
    params = load_yaml(path)["model"]["params"]
    unet = model.model.diffusion_model
    hp = dict(params["unet_config"]["params"])
    sd = {k: v.detach() for k, v in unet.state_dict().items()}
    T, h, w = a.frames, a.height, a.width
    g = torch.Generator().manual_seed(77)
    white = dict(x=torch.randn(1, 8, T, h, w, generator=g).to(DEV), x_T=torch.randn(1, 4, T, h, w, generator=g).to(DEV),
                 cat=(torch.randn(1, 4, T, h, w, generator=g) * 0.8).to(DEV))
    smooth = {k: low_pass(v) for k, v in white.items()}
    ctx = torch.randn(1, 77 + 16 * T, 1024, generator=g).to(DEV)
    uctx = torch.randn(1, 77 + 16 * T, 1024, generator=g).to(DEV)
    ts, fs = torch.tensor([799], device=DEV), torch.tensor([10], device=DEV)
    tables = O.diffusion_tables(params["timesteps"], params["linear_start"], params["linear_end"], params["rescale_betas_zero_snr"])
    scale_arr = O.dynamic_rescale_table(params["timesteps"], params["base_scale"])

    def apply_oracle(xx, t, c):
        return O.unet_forward(sd, hp, torch.cat([xx, c["c_concat"][0]], dim=1), t.to(DEV), c["c_crossattn"][0], fs)

    was = A.SATTN_KV_POOL, A.SATTN_KV_POOL_MIN_TOKENS
    levels = [(h >> l, w >> l, 320 << min(l, 2)) for l in range(4)]
    rows = [(None, was[1])] + [(m, int(v)) for v in a.thresholds.split(",") if v for m in ("mean", "nearest")]
    print(f"latent {T} x {h} x {w}, {a.yaml}, {a.steps} steps; tokens a frame per level: {[hh * ww for hh, ww, _ in levels]}", flush=True)
    try:
        with torch.no_grad():
            for name, inp in (("white noise", white), ("low-passed 4x", smooth)):
                cond, uc = {"c_crossattn": [ctx], "c_concat": [inp["cat"]]}, {"c_crossattn": [uctx], "c_concat": [inp["cat"]]}
                A.SATTN_KV_POOL = None
                ref_fwd = O.unet_forward(sd, hp, inp["x"], ts, ctx, fs)
                ref_traj, _ = O.ddim_sample(apply_oracle, tables, scale_arr, inp["x_T"], cond, uc, steps=a.steps, eta=0.0, cfg_scale=7.5, guidance_rescale=0.7,
                                            spacing="uniform_trailing", parameterization="v")
                for mode, thr in rows:
                    A.SATTN_KV_POOL, A.SATTN_KV_POOL_MIN_TOKENS = mode, thr
                    pooled = [i for i, (hh, ww, c) in enumerate(levels) if A.kv_pool_plan(hh, ww, c) is not None]
                    y = unet._forward(inp["x"], ts, context=ctx, fs=fs)
                    ours, _ = DDIMSampler(model).sample(S=a.steps, conditioning=cond, batch_size=1, shape=[4, T, h, w], verbose=False,
                                                        unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=0.0, cfg_img=None, mask=None,
                                                        x0=None, fs=fs, timestep_spacing="uniform_trailing", guidance_rescale=0.7, x_T=inp["x_T"],
                                                        log_every_t=a.steps, unconditional_conditioning_img_nonetext=None)
                    print(f"{name} | VCX_SATTN_KV_POOL={mode or 0} MIN_TOKENS={thr} (levels pooled: {pooled}) | UNet forward vs plain fp32 oracle rel-L2 "
                          f"{rel_l2(y, ref_fwd):.3e} PSNR {psnr(y, ref_fwd):.2f} dB | {a.steps}-step trajectory, final latent rel-L2 {rel_l2(ours, ref_traj):.3e} "
                          f"PSNR {psnr(ours, ref_traj):.2f} dB", flush=True)
    finally:
        A.SATTN_KV_POOL, A.SATTN_KV_POOL_MIN_TOKENS = was


if __name__ == "__main__":
    main()
