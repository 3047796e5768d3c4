"""rel-L2 / PSNR against the fp32 oracle at the config-1 latent (16 x 40 x 64, inference_pvd_512.yaml, synthetic weights) with the MXFP8
switches - VCX_FF_MXFP8 (feed-forward), VCX_TCONV_MXFP8 (temporal convolutions), VCX_RESCONV_MXFP8 (ResBlock 3x3 convolutions),
VCX_TATTN_MXFP8 (temporal attention) and VCX_SATTN_MXFP8 (spatial attention) - off, alone and together: one UNet forward, and a 10-step DDIM trajectory (eta 0, CFG 7.5, guidance rescale 0.7) of the product sampler against
the oracle sampler on the oracle UNet.  The skip lists are as the environment sets them; --all-widths empties all five.  Figures for
profiles/mxfp8_ff.md, profiles/mxfp8_tconv.md, profiles/mxfp8_resconv.md, profiles/mxfp8_tattn.md and profiles/mxfp8_sattn.md; the last row
of the default table and --only-restail add VCX_RESCONV_MXFP8_TAIL (the skip convolution as a K tail; profiles/mxfp8_resconv_tail.md).
    python tools/mxfp8_accuracy.py [--steps 10] [--all-widths] [--only-tconv | --only-resconv | --only-tattn | --only-sattn | --only-restail]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"


def rel_l2(a, b):
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def psnr(a, b, peak=2.0):
    mse = float(((a.detach().double() - b.detach().double()) ** 2).mean())
    return 10 * torch.log10(torch.tensor(peak * peak / max(mse, 1e-30))).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--yaml", default="inference_pvd_512.yaml")
    ap.add_argument("--all-widths", action="store_true", help="empty FF_MXFP8_SKIP_DIMS, TCONV_MXFP8_SKIP_DIMS, RESCONV_MXFP8_SKIP_DIMS, TATTN_MXFP8_SKIP_DIMS and SATTN_MXFP8_SKIP_DIMS")
    ap.add_argument("--only-tconv", action="store_true", help="skip the feed-forward-only run (recorded in profiles/mxfp8_ff.md)")
    ap.add_argument("--only-resconv", action="store_true", help="all off, the ResBlock switch alone (under both KEEP_FOLD settings), all three switches on")
    ap.add_argument("--only-tattn", action="store_true", help="all off, the temporal-attention switch alone, all four switches on")
    ap.add_argument("--only-sattn", action="store_true", help="all off, the spatial-attention switch alone, all five switches on")
    ap.add_argument("--only-restail", action="store_true", help="all off, the ResBlock switch alone, the ResBlock switch with VCX_RESCONV_MXFP8_TAIL, all five switches "
                                                                "without and with it")
    a = ap.parse_args()
    from oracle import lvdm_oracle as O
    from viewcrafter_amd.builder import build_diffusion_model, randomize_parameters
    from viewcrafter_amd.config import load_yaml
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from viewcrafter_amd.lvdm.modules import attention as A
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    path = os.path.join(ROOT, "configs", a.yaml)
    model = build_diffusion_model(path, device=DEV, conditioners="identity")
    randomize_parameters(model, seed=0)
    params = load_yaml(path)["model"]["params"]
    unet = model.model.diffusion_model
    hp = dict(params["unet_config"]["params"])
    sd = {k: v.detach() for k, v in unet.state_dict().items()}
    T, h, w = 16, 40, 64
    g = torch.Generator().manual_seed(77)
    x = torch.randn(1, 8, T, h, w, generator=g).to(DEV)
    ctx = torch.randn(1, 77 + 256, 1024, generator=g).to(DEV)
    uctx = torch.randn(1, 77 + 256, 1024, generator=g).to(DEV)
    x_T = torch.randn(1, 4, T, h, w, generator=g).to(DEV)
    cat = (torch.randn(1, 4, T, h, w, generator=g) * 0.8).to(DEV)
    ts, fs = torch.tensor([799], device=DEV), torch.tensor([10], device=DEV)
    cond, uc = {"c_crossattn": [ctx], "c_concat": [cat]}, {"c_crossattn": [uctx], "c_concat": [cat]}
    tables = O.diffusion_tables(params["timesteps"], params["linear_start"], params["linear_end"], params["rescale_betas_zero_snr"])
    scale_arr = O.dynamic_rescale_table(params["timesteps"], params["base_scale"])

    def apply_oracle(xx, t, c):
        return O.unet_forward(sd, hp, torch.cat([xx, c["c_concat"][0]], dim=1), t.to(DEV), c["c_crossattn"][0], fs)

    was = A.FF_MXFP8, U.TCONV_MXFP8, A.FF_MXFP8_SKIP_DIMS, U.TCONV_MXFP8_SKIP_DIMS, U.RESCONV_MXFP8, U.RESCONV_MXFP8_SKIP_DIMS, U.RESCONV_MXFP8_KEEP_FOLD
    was_tattn = A.TATTN_MXFP8, A.TATTN_MXFP8_SKIP_DIMS
    was_sattn = A.SATTN_MXFP8, A.SATTN_MXFP8_SKIP_DIMS
    was_tail = U.RESCONV_MXFP8_TAIL
    if a.all_widths:
        A.FF_MXFP8_SKIP_DIMS = U.TCONV_MXFP8_SKIP_DIMS = U.RESCONV_MXFP8_SKIP_DIMS = A.TATTN_MXFP8_SKIP_DIMS = A.SATTN_MXFP8_SKIP_DIMS = frozenset()
    print(f"skip lists: feed-forward {sorted(A.FF_MXFP8_SKIP_DIMS)}, temporal convolutions {sorted(U.TCONV_MXFP8_SKIP_DIMS)}, "
          f"ResBlock convolutions {sorted(U.RESCONV_MXFP8_SKIP_DIMS)}, temporal attention {sorted(A.TATTN_MXFP8_SKIP_DIMS)}, "
          f"spatial attention {sorted(A.SATTN_MXFP8_SKIP_DIMS)}", flush=True)
    # (feed-forward, temporal convolutions, ResBlock convolutions, KEEP_FOLD or None = as set, temporal attention[, spatial attention[, the
    # skip convolution as a K tail]])
    if a.only_restail:
        rows = [(False, False, False, None, False, False, False), (False, False, True, False, False, False, False), (False, False, True, False, False, False, True),
                (True, True, True, False, True, True, False), (True, True, True, False, True, True, True)]
    elif a.only_sattn:
        rows = [(False, False, False, None, False, False), (False, False, False, None, False, True), (True, True, True, None, True, True)]
    elif a.only_tattn:
        rows = [(False, False, False, None, False), (False, False, False, None, True), (True, True, True, None, True)]
    elif a.only_resconv:
        rows = [(False, False, False, None, False), (False, False, True, True, False), (False, False, True, False, False), (True, True, True, None, False)]
    else:
        rows = [(ff, tconv, False, None, False) for ff, tconv in ((False, False), (True, False), (False, True), (True, True)) if not (a.only_tconv and ff and not tconv)]
        rows += [(False, False, True, None, False), (True, True, True, None, False), (False, False, False, None, True), (True, True, True, None, True)]
        rows += [(False, False, True, False, False, False, True)]
    try:
        with torch.no_grad():
            ref_fwd = O.unet_forward(sd, hp, x, ts, ctx, fs)
            ref_traj, _ = O.ddim_sample(apply_oracle, tables, scale_arr, x_T, cond, uc, steps=a.steps, eta=0.0, cfg_scale=7.5, guidance_rescale=0.7,
                                        spacing="uniform_trailing", parameterization="v")
            for ff, tconv, resconv, keep, tattn, *rest in rows:
                sattn, tail = bool(rest and rest[0]), bool(len(rest) > 1 and rest[1])
                U.RESCONV_MXFP8_TAIL = tail
                A.FF_MXFP8, U.TCONV_MXFP8, U.RESCONV_MXFP8, A.TATTN_MXFP8, A.SATTN_MXFP8 = ff, tconv, resconv, tattn, sattn
                U.RESCONV_MXFP8_KEEP_FOLD = was[6] if keep is None else keep
                y = unet._forward(x, ts, context=ctx, fs=fs)
                ours, _ = DDIMSampler(model).sample(S=a.steps, conditioning=cond, batch_size=1, shape=[4, T, h, w], verbose=False,
                                                    unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=0.0, cfg_img=None, mask=None,
                                                    x0=None, fs=fs, timestep_spacing="uniform_trailing", guidance_rescale=0.7, x_T=x_T,
                                                    log_every_t=a.steps, unconditional_conditioning_img_nonetext=None)
                print(f"VCX_FF_MXFP8={int(ff)} VCX_TCONV_MXFP8={int(tconv)} VCX_RESCONV_MXFP8={int(resconv)}" + (f" (KEEP_FOLD={int(U.RESCONV_MXFP8_KEEP_FOLD)}, TAIL={int(tail)})" if resconv else "") + f" VCX_TATTN_MXFP8={int(tattn)} VCX_SATTN_MXFP8={int(sattn)}: UNet forward vs fp32 oracle rel-L2 {rel_l2(y, ref_fwd):.3e} PSNR {psnr(y, ref_fwd):.2f} dB | "
                      f"{a.steps}-step trajectory, final latent rel-L2 {rel_l2(ours, ref_traj):.3e} PSNR {psnr(ours, ref_traj):.2f} dB", flush=True)
    finally:
        A.FF_MXFP8, U.TCONV_MXFP8, A.FF_MXFP8_SKIP_DIMS, U.TCONV_MXFP8_SKIP_DIMS, U.RESCONV_MXFP8, U.RESCONV_MXFP8_SKIP_DIMS, U.RESCONV_MXFP8_KEEP_FOLD = was
        A.TATTN_MXFP8, A.TATTN_MXFP8_SKIP_DIMS = was_tattn
        A.SATTN_MXFP8, A.SATTN_MXFP8_SKIP_DIMS = was_sattn
        U.RESCONV_MXFP8_TAIL = was_tail


if __name__ == "__main__":
    main()
