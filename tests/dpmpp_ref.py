"""DPM-Solver++(2M) in fp64 torch, restated from the formulas (arXiv 2211.01095, data-prediction multistep form) - the yardstick of
tests/test_dpmpp2m_cpu.py and tests/test_dpmpp2m_gpu.py.  Written in the lambda / expm1 form, independently of the product, which
writes the first-order part as the DDIM step and precomputes one coefficient (utils_diffusion.dpmpp2m_coefficients).

Marginal: x_t = A x0 + b eps with A = s a, a = sqrt(alpha_cumprod), b = sqrt(1 - alpha_cumprod), s = the dynamic-rescale factor;
lambda = log(A / b).  One step from (A, b, lambda) to (A_p, b_p, lambda_p), h = lambda_p - lambda:
    first order :  x_p = (b_p / b) x - A_p expm1(-h) D
    second order:  x_p = (b_p / b) x - A_p expm1(-h) (D + (D - D_last) / (2 r)),   r = (lambda - lambda_last) / h
with D = x0 / s the data prediction in true units.  Limits: a = 0 (zero terminal SNR) gives lambda = -inf, h = +inf and
expm1(-h) = -1 exactly, so the first-order step needs no special case; a step whose lambda_last is -inf would have r = inf and is
first order by definition, as are the first step taken (no history) and the last one (index 0).
"""
import math

import torch

F64 = torch.float64


def tables(alphas, alphas_prev, scale=None, scale_prev=None):
    """Per DDIM index: dict of fp64 tensors a, b, s, A, lam and their *_p counterparts (from alphas_prev / scale_prev)."""
    al, al_p = torch.as_tensor(alphas, dtype=F64), torch.as_tensor(alphas_prev, dtype=F64)
    s = torch.ones_like(al) if scale is None else torch.as_tensor(scale, dtype=F64)
    s_p = torch.ones_like(al) if scale_prev is None else torch.as_tensor(scale_prev, dtype=F64)
    t = dict(a=al.sqrt(), b=(1 - al).sqrt(), s=s, a_p=al_p.sqrt(), b_p=(1 - al_p).sqrt(), s_p=s_p)
    t["A"], t["A_p"] = t["s"] * t["a"], t["s_p"] * t["a_p"]
    t["lam"], t["lam_p"] = torch.log(t["A"]) - torch.log(t["b"]), torch.log(t["A_p"]) - torch.log(t["b_p"])      # log(0) = -inf
    return t


def step_ratio(t, i):
    """r of the step at index i, or None where the step is first order (first taken, lambda_last not finite, last)."""
    S = t["lam"].shape[0]
    if i == S - 1 or i == 0 or not math.isfinite(float(t["lam"][i + 1])):
        return None
    return float((t["lam"][i] - t["lam"][i + 1]) / (t["lam_p"][i] - t["lam"][i]))


def orders(t):
    return [1 if step_ratio(t, i) is None else 2 for i in range(t["lam"].shape[0])]


def history_coefficient(t, i):
    """What multiplies (D - D_last) in the second-order step: -A_p expm1(-h) / (2 r); 0 where the step is first order."""
    r = step_ratio(t, i)
    if r is None:
        return 0.0
    h = t["lam_p"][i] - t["lam"][i]
    return float(-t["A_p"][i] * torch.expm1(-h) / (2.0 * r))


def guided(v_cond, v_uncond, v_img, cfg, cfg_img, rescale):
    """CFG / three-way combine and guidance rescale (unbiased per-sample standard deviations), fp64."""
    vc = v_cond.to(F64)
    if v_uncond is None:
        return vc
    vu = v_uncond.to(F64)
    if v_img is None:
        v = vu + cfg * (vc - vu)
    else:
        vi = v_img.to(F64)
        v = vu + cfg_img * (vi - vu) + cfg * (vc - vi)
    if rescale > 0:
        dims = tuple(range(1, v.dim()))
        v = rescale * (v * (vc.std(dim=dims, keepdim=True) / v.std(dim=dims, keepdim=True))) + (1 - rescale) * v
    return v


def step(x, v_cond, v_uncond, v_img, d_last, *, a, b, s, A_p, b_p, s_p, r, cfg=1.0, cfg_img=0.0, rescale=0.0, is_v=True):
    """One solver step in fp64.  a, b: the pair the parameterisation reads (x0 = a x - b v | (x - b eps) / a); A_p = s_p a_p.
    r = None: first order (d_last unused).  Returns (x_prev, pred_x0 = x0 s_p / s, D = x0 / s)."""
    x = x.to(F64)
    v = guided(v_cond, v_uncond, v_img, cfg, cfg_img, rescale)
    x0 = a * x - b * v if is_v else (x - b * v) / a
    D = x0 / s
    lam = math.log(s * a / b) if a > 0 else -math.inf
    h = math.log(A_p / b_p) - lam
    phi = -A_p * math.expm1(-h)                                   # h = +inf: expm1 = -1, phi = A_p
    Dbar = D if r is None else D + (D - d_last.to(F64)) / (2.0 * r)
    return (b_p / b) * x + phi * Dbar, x0 * (s_p / s), D


def step_from_coef(x, v_cond, v_uncond, v_img, d_last, coef, cfg_img, inv_s, c_h):
    """step() on the inputs of one vcx_dpmpp2m_step_f32 call (include/vcx.h): coef = {sqrt_acp_t, sqrt_1m_acp_t, a_prev, 0, scale_ratio,
    cfg, guidance_rescale, is_v}, every number taken as the fp32 value the kernel receives.  r follows from c_h = phi / (2 r)."""
    f = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
    a, b, a_prev, ratio, cfg, resc, inv_s, c_h, cfg_img = (f(coef[0]), f(coef[1]), f(coef[2]), f(coef[4]), f(coef[5]), f(coef[6]), f(inv_s),
                                                          f(c_h), f(cfg_img))
    assert float(coef[3]) == 0.0
    s = 1.0 / inv_s
    s_p = ratio * s
    A_p, b_p = s_p * math.sqrt(a_prev), math.sqrt(1.0 - a_prev)
    r = None
    if c_h != 0.0:
        h = math.log(A_p / b_p) - math.log(s * a / b)
        r = -A_p * math.expm1(-h) / (2.0 * c_h)
    return step(x, v_cond, v_uncond, v_img, d_last, a=a, b=b, s=s, A_p=A_p, b_p=b_p, s_p=s_p, r=r, cfg=cfg, cfg_img=cfg_img,
                rescale=resc if v_uncond is not None else 0.0, is_v=coef[7] != 0.0)


def loop(denoise, x_T, alphas, alphas_prev, scale=None, scale_prev=None, ab=None, cfg=1.0, cfg_img=0.0, rescale=0.0, is_v=True,
         first_order=False):
    """The whole sampler: index S - 1 down to 0.  denoise(x fp64, index) -> (v_cond, v_uncond | None, v_img | None).  ab: per-index
    (a, b) the parameterisation reads where they are not sqrt(alphas) / sqrt(1 - alphas) bit for bit (the v-parameterisation reads
    the model's own fp32 tables).  first_order=True is DDIM at eta = 0.  Returns (x_0, [orders taken])."""
    t = tables(alphas, alphas_prev, scale, scale_prev)
    S = t["lam"].shape[0]
    x, d_last, taken = x_T.to(F64), None, []
    for i in range(S - 1, -1, -1):
        r = None if first_order else step_ratio(t, i)
        a, b = (float(t["a"][i]), float(t["b"][i])) if ab is None else (float(ab[i][0]), float(ab[i][1]))
        v_c, v_u, v_i = denoise(x, i)
        x, _, d_last = step(x, v_c, v_u, v_i, d_last, a=a, b=b, s=float(t["s"][i]), A_p=float(t["A_p"][i]), b_p=float(t["b_p"][i]),
                            s_p=float(t["s_p"][i]), r=r, cfg=cfg, cfg_img=cfg_img, rescale=rescale, is_v=is_v)
        taken.append(1 if r is None else 2)
    return x, taken
