"""Rounding quality: how far a kernel's fp16 output is from the exact result, measured against the ONE rounding it cannot avoid.

The references of tests/test_rounding_gpu.py and the checks of tests/test_rounding_cpu.py; imports no GPU code (every function runs on
whatever device its tensors live on).

    E = rms(out - ref) / rms(fp16(ref) - ref)                      (both in fp64, absolute errors, over all elements)

is 1 for a correctly rounded result.  One rounding after an fp32-level error d gives E^2 = 1 + 12 (d / ulp16)^2, so the bound of 1.05
allows d up to 0.09 fp16 ulp (about 700 fp32 ulps) - far beyond any fp32 summation order at K <= 2880 - while the mildest SECOND
rounding (a result rounded to fp16 before an addend of its own size is added and the sum rounded again) gives 1.34.  The rounding error
of a continuous value is uniform, so the sampling noise of E over n elements is 0.45 / sqrt(n): 0.25 % at the n >= 32768 every case has.

The reference is always the documented function (include/vcx.h) of the operands the kernel actually receives - the fp16 tensors as
stored, fp32 bias / statistics / colsum as given, the already rounded W' of the folded forms - evaluated in fp64; never another fp16
kernel, never the unfused pair where the fusion changes the function.
"""
import math

import torch
import torch.nn.functional as F

from tests import exact_inputs as X

E_BOUND = 1.05           # one-rounding kernels (derivation above); also the allowance of a kernel over its rounding-point model
MISMATCH_CAP = 0.10      # share of elements whose bits differ from fp16(ref): half of the mildest wrong behaviour (30 %), references sit at 0.03 - 0.5 %
E_MODEL_CAP = 1.45       # a rounding-point model (MODELS) itself must stay below this on the chosen inputs
N_MIN = 32768
F64 = torch.float64

RECORD = []              # (kernel, case, E, E_model or None, mismatch) of this process, in order: tools / the profile table read it


def _ulp16(mag64):
    """exact_inputs.f16_ulp on the tensor's own device."""
    return torch.exp2(torch.floor(torch.log2(mag64.clamp_min(2.0 ** -14))) - 10)


def rounding_stats(out_f16, ref_f64):
    """E, mismatch, worst, n of an fp16 output against the fp64 reference (any device; see the module docstring).
    worst: the largest |out - ref| in fp16 ulps of max(|ref|, rms(ref)) - per-element ulps of the reference itself would let the
    near-zero outputs of a cancellation dominate (8 'ulps' on a correct fp32 result)."""
    assert out_f16.dtype == torch.float16 and ref_f64.dtype == F64 and tuple(out_f16.shape) == tuple(ref_f64.shape)
    ref = ref_f64.to(out_f16.device)
    err = out_f16.double() - ref
    ideal = ref.half()
    den = float(((ideal.double() - ref) ** 2).mean().sqrt())
    num = float((err ** 2).mean().sqrt())
    rms = float((ref ** 2).mean().sqrt())
    ulps = err.abs() / _ulp16(ref.abs().clamp_min(rms))
    finite = bool(torch.isfinite(out_f16).all())
    return dict(E=num / den if den > 0 and finite else float("inf"), mismatch=float((out_f16 != ideal).double().mean()),
                worst=float(ulps.max()) if finite else float("inf"), n=out_f16.numel())


def _where_wrong(out_f16, ref_f64):
    """Where the elements sit that are more than one fp16 ulp of max(|ref|, rms) off (count, first index, row / column modulo the tile
    sizes - exact_inputs._where); falls back to the elements whose bits differ from fp16(ref)."""
    ref = ref_f64.to(out_f16.device)
    rms = float((ref ** 2).mean().sqrt())
    ulp = _ulp16(ref.abs().clamp_min(rms))
    bad = ~((out_f16.double() - ref).abs() <= ulp)
    what = "more than one ulp off"
    if not bool(bad.any()):
        bad, what = out_f16 != ref.half(), "bits differ from fp16(ref)"
    return f"{what}: {X._where(bad.cpu())}" if bool(bad.any()) else "no element differs"


def check_rounding(kernel, case, out_f16, ref_f64, e_model=None, bound=E_BOUND):
    """Print `kernel case E mismatch`, record it, and assert E <= bound (x E_model where the kernel has a rounding-point model) and
    mismatch <= MISMATCH_CAP (one-rounding kernels only: a model with rounded probabilities has no correctly rounded target)."""
    st = rounding_stats(out_f16, ref_f64)
    RECORD.append((kernel, case, st["E"], e_model, st["mismatch"]))
    print(f"\n[rounding] {kernel} {case} E {st['E']:.4f}" + (f" E_model {e_model:.4f}" if e_model is not None else "") +
          f" mismatch {100 * st['mismatch']:.2f} % worst {st['worst']:.2f} ulp n {st['n']}")
    assert st["n"] >= N_MIN, f"{kernel} {case}: {st['n']} outputs, the noise of E needs >= {N_MIN}"
    limit = bound * (e_model if e_model is not None else 1.0)
    assert st["E"] <= limit, (f"{kernel} {case}: excess-error ratio E = {st['E']:.4f} > {limit:.4f}" +
                              (f" (= {bound} x E_model {e_model:.4f})" if e_model is not None else " (one rounding of the fp64 result is 1.0)") +
                              f"; mismatch {100 * st['mismatch']:.2f} %, worst {st['worst']:.2f} ulp; {_where_wrong(out_f16, ref_f64)}")
    if e_model is None:
        assert st["mismatch"] <= MISMATCH_CAP, f"{kernel} {case}: {100 * st['mismatch']:.2f} % of the elements differ from fp16(ref) (E {st['E']:.4f}); {_where_wrong(out_f16, ref_f64)}"
    return st


def model_E(model_f64, ref_f64):
    """E of a rounding-point model: its last step is the output rounding, so it is an fp16-representable fp64 tensor."""
    return rounding_stats(model_f64.half(), ref_f64)["E"]


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=g) * scale


def h64(x):
    """fp64 of the fp16 rounding of x: one rounding point of a model."""
    return x.half().double()


# ------------------------------------------------------------------------------------------------------------------ linear layers
# N(0, 1) activations, N(0, 1 / K) weights: outputs of order one; bias / rowadd / residual of order one, so that they are rounded
# together with the sum.  M x N >= 32768 everywhere; rows: tiles + a ragged 37, columns: a tile + 8.
def lin(M, N, K, alpha=1.0, bias="n", rowadd_div=0, residual=True, knobs=None, seed=0):
    return dict(M=M, N=N, K=K, alpha=alpha, bias=bias, rowadd_div=rowadd_div, residual=residual, knobs=knobs or {}, seed=seed)


LINEAR_CASES = {
    # the register-staged kernel (knob GEMM_DMA = 0; K % 64 != 0 under the default knobs)
    "reg_k64": lin(293, 136, 64, knobs=dict(GEMM_DMA=0)),
    "reg_k320": lin(293, 136, 320, alpha=0.37, knobs=dict(GEMM_DMA=0), seed=1),
    "reg_k2880": lin(293, 136, 2880, knobs=dict(GEMM_DMA=0), seed=2),
    "reg_k72": lin(293, 136, 72, seed=3),
    # the epilogues on the tiled engine's automatic plan
    "plain": lin(293, 136, 320, bias=None, residual=False, seed=4),
    "alpha": lin(293, 136, 320, alpha=0.37, bias=None, residual=False, seed=5),
    "bias_n": lin(293, 136, 320, residual=False, seed=6),
    "bias_m": lin(293, 136, 320, bias="m", residual=False, seed=7),
    "rowadd": lin(300, 136, 320, bias=None, rowadd_div=100, residual=False, seed=8),
    "residual": lin(293, 136, 320, bias=None, seed=9),
    "bias_residual_k64": lin(293, 136, 64, seed=10),
    "bias_residual_k1280": lin(293, 136, 1280, seed=11),
    "bias_residual_k2880": lin(1024 - 37, 640, 2880, alpha=0.5, seed=12),
}
_CFG_K = (64, 320, 1280, 2880, 320, 1280)
for _cfg, (_tm, _tn) in X.TILE.items():          # the tiled engine under every forced configuration: two row tiles + 37 (more for the 64-row ones)
    _rows = 2 * _tm + 37 if _tm > 64 else (4 if _tn > 64 else 8) * _tm + 37
    LINEAR_CASES[f"cfg{_cfg}"] = lin(_rows, _tn + 8, _CFG_K[_cfg], alpha=(1.0, 0.5, 2.0)[_cfg % 3], knobs=dict(GEMM_CFG=_cfg), seed=20 + _cfg)
PLAN_SPLIT = lin(0, 320, 64, seed=30)            # M from the device's CU count (tests/test_exact_gpu.py: two whole rounds of tiles + 8 row tiles)
# weight-stationary kernels (csrc/gemm_ws.hip): their minimum of 8192 rows + a ragged remainder
WS_M = 8192 + 37
WS_CASES = {
    "plain": lin(WS_M, 320, 320, bias=None, residual=False, seed=40),
    "bias_residual": lin(WS_M, 320, 320, seed=41),
    "rowadd_residual": lin(WS_M, 320, 320, bias=None, rowadd_div=4096, seed=42),
    "rowstats": lin(WS_M, 320, 320, seed=43),
    "colstats": lin(8192 + 64, 320, 320, seed=44),          # column moments come in 64-row strips
    "wide_960": lin(WS_M, 960, 320, seed=45),
}


def lin_problem(c, M=None):
    M, N, K, s = (c["M"] if M is None else M), c["N"], c["K"], 100 * c["seed"] + 7000
    p = dict(x=randn((M, K), s + 1).half(), w=randn((N, K), s + 2, K ** -0.5).half(), bias=None, rowadd=None, residual=None)
    if c["bias"]:
        p["bias"] = randn((N if c["bias"] == "n" else M,), s + 3)
    if c["rowadd_div"]:
        p["rowadd"] = randn(((M + c["rowadd_div"] - 1) // c["rowadd_div"], N), s + 4)
    if c["residual"]:
        p["residual"] = randn((M, N), s + 5).half()
    return p


def lin_ref(c, p, dtype=F64):
    """alpha x W^T + bias + rowadd + residual in `dtype` on the tensors' device (fp64: the reference; fp32: the plain torch form)."""
    ref = c["alpha"] * (p["x"].to(dtype) @ p["w"].to(dtype).t())
    if c["bias"] == "n":
        ref = ref + p["bias"].to(dtype)
    elif c["bias"] == "m":
        ref = ref + p["bias"].to(dtype)[:, None]
    if c["rowadd_div"]:
        ref = ref + p["rowadd"].to(dtype).repeat_interleave(c["rowadd_div"], 0)[:ref.shape[0]]
    if c["residual"]:
        ref = ref + p["residual"].to(dtype)
    return ref


def lin_f32_bound(c, p):
    """OUT_F32: a bound on |out - ref| per element, valid for ANY order of the fp32 sum: (K + 4) 2^-24 (|alpha| |x| |w|^T + |addends|) -
    K - 1 additions and the epilogue's few operations, each rounding what has been accumulated by at most 2^-24 relative."""
    mag = abs(c["alpha"]) * (p["x"].double().abs() @ p["w"].double().abs().t())
    mag = mag + lin_ref(dict(c, alpha=0.0), {k: (v.abs() if torch.is_tensor(v) else v) for k, v in p.items()})
    return (c["K"] + 4) * 2.0 ** -24 * mag


# GEGLU: N = 2 D projection rows, out[m, j] = a_j * gelu_erf(g_j); K, D
GEGLU_CASES = {"k64": (300, 64, 128), "k320": (293, 320, 320)}


def geglu_problem(M, K, D, seed):
    return dict(x=randn((M, K), seed + 1).half(), w=randn((2 * D, K), seed + 2, K ** -0.5).half(), bias=randn((2 * D,), seed + 3))


def geglu_ref(h, dtype=F64):
    """x * 0.5 g (1 + erf(g / sqrt 2)) of h = [x | g]."""
    a, g = h.to(dtype).chunk(2, dim=-1)
    return a * (0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0))))


# LayerNorm folded into the projection: rows x K -> N; `offset`: a common offset of every row in standard deviations.  With an offset of
# 3 the accumulator holds x W'^T ~ 3 colsum ~ 3 and mean colsum cancels it to O(1) BY DESIGN; the accumulator's fp32 rounding is then
# 3 x 2^-24, three fp32 ulps of the result - nothing next to the 700 the bound allows, so the offset case is held to the same 1.05.
LNFOLD_CASES = {"k320": (293, 136, 320, 1.0, 0.0), "k64_alpha": (549, 72, 64, 0.37, 0.0), "k1280": (293, 136, 1280, 1.0, 0.0), "k320_offset": (293, 136, 320, 1.0, 3.0)}


def lnfold_problem(M, N, K, offset, seed):
    """x fp16, the folded (W' fp16, colsum fp32, bias' fp32) of packing.fold_layernorm restated (w' = fp16(gamma o w), colsum = fp32 row
    sums of the ROUNDED w', bias' = bias + w beta), so that this module imports nothing of the package."""
    x = (randn((M, K), seed + 1) + offset).half()
    w32, gamma, beta, bias = randn((N, K), seed + 2, K ** -0.5), 1 + 0.3 * randn((K,), seed + 3), 0.2 * randn((K,), seed + 4), randn((N,), seed + 5)
    wf = (w32 * gamma[None, :]).half()
    return dict(x=x, wf=wf, colsum=wf.double().sum(1).float(), bias=(w32 @ beta + bias).contiguous())


def row_stats_f32(x, eps=1e-5):
    """(mean, rstd) fp32 per row of an fp16 tensor: what the CPU tests hand to lnfold_ref in place of vcx_rowstats_f16."""
    xd = x.double()
    return torch.stack([xd.mean(1), 1.0 / torch.sqrt(xd.var(1, unbiased=False) + eps)], dim=1).float()


def lnfold_ref(p, stats, alpha, dtype=F64):
    """alpha rstd (x W'^T - mean colsum) + bias' with the statistics AS PASSED (include/vcx.h VCX_GEMM_LNFOLD)."""
    acc = p["x"].to(dtype) @ p["wf"].to(dtype).t()
    mean, rstd = stats[:, 0].to(dtype)[:, None], stats[:, 1].to(dtype)[:, None]
    return alpha * rstd * (acc - mean * p["colsum"].to(dtype)[None, :]) + p["bias"].to(dtype)[None, :]


# ------------------------------------------------------------------------------------------------------------------ convolutions
# exact_inputs.conv_case geometry with real-valued data; `rowadd`: a per-image addend vector (the ResBlock embedding add)
def _cc(*a, rowadd=False, dma=None, **kw):
    c = X.conv_case(*a, **kw)
    c.update(rowadd=rowadd, dma=dma)
    return c


CONV_CASES = {
    "c32_s1": _cc(2, 17, 19, 32, 136),                                # cin = 32: the register-staged kernel
    "c64_s1": _cc(2, 17, 19, 64, 136),
    "c320_s1": _cc(1, 17, 19, 320, 136),                              # K = 2880
    "c32_s2": _cc(4, 17, 19, 32, 104, stride=2),
    "c64_s2": _cc(4, 17, 19, 64, 104, stride=2),
    "c64_ups": _cc(2, 9, 11, 64, 72, ups=1),
    "c32_ups": _cc(2, 9, 11, 32, 72, ups=1),
    "c64_vae_down": _cc(4, 16, 18, 64, 136, stride=2, pad=(0, 0), asym=True),
    "c64_1x1_residual": _cc(2, 17, 19, 64, 136, kh=1, kw=1, residual=True),
    "c320_1x1_residual": _cc(2, 17, 19, 320, 136, kh=1, kw=1, residual=True),
    "c64_tapmajor": _cc(2, 17, 19, 64, 136, slabk=False),
    "c64_slabk_register": _cc(2, 17, 19, 64, 136, dma=0),              # slab-major K on the register-staged kernel (knob GEMM_DMA = 0)
    "c320_slabk_register": _cc(1, 17, 19, 320, 136, dma=0),
    "c64_temporal": _cc(2, 5, 67, 64, 72, kh=3, kw=1),
    "c320_temporal": _cc(2, 5, 67, 320, 72, kh=3, kw=1),
    "c64_tail1": _cc(2, 17, 19, 64, 136, tails=(64,)),
    "c64_tail2": _cc(2, 17, 19, 64, 72, tails=(128, 64)),
    "c320_tail1": _cc(1, 17, 19, 320, 136, tails=(64,)),             # K = 2880 + 64
    "c64_rowadd": _cc(2, 17, 19, 64, 136, rowadd=True, residual=True),
}


def conv_problem(c, seed):
    Ho, Wo = X.conv_out_hw(c)
    M = c["n"] * Ho * Wo
    K = c["kh"] * c["kw"] * c["cin"] + sum(c["tails"])
    p = dict(x=randn((c["n"], c["H"], c["W"], c["cin"]), seed + 1).half(), w=randn((c["cout"], c["cin"], c["kh"], c["kw"]), seed + 2, K ** -0.5).half(),
             bias=randn((c["cout"],), seed + 3), out_hw=(Ho, Wo), residual=None, rowadd=None)
    p["tail_src"] = [randn((M, k), seed + 10 + j).half() for j, k in enumerate(c["tails"])]
    p["tail_w"] = [randn((c["cout"], k), seed + 20 + j, K ** -0.5).half() for j, k in enumerate(c["tails"])]
    if c["residual"]:
        p["residual"] = randn((M, c["cout"]), seed + 30).half()
    if c["rowadd"]:
        p["rowadd"] = randn((c["n"], c["cout"]), seed + 31)
    return p


def _conv_addends(c, p, y, dtype):
    """+ K tail + residual + per-image rowadd on y [n, Ho, Wo, cout]."""
    n, Ho, Wo, cout = y.shape
    for src, wt in zip(p["tail_src"], p["tail_w"]):
        y = y + (src.to(dtype) @ wt.to(dtype).t()).view(y.shape)
    if p["residual"] is not None:
        y = y + p["residual"].to(dtype).view(y.shape)
    if p["rowadd"] is not None:
        y = y + p["rowadd"].to(dtype)[:, None, None, :]
    return y


def conv_ref(c, p):
    """The convolution tap by tap in fp64 on the tensors' device (no library convolution: fp64 is not every backend's), + bias."""
    x = p["x"].double()
    if c["ups"]:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)          # nearest 2x
    ph, pw = (0, 0) if c["asym"] else c["pad"]
    x = F.pad(x, (0, 0, pw, pw + (1 if c["asym"] else 0), ph, ph + (1 if c["asym"] else 0)))
    Ho, Wo = p["out_hw"]
    s = c["stride"]
    w = p["w"].double()
    y = p["bias"].double().expand(c["n"], Ho, Wo, c["cout"]).clone()
    for ky in range(c["kh"]):
        for kx in range(c["kw"]):
            y += x[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s, :] @ w[:, :, ky, kx].t()
    return _conv_addends(c, p, y, F64)


def conv_f32(c, p):
    """The plain fp32 torch form: F.conv2d."""
    x = p["x"].float().permute(0, 3, 1, 2)
    if c["ups"]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if c["asym"]:
        x = F.pad(x, (0, 1, 0, 1))
    y = F.conv2d(x, p["w"].float(), p["bias"], stride=c["stride"], padding=(0, 0) if c["asym"] else c["pad"]).permute(0, 2, 3, 1)
    return _conv_addends(c, p, y, torch.float32)


# ------------------------------------------------------------------------------------------------------------------ norms, softmax
GROUPNORM_CASES = {"c64": (2, 300, 64, 1e-5), "c320": (2, 77, 320, 1e-6)}          # n, pixels, C, eps
GROUPNORM_SPLIT = (2, 200, 64, 32, 1e-5)                                           # n, pixels, c1, c2, eps
GN_FOLD = (2, 500, 320, 136, 1e-6)                                                 # n, pixels, C, N, eps
LAYERNORM_CASES = {64: 520, 320: 110, 1280: 37}                                    # C -> rows
SOFTMAX_CASES = {512: (70, 520), 135: (250, 144)}                                  # n -> (rows, ld)


def gn_problem(n, pix, C, seed):
    return dict(x=(randn((n, pix, C), seed + 1) * (1 + randn((1, 1, C), seed + 2).abs()) + 0.5 * randn((1, 1, C), seed + 3)).half(),
                gamma=1 + 0.3 * randn((C,), seed + 4), beta=0.5 * randn((C,), seed + 5))


def gn_stats_f32(x, groups=32):
    """(mean, biased variance) fp32 [n, groups, 2]: what the CPU tests use in place of vcx_groupnorm_stats_f16."""
    n, pix, C = x.shape
    xd = x.double().view(n, pix, groups, C // groups)
    return torch.stack([xd.mean(dim=(1, 3)), xd.var(dim=(1, 3), unbiased=False)], dim=-1).float()


def gn_ref(x, stats, gamma, beta, eps, silu, dtype=F64, groups=32):
    """(x - mean) rsqrt(var + eps) gamma + beta [, x sigmoid(x)] with the fp32 statistics AS GIVEN (include/vcx.h)."""
    n, pix, C = x.shape
    mean = stats[..., 0].to(dtype).repeat_interleave(C // groups, 1)[:, None, :]
    rstd = (1.0 / torch.sqrt(stats[..., 1].to(dtype) + eps)).repeat_interleave(C // groups, 1)[:, None, :]
    y = (x.to(dtype) - mean) * rstd * gamma.to(dtype) + beta.to(dtype)
    return y * torch.sigmoid(y) if silu else y


def gn_fold_wn_ref(w32, gamma, stats, eps, dtype=F64, groups=32):
    """Wn[n][o][c] = W[o][c] gamma[c] rstd[n, g(c)] before its fp16 rounding."""
    C = w32.shape[1]
    rstd = (1.0 / torch.sqrt(stats[..., 1].to(dtype) + eps)).repeat_interleave(C // groups, 1)          # [n, C]
    return w32.to(dtype)[None] * (gamma.to(dtype)[None, :] * rstd)[:, None, :]


def ln_problem(rows, C, seed):
    return dict(x=(randn((rows, C), seed + 1) * 2 + 0.4).half(), gamma=1 + 0.3 * randn((C,), seed + 2), beta=0.5 * randn((C,), seed + 3))


def ln_ref(p, eps=1e-5, dtype=F64):
    x = p["x"].to(dtype)
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * p["gamma"].to(dtype) + p["beta"].to(dtype)


# ------------------------------------------------------------------------------------------------------------------ attention
# The attention kernels round the probabilities to fp16 before P V: ONE rounding is not their contract.  MODELS writes their rounding
# points down, each with the source line it comes from; attn_model() emulates exactly those in fp64 - everything else exact (scores,
# exponentials, sums) - and a kernel is held to E_kernel <= 1.05 E_model on the same inputs: the 5 % is the allowance for the summation
# order and the fp32 arithmetic.  A wider gap means a rounding point that is missing here.
# The running maximum is part of the model where a kernel defers it (FLASH_DEFER = 8 in log2 units): a tile of keys is exponentiated
# against the maximum of the EARLIER tiles unless some query of the wave's block exceeds that by more than 2^8, so the largest probability
# of a row is 2^x, x <= 8, with a full fp16 rounding error, where the exact row maximum would make it exactly 1.  On peaked softmaxes
# (logit gain 4) that alone is worth 17 % of E (measured on an MI355X: 1.24 - 1.28 against 1.06 for the exact-maximum model), far
# beyond the 5 % allowance, so the schedule - block of queries that vote, keys per tile - is emulated; it changes WHAT is rounded, not how
# often.  The temporal kernels use the exact row maximum.
_P16 = "unnormalised P = exp(s - m) to fp16 before the P V product, m the deferred running maximum: "
MODELS = {
    "flash_d64": [(_P16 + "blocks of 32 queries, tiles of 64 keys", "csrc/attention.hip:231-260"),
                  ("O = (P16 V) / l with l the fp32 sum of the UNROUNDED P, to fp16", "csrc/attention.hip:311")],
    "flash_d64_v2": [(_P16 + "blocks of 64 queries, tiles of 64 keys", "csrc/attention_v2.hip:243"), ("the deferred maximum's vote", "csrc/attention_v2.hip:500"),
                     ("O = (P16 V) / l (l: fp32 sum of the unrounded P, SUMV = 1), to fp16", "csrc/attention_v2.hip:560")],
    "flash_d64_accumulate": [(_P16 + "as flash_d64", "csrc/attention.hip:231-260"), ("the first call's O to fp16 (stored)", "csrc/attention.hip:311"),
                             ("read back, added to the second result in fp32, to fp16", "csrc/attention.hip:306-311")],
    "flash_dual_qb1": [(_P16 + "as flash_d64, both sets", "csrc/attention.hip:231-260"), ("first set's O / l kept in fp32", "csrc/attention.hip:287"),
                       ("sum of the two to fp16", "csrc/attention.hip:304-311")],
    "flash_dual_qb2": [(_P16 + "as flash_d64, both sets", "csrc/attention.hip:231-260"), ("first set's O / l kept as packed fp16 (registers)", "csrc/attention.hip:288"),
                       ("fp16 first + fp32 second, to fp16", "csrc/attention.hip:304-311")],
    "xattn_resident": [(_P16 + "blocks of 32 queries, tiles of 64 keys, both sets", "csrc/attention.hip:460-489"),
                       ("first set's O / l kept as packed fp16", "csrc/attention.hip:512"), ("fp16 first + fp32 second, to fp16", "csrc/attention.hip:522-523")],
    "xattn_resident2": [(_P16 + "blocks of 32 queries, HALF tiles of 32 keys, both sets", "csrc/attention.hip:755-793"),
                        ("first set's O / l kept as packed fp16 (parked in LDS)", "csrc/attention.hip:680-681"), ("fp16 first + fp32 second, to fp16", "csrc/attention.hip:819")],
    "flash_d512": [(_P16 + "blocks of 16 queries, tiles of 32 keys", "csrc/attention.hip:977-995"), ("O = (P16 V) / l, to fp16", "csrc/attention.hip:1020-1021")],
    "temporal_d64": [("unnormalised P = exp(s - exact row max) to fp16 before the P V product (T <= 32; the 2 x 2-tile kernel beyond: :1310)", "csrc/attention.hip:1150"),
                     ("O = (P16 V) (1 / l) in fp32, to fp16 (:1341 beyond 32 frames)", "csrc/attention.hip:1188-1202")],
    "temporal_d64_relp": [("P16 as temporal_d64", "csrc/attention.hip:1150"), ("inner slots: fp16(P16 / l)", "csrc/attention.hip:1159-1163"),
                          ("end slots: fp32 sum of P16 / l over the keys beyond +-R, to fp16", "csrc/attention.hip:1161-1170")],
    "softmax_rows": [("exp(x - max) / sum in fp32, to fp16: one rounding", "csrc/attention.hip:1389")],
}
# which points a model applies: p16 (probabilities), defer = (queries per voting block, keys per tile) of the deferred maximum, keep16 (the
# first of two partial results), readback (ACCUMULATE)
FLASH_DEFER_LOG2 = 8.0
MODEL_POINTS = {"flash_d64": dict(p16=True, defer=(32, 64)), "flash_d64_v2": dict(p16=True, defer=(64, 64)),
                "flash_d64_accumulate": dict(p16=True, defer=(32, 64), readback=True), "flash_dual_qb1": dict(p16=True, defer=(32, 64)),
                "flash_dual_qb2": dict(p16=True, defer=(32, 64), keep16=True), "xattn_resident": dict(p16=True, defer=(32, 64), keep16=True),
                "xattn_resident2": dict(p16=True, defer=(32, 32), keep16=True), "flash_d512": dict(p16=True, defer=(16, 32)), "temporal_d64": dict(p16=True)}


def attn_exact(q, k, v, c, base2=False, mask=None, add=None):
    """softmax(c q k^T [+ c add]) v in fp64; q [..., nq, d], k / v [..., nk, d].  base2: the logits are base-2 (VCX_ATTN_LOG2_LOGITS).
    Returns (o, p, e, l, s): the output, the probabilities, exp(s - rowmax), their row sums, and the logits minus the row maximum."""
    s = q.double() @ k.double().transpose(-1, -2)
    if add is not None:
        s = s + add
    s = s * c
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    s = s - s.max(-1, keepdim=True).values
    e = torch.exp2(s) if base2 else torch.exp(s)
    l = e.sum(-1, keepdim=True)
    return (e / l) @ v.double(), e / l, e, l, s


def deferred_max(s, qblock, ktile, thr):
    """The running maximum in effect for every key [..., nq, nk] under the deferred update of the flash kernels: tile by tile, the maximum
    moves to max(m, tile maximum) - for all queries of a block of `qblock` consecutive queries at once - when ANY of them has a tile
    maximum above its m + thr; the first tile always moves it."""
    nq, nk = s.shape[-2:]
    pad = (-nq) % qblock
    m = torch.full(s.shape[:-1] + (1,), float("-inf"), dtype=s.dtype, device=s.device)
    M = torch.empty_like(s)
    for k0 in range(0, nk, ktile):
        cand = s[..., k0:k0 + ktile].max(-1, keepdim=True).values
        trig = F.pad(cand > m + thr, (0, 0, 0, pad))                                            # (-inf + thr: the first tile)
        trig = trig.view(trig.shape[:-2] + (-1, qblock, 1)).any(-2, keepdim=True).expand(trig.shape[:-2] + (-1, qblock, 1)).reshape(trig.shape)[..., :nq, :]
        m = torch.where(trig, torch.maximum(m, cand), m)
        M[..., k0:k0 + ktile] = m
    return M


def attn_unrounded(q, k, v, c, base2=False, mask=None, add=None, p16=True, normalise_first=False, defer=None, extra_rounding=False):
    """The attention output BEFORE its output rounding under the rounding points of MODELS: unnormalised probabilities rounded to fp16
    (p16) relative to the exact row maximum or (defer = (qblock, ktile)) the deferred running one, the row sum from the unrounded ones.
    Two variants that the CPU tests set against a model: normalise_first - P = fp16(e / l), then no later scaling (another place for the
    same number of roundings: it costs the exact-maximum models 15 %) - and extra_rounding - ONE MORE point, the accumulated P16 V
    rounded to fp16 before it is scaled by 1 / l."""
    o, p, e, l, s = attn_exact(q, k, v, c, base2, mask, add)
    if normalise_first:
        return h64(p) @ v.double()
    if not p16:
        return (e @ v.double()) / l
    if defer is None:
        num = h64(e) @ v.double()
    else:
        M = deferred_max(s, defer[0], defer[1], FLASH_DEFER_LOG2 * (1.0 if base2 else math.log(2.0)))      # <= 0: relative to the row maximum
        ex = torch.exp2 if base2 else torch.exp
        num = (h64(ex(s - M)) * ex(M)) @ v.double()
    return (h64(num) if extra_rounding else num) / l


def attn_model(kernel, parts, **variant):
    """The model output (fp64, fp16-representable) of `kernel` for parts = [(q, k, v, c, base2, mask, add), ...]: one part, or the two of
    a dual / accumulating call in the order they are computed."""
    pts = dict(MODEL_POINTS[kernel], **variant)
    outs = [attn_unrounded(*part, p16=pts.get("p16", False), normalise_first=pts.get("normalise_first", False), defer=pts.get("defer"),
                           extra_rounding=pts.get("extra_rounding", False)) for part in parts]
    if len(outs) == 1:
        return h64(outs[0])
    first = h64(outs[0]) if (pts.get("keep16") or pts.get("readback")) else outs[0]
    return h64(first + outs[1])


def flash_problem(G, heads, nq, nk, gain, seed, d=64):
    """q [G, heads, nq, d] (x gain), k, v [G, heads, nk, d]: N(0, 1), so that scale = d^-0.5 gives logits of standard deviation `gain`."""
    return randn((G, heads, nq, d), seed + 1, gain).half(), randn((G, heads, nk, d), seed + 2).half(), randn((G, heads, nk, d), seed + 3).half()


# Two partial results with the first one rounded before the sum (ACCUMULATE's read-back, the packed first half of three of the four dual
# forms) make a THREE-point model, and its E depends on how the two halves compare: with a first half as large as the second or larger -
# 77 text keys against 256 image keys at logit gain 1 - it sits at 1.5 - 1.6, above E_MODEL_CAP.  The cases below keep every model under
# the cap (tests/test_rounding_cpu.py asserts it and prints the others): ACCUMULATE onto the longer key set's result, the packed dual
# forms at logit gains 4 and 6, the fp32 one at 1 and 4.
ACCUMULATE_CASES = ((256, 77), (1024, 77))                      # (nk of the first call, nk of the accumulating call), gains 1 and 4
DUAL_KEYS = (77, 256)
DUAL_GAINS = {"flash_dual_qb1": (1.0, 4.0), "flash_dual_qb2": (4.0, 6.0), "xattn_resident": (4.0, 6.0), "xattn_resident2": (4.0, 6.0)}


def accumulate_problem(nk1, nk2, gain):
    q, k1, v1 = flash_problem(2, 2, 128, nk1, gain, 730)
    return q, k1, v1, randn((2, 2, nk2, 64), 735).half(), randn((2, 2, nk2, 64), 736).half()


def dual_problem(gain, B=2, T=2, heads=2, nq=128):
    """q [B T, heads, nq, 64] (x gain), two key / value sets [B, heads, nk, 64] shared by the T frames of a video."""
    q = randn((B * T, heads, nq, 64), 740, gain).half()
    return (q,) + tuple(randn((B, heads, nk, 64), 741 + i).half() for i, nk in enumerate((DUAL_KEYS[0], DUAL_KEYS[0], DUAL_KEYS[1], DUAL_KEYS[1])))


LOG2E = 1.4426950408889634


def log2_q(q, scale):
    """What a caller of VCX_ATTN_LOG2_LOGITS stores: fp16(q scale log2 e) - the kernel's operand, so the reference starts from it."""
    return (q.float() * (scale * LOG2E)).half()


TEMPORAL_CASES = {16: 16, 25: 11, 33: 8, 64: 4}                  # T -> pixels (x 2 heads x 64 columns >= 32768 outputs)
TEMPORAL_REL_CASES = {16: (64, 8), 25: (20, 16)}                 # T -> (pixels, R): tokens x heads x (2 R + 1) slots >= 32768


def temporal_problem(B, T, P, heads, seed, gain=1.0):
    """q, k, v [B, T, P, heads, 64]"""
    return tuple(randn((B, T, P, heads, 64), seed + i, gain if i == 1 else 1.0).half() for i in (1, 2, 3))


def temporal_split(t):
    """[B, T, P, heads, 64] -> [B, P, heads, T, 64]"""
    return t.permute(0, 2, 3, 1, 4)


def temporal_merge(o):
    """[B, P, heads, T, 64] -> [(b t p), heads * 64]"""
    B, P, heads, T, d = o.shape
    return o.permute(0, 3, 1, 2, 4).reshape(B * T * P, heads * d)


def rel_index(T, R, device="cpu"):
    t = torch.arange(T, device=device)
    return (t[None, :] - t[:, None]).clamp(-R, R) + R          # [query, key] -> slot


def relp_ref_and_model(q, k, relg, R, scale, causal):
    """relp of vcx_attn_temporal_d64_rel_f16 in fp64 - (reference, model), each [B, P, heads, T, 2R + 1] - for q, k [B, P, heads, T, 64] and
    relg [B, P, heads, T, 64]: the probabilities of a query by clipped distance.  Model: P16 / l per key, inner slots rounded to fp16,
    end slots summed in fp32 (exact here) and rounded."""
    T = q.shape[-2]
    idx = rel_index(T, R, q.device).expand(q.shape[:-2] + (T, T))
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool, device=q.device)) if causal else None
    _, p, e, l, _ = attn_exact(q, k, k, scale, mask=mask, add=torch.gather(relg.double(), -1, idx))
    slots = torch.zeros(q.shape[:-1] + (2 * R + 1,), dtype=F64, device=q.device)
    ref = slots.scatter_add(-1, idx, p)
    model = h64(slots.scatter_add(-1, idx, h64(e) / l))
    return ref, model


# ------------------------------------------------------------------------------------------------------------------ planted defects
def defect_second_rounding(c, p):
    """The result rounded to fp16, then the residual added and rounded again."""
    c0 = dict(c, residual=False)
    return (lin_ref(c0, p, torch.float32).half().float() + p["residual"].float()).half()


def defect_slab_rounding(c, p, slab=64):
    """The accumulator rounded to fp16 after every 64-wide K slab."""
    x, w = p["x"].float(), p["w"].float()
    acc = torch.zeros((x.shape[0], w.shape[0]))
    for k0 in range(0, c["K"], slab):
        acc = (acc + x[:, k0:k0 + slab] @ w[:, k0:k0 + slab].t()).half().float()
    return lin_ref(dict(c, alpha=0.0), p, torch.float32).add(c["alpha"] * acc).half()


def defect_truncation(c, p):
    """The final conversion toward zero instead of to nearest-even."""
    y = lin_ref(c, p, torch.float32)
    h = y.half()
    away = h.float().abs() > y.abs()                              # rounded away from zero: step one fp16 back toward it
    bits = h.view(torch.int16)
    return torch.where(away, bits - 1, bits).view(torch.float16)


# ------------------------------------------------------------------------------------------------------------------ DDIM step
def ddim_ref(x, v_cond, v_uncond, noise, coef, v_img=None, cfg_img=0.0, dtype=F64):
    """include/vcx.h vcx_ddim_step3_f32 in `dtype` throughout (fp64: the reference; fp32: the plain torch form whose own error scales the
    bound).  coef = {sqrt_acp_t, sqrt_1m_acp_t, a_prev, sigma_t, scale_ratio, cfg_scale, guidance_rescale, parameterization_is_v} as the
    fp32 values the kernel receives; the host-side square roots of a_prev and 1 - a_prev - sigma^2 are fp32 there (csrc/elementwise.hip)."""
    f32 = lambda t: float(torch.as_tensor(t, dtype=torch.float32))
    sa, s1, a_prev, sigma, ratio, cfg, resc, is_v = [f32(c) for c in coef[:8]]
    cfg_img = f32(cfg_img)
    sqrt_a_prev = f32(torch.sqrt(torch.tensor(a_prev, dtype=torch.float32)))
    dir2 = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(a_prev, dtype=torch.float32) - torch.tensor(sigma, dtype=torch.float32) ** 2
    dir_coef = f32(torch.sqrt(dir2.clamp_min(0)))
    t = lambda z: None if z is None else z.to(dtype)
    x, vc, vu, vi, nz = t(x), t(v_cond), t(v_uncond), t(v_img), t(noise)
    if vu is None:
        v = vc
    elif vi is None:
        v = vu + cfg * (vc - vu)
    else:
        v = vu + cfg_img * (vi - vu) + cfg * (vc - vi)
    if vu is not None and resc > 0:
        dims = tuple(range(1, v.dim()))
        v = v * (resc * (vc.std(dim=dims, keepdim=True) / v.std(dim=dims, keepdim=True)) + (1 - resc))
    if is_v:
        e_t, x0 = sa * v + s1 * x, sa * x - s1 * v
    else:
        e_t, x0 = v, (x - s1 * v) / sa
    x0 = x0 * ratio
    xp = sqrt_a_prev * x0 + dir_coef * e_t
    if nz is not None and sigma != 0:
        xp = xp + sigma * nz
    return xp, x0


DDIM_BRANCHES = {
    # name: (coef, uncond, img, cfg_img, noise given)
    "no_guidance": ([0.6, 0.8, 0.5, 0.0, 1.0, 7.5, 0.7, 1.0], False, False, 0.0, False),
    "cfg": ([0.6, 0.8, 0.5, 0.0, 1.0, 7.5, 0.0, 1.0], True, False, 0.0, False),
    "cfg_rescale": ([0.6, 0.8, 0.5, 0.0, 1.0, 7.5, 0.7, 1.0], True, False, 0.0, False),
    "multicond": ([0.6, 0.8, 0.5, 0.0, 1.0, 7.5, 0.0, 1.0], True, True, 3.0, False),
    "multicond_rescale": ([0.6, 0.8, 0.5, 0.0, 1.0, 7.5, 0.7, 1.0], True, True, 3.0, False),
    "eps_param": ([0.6, 0.8, 0.5, 0.0, 1.0, 7.5, 0.7, 0.0], True, False, 0.0, False),
    "noise": ([0.6, 0.8, 0.5, 0.3, 1.0, 7.5, 0.7, 1.0], True, False, 0.0, True),
    "sigma0_with_noise_pointer": ([0.6, 0.8, 0.5, 0.0, 1.0, 7.5, 0.7, 1.0], True, False, 0.0, True),
    "scale_ratio": ([0.6, 0.8, 0.5, 0.0, 0.85, 7.5, 0.7, 1.0], True, False, 0.0, False),
}
DDIM_SIZES = [(1, 2), (3, 255), (1, 257), (3, 65536 + 3)]          # (B, n): the reduction grid is capped at 256 blocks of 256 threads


def ddim_problem(B, n, seed, offset=0.0):
    """x, v_cond, v_uncond, v_img, noise fp32 [B, n]; sample b has standard deviation 0.5 + b (a statistic read from the wrong sample
    shows); `offset`: a common offset of v_cond / v_uncond / v_img in standard deviations."""
    sd = (0.5 + torch.arange(B, dtype=torch.float32))[:, None]
    x, vc, du, di, nz = [randn((B, n), seed + i) for i in range(5)]
    vc = vc * sd
    return x, vc + offset * sd, (0.8 * vc + 0.3 * sd * du) + offset * sd, (0.9 * vc + 0.2 * sd * di) + offset * sd, nz
