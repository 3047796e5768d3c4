"""Rounding quality of every kernel family that writes fp16: the error against the fp64 result of the documented function, relative to the
ONE rounding a correct kernel cannot avoid (tests/rounding_quality.py: E = rms(out - ref) / rms(fp16(ref) - ref)).

 - one-rounding tier (GEMM / convolution epilogues, norms, softmax, element-wise): E <= 1.05, derived in tests/rounding_quality.py; the
   share of elements that differ from fp16(ref) is printed and capped at 10 %.
 - attention tier: the kernels round the probabilities to fp16 before P V; their rounding points are written down in
   rounding_quality.MODELS with source lines, emulated in fp64, and E_kernel <= 1.05 E_model on the same inputs.
 - the DDIM step (fp32) against fp64, bounded by the error of the plain fp32 torch form in the same run.
tests/test_rounding_cpu.py shows on the same inputs that the fp32 torch form passes and that planted extra roundings fail.
Every case prints `[rounding] kernel case E mismatch`; profiles/rounding_quality.md keeps one run's values.
"""
import pytest
import torch

from tests import exact_inputs as X
from tests import rounding_quality as R
from tests.test_exact_gpu import environ, knobs, kv_layout, plan_lines

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(p):
    return {k: (v.to(DEV) if torch.is_tensor(v) else [t.to(DEV) for t in v] if isinstance(v, list) else v) for k, v in p.items()}


def run_lin(c, p, out_f32=False):
    from viewcrafter_amd import ops
    M, K = p["x"].shape
    kw = {}
    if p["rowadd"] is not None:
        kw.update(rowadd=p["rowadd"], rowadd_div=c["rowadd_div"])
    if p["residual"] is not None:
        kw.update(residual=p["residual"])
    out = ops.gemm(p["x"], p["w"], M=M, N=c["N"], K=K, lda=K, alpha=c["alpha"], bias=p["bias"], bias_m=c["bias"] == "m", out_f32=out_f32, **kw)
    torch.cuda.synchronize()
    return out


# ================================================================================================================ vcx_gemm_f16, linear mode
@pytest.mark.parametrize("name", sorted(R.LINEAR_CASES))
def test_linear_rounds_once(name, capfd):
    """The register-staged kernel (GEMM_DMA 0, K = 72), the tiled engine on its automatic plan with every epilogue (plain, alpha, BIAS_N,
    BIAS_M, ROWADD, RESIDUAL, bias + residual) and under GEMM_CFG 0 - 5, K in {64, 320, 1280, 2880}."""
    c = R.LINEAR_CASES[name]
    p = dev(R.lin_problem(c))
    capfd.readouterr()
    with knobs(**c["knobs"]), environ("VCX_GEMM_PLAN_TRACE", "1"):
        out = run_lin(c, p)
    lines = plan_lines(capfd.readouterr().err)
    register = name.startswith("reg_")
    assert bool(lines) != register, f"{name}: expected the {'register-staged kernel' if register else 'tiled engine'}: {lines}"
    if "GEMM_CFG" in c["knobs"]:
        assert all(f"cfg {c['knobs']['GEMM_CFG']} " in l for l in lines), lines
    R.check_rounding("gemm_linear", name, out, R.lin_ref(c, p))


def test_linear_rounds_once_on_a_plan_of_two_segments(capfd):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    c = R.PLAN_SPLIT
    p = dev(R.lin_problem(c, M=(2 * ncu + 8) * 256 - 37))
    capfd.readouterr()
    with environ("VCX_GEMM_PLAN_TRACE", "1"):
        out = run_lin(c, p)
    lines = plan_lines(capfd.readouterr().err)
    assert len(lines) == 2 and "seg 1/2" in lines[0] and "seg 2/2" in lines[1], lines
    R.check_rounding("gemm_linear", "plan_split", out, R.lin_ref(c, p))


@pytest.mark.parametrize("name", ["bias_residual_k64", "bias_residual_k1280", "reg_k72", "cfg2"])
def test_linear_fp32_output_is_inside_the_summation_order_bound(name):
    """OUT_F32: no fp16 rounding, so E does not apply: |out - ref| <= (K + 4) 2^-24 (|alpha| |x| |w|^T + |addends|) per element, which
    holds for any order of the fp32 sum (rounding_quality.lin_f32_bound)."""
    c = R.LINEAR_CASES[name]
    p = dev(R.lin_problem(c))
    with knobs(**c["knobs"]):
        out = run_lin(c, p, out_f32=True)
    assert out.dtype == torch.float32
    ref, bound = R.lin_ref(c, p), R.lin_f32_bound(c, p)
    print(f"\n[rounding] gemm_linear_f32 {name} max err / bound {float(((out.double() - ref).abs() / bound).max()):.3f}")
    X.assert_elementwise(out, ref, bound.cpu(), f"fp32 output {name}")


@pytest.mark.parametrize("name", sorted(R.GEGLU_CASES))
def test_geglu_rounds_once(name):
    """VCX_GEMM_GEGLU against fp64 x * 0.5 g (1 + erf(g / sqrt 2)) of the fp64 projection: the halves are never rounded on their own."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_geglu
    M, K, D = R.GEGLU_CASES[name]
    p = dev(R.geglu_problem(M, K, D, 300))
    wp, bp = pack_geglu(p["w"], p["bias"])
    out = ops.linear(p["x"], wp, bp, geglu=True)
    ref = R.geglu_ref(p["x"].double() @ p["w"].double().t() + p["bias"].double())
    R.check_rounding("gemm_geglu", name, out, ref)


@pytest.mark.parametrize("name", sorted(R.LNFOLD_CASES))
def test_lnfold_rounds_once(name):
    """VCX_GEMM_LNFOLD against alpha rstd (x W'^T - mean colsum) + bias' in fp64 with the statistics as passed (vcx_rowstats_f16's fp32
    pairs), zero-mean rows and rows offset by three standard deviations (rounding_quality.LNFOLD_CASES: what the cancellation may cost)."""
    from viewcrafter_amd import ops
    M, N, K, alpha, offset = R.LNFOLD_CASES[name]
    p = dev(R.lnfold_problem(M, N, K, offset, 400))
    st = ops.row_stats(p["x"], 1e-5)
    out = ops.linear(p["x"], p["wf"], p["bias"], alpha=alpha, ln_stats=st, ln_colsum=p["colsum"])
    R.check_rounding("gemm_lnfold", name, out, R.lnfold_ref(p, st, alpha))


def test_lnfold_transposed_rounds_once():
    """VCX_GEMM_LNFOLD_T: out[d, token]; the statistics index the output columns, colsum / bias' the rows."""
    from viewcrafter_amd import ops
    tokens, D = 136, 320
    p = dev(R.lnfold_problem(tokens, D, D, 0.0, 410))
    st = ops.row_stats(p["x"], 1e-5)
    out = ops.gemm(p["wf"], p["x"], M=D, N=tokens, K=D, lda=D, bias=p["bias"], bias_m=True, ln_stats=st, ln_colsum=p["colsum"], ln_t=True)
    R.check_rounding("gemm_lnfold_t", "d320", out, R.lnfold_ref(p, st, 1.0).t().contiguous())


@pytest.mark.parametrize("offset", [0.0, 3.0])
def test_lnfold_geglu_rounds_once(offset):
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_geglu
    M, K, D = 293, 320, 320
    p = dev(R.lnfold_problem(M, 2 * D, K, offset, 420))
    st = ops.row_stats(p["x"], 1e-5)
    wp, bp = pack_geglu(p["wf"], p["bias"])
    _, cp = pack_geglu(p["wf"], p["colsum"])
    out = ops.linear(p["x"], wp, bp, geglu=True, ln_stats=st, ln_colsum=cp)
    R.check_rounding("gemm_lnfold_geglu", f"offset{offset:g}", out, R.geglu_ref(R.lnfold_ref(p, st, 1.0)))


# ================================================================================================================ weight-stationary kernels
def _route(M, N, K, flags):
    from viewcrafter_amd import _lib, ops
    import ctypes
    return _lib.lib().vcx_gemm_route(ctypes.byref(ops._gemm_desc(M, N, K, K, N // 2 if flags & ops.GEMM_GEGLU else N, flags=flags)), 0)


@pytest.mark.parametrize("name", sorted(R.WS_CASES))
def test_weight_stationary_kernels_round_once(name, capfd):
    """csrc/gemm_ws.hip at M = 8192 + 37: plain, bias + residual, rowadd + residual, with the ROWSTATS / COLSTATS by-products (the fp16
    output only) and the wide form; the tiled engine prints no plan line."""
    from viewcrafter_amd import ops
    c = R.WS_CASES[name]
    p = dev(R.lin_problem(c))
    kw = {}
    if p["rowadd"] is not None:
        kw.update(rowadd=p["rowadd"], rowadd_div=c["rowadd_div"])
    if name == "rowstats":
        assert ops.rowstats_ok(c["M"], c["N"], c["K"], ldr=c["N"])
        kw.update(rowstats=ops.rowstats_buffer(c["M"], DEV))
    if name == "colstats":
        assert ops.colstats_ok(c["M"], 64, c["K"], c["N"])
        kw.update(colstats=ops.colstats_buffer(c["M"], c["N"], DEV))
    capfd.readouterr()
    with environ("VCX_GEMM_PLAN_TRACE", "1"):
        out = ops.linear(p["x"], p["w"], p["bias"], residual=p["residual"], **kw)
        torch.cuda.synchronize()
    assert not plan_lines(capfd.readouterr().err), "the tiled engine took a weight-stationary shape"
    R.check_rounding("gemm_ws320", name, out, R.lin_ref(c, p))


def test_weight_stationary_geglu_rounds_once():
    from viewcrafter_amd import _lib, ops
    from viewcrafter_amd.packing import pack_geglu
    M, K, D = R.WS_M, 320, 256
    assert _route(M, 2 * D, K, ops.GEMM_GEGLU | ops.GEMM_BIAS_N) == _lib.ROUTE_WS320_GEGLU
    p = dev(R.geglu_problem(M, K, D, 310))
    wp, bp = pack_geglu(p["w"], p["bias"])
    out = ops.linear(p["x"], wp, bp, geglu=True)
    ref = R.geglu_ref(p["x"].double() @ p["w"].double().t() + p["bias"].double())
    R.check_rounding("gemm_ws320_geglu", "n512", out, ref)


@pytest.mark.parametrize("N,ws,offset", [(960, 1, 0.0), (960, 1, 3.0), (576, 5, 0.0)])
def test_weight_stationary_lnfold_rounds_once(N, ws, offset):
    """gemm_ws320_lnf_kernel: N = 960 under the product rule, N = 576 (N % 64 == 0, a last column block a quarter full) under GEMM_WS 5."""
    from viewcrafter_amd import _lib, ops
    M, K = R.WS_M, 320
    p = dev(R.lnfold_problem(M, N, K, offset, 430))
    st = ops.row_stats(p["x"], 1e-5)
    with knobs(GEMM_WS=ws):
        assert _route(M, N, K, ops.GEMM_LNFOLD | ops.GEMM_BIAS_N) == _lib.ROUTE_WS320_LNF
        out = ops.linear(p["x"], p["wf"], p["bias"], alpha=0.37, ln_stats=st, ln_colsum=p["colsum"])
    R.check_rounding("gemm_ws320_lnf", f"n{N}_offset{offset:g}", out, R.lnfold_ref(p, st, 0.37))


@pytest.mark.parametrize("name,route", [("3x200", "grouped"), ("3x200", "loop"), ("ws_8x1024", "ws320")])
def test_gemm_units_round_once_on_every_route(name, route):
    from viewcrafter_amd import ops
    units, unit_rows, N, K = X.UNITS_CASES[name]
    x, w, b = R.randn((units * unit_rows, K), 50).half().to(DEV), R.randn((units, N, K), 51, K ** -0.5).half().to(DEV), R.randn((units, N), 52).to(DEV)
    with environ("VCX_GEMM_UNITS_LOOP", "1" if route == "loop" else "0"):
        assert ops.units_route(units * unit_rows, N, K, unit_rows) == route
        out = ops.gemm_units(x, w, b, unit_rows=unit_rows)
        torch.cuda.synchronize()
    ref = torch.einsum("urk,unk->urn", x.double().view(units, unit_rows, K), w.double()) + b.double()[:, None, :]
    R.check_rounding("gemm_units", f"{name}_{route}", out, ref.reshape(units * unit_rows, N))


# ================================================================================================================ convolutions
def run_conv(c, p):
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import conv_slab_major, pack_conv
    taps = c["kh"] * c["kw"]
    slabk = conv_slab_major(c["cin"], taps) if c["slabk"] is None else c["slabk"]
    w = p["w"]
    wp = pack_conv(w) if slabk == conv_slab_major(c["cin"], taps) else w.reshape(c["cout"], c["cin"], taps).permute(0, 2, 1).reshape(c["cout"], -1).contiguous()
    if p["tail_w"]:
        wp = torch.cat([wp] + p["tail_w"], dim=1).contiguous()
    Ho, Wo = p["out_hw"]
    M, N, K = c["n"] * Ho * Wo, c["cout"], wp.shape[1]
    geom = dict(in_h=c["H"], in_w=c["W"], out_h=Ho, out_w=Wo, cin=c["cin"], kh=c["kh"], kw=c["kw"], stride=c["stride"], pad_h=c["pad"][0], pad_w=c["pad"][1],
                ups=c["ups"], slabk=slabk)
    kw = {}
    if p["residual"] is not None:
        kw.update(residual=p["residual"], ldr=N)
    if p["rowadd"] is not None:
        kw.update(rowadd=p["rowadd"], rowadd_div=Ho * Wo)
    if p["tail_src"]:
        kw.update(tail=p["tail_src"])
    out = ops.gemm(p["x"], wp, M=M, N=N, K=K, lda=p["x"].stride(2), bias=p["bias"], conv=geom, **kw)
    torch.cuda.synchronize()
    return out.view(c["n"], Ho, Wo, N)


@pytest.mark.parametrize("name", sorted(R.CONV_CASES))
def test_convolutions_round_once(name, capfd):
    """3 x 3 at stride 1 / 2, fused nearest-2x, the VAE's asymmetric pad, 1 x 1 + residual, slab-major K on both kernels and tap-major K,
    temporal (3,1,1), a K tail with one and two sources, the per-image rowadd; cin in {32, 64, 320} (K up to 2880 + a tail of 64)."""
    c = R.CONV_CASES[name]
    p = dev(R.conv_problem(c, 500))
    dma = c["cin"] % 64 == 0 and c["dma"] != 0
    capfd.readouterr()
    with knobs(**({} if c["dma"] is None else dict(GEMM_DMA=c["dma"]))), environ("VCX_GEMM_PLAN_TRACE", "1"):
        out = run_conv(c, p)
    assert bool(plan_lines(capfd.readouterr().err)) == dma, f"{name}: expected the {'tiled engine' if dma else 'register-staged kernel'}"
    R.check_rounding("gemm_conv", name, out, R.conv_ref(c, p))


# ================================================================================================================ norms, softmax, element-wise
@pytest.mark.parametrize("name", sorted(R.GROUPNORM_CASES))
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_apply_rounds_once(name, silu):
    """vcx_groupnorm_apply_f16 with the statistics handed in as fp32 (the reference uses exactly those)."""
    from viewcrafter_amd import ops
    n, pix, C, eps = R.GROUPNORM_CASES[name]
    p = dev(R.gn_problem(n, pix, C, 600))
    stats = ops.group_norm_stats(p["x"])
    out = ops.group_norm(p["x"], p["gamma"], p["beta"], eps, silu, stats=stats)
    R.check_rounding("groupnorm_apply", f"{name}_silu{int(silu)}", out, R.gn_ref(p["x"], stats, p["gamma"], p["beta"], eps, silu))


def test_groupnorm_over_a_split_concat_rounds_once():
    from viewcrafter_amd import ops
    n, pix, c1, c2, eps = R.GROUPNORM_SPLIT
    p = dev(R.gn_problem(n, pix, c1 + c2, 640))
    x1, x2 = p["x"][..., :c1].contiguous(), p["x"][..., c1:].contiguous()
    stats = ops.group_norm_stats(p["x"])
    out = ops.group_norm(x1, p["gamma"], p["beta"], eps, True, stats=stats, x2=x2)
    R.check_rounding("groupnorm_apply2", "c64+32_silu1", out, R.gn_ref(p["x"], stats, p["gamma"], p["beta"], eps, True))


def test_groupnorm_fold_linear_weights_round_once():
    """vcx_groupnorm_fold_linear_f16: Wn = fp16(W gamma rstd) from the fp32 master weights and the fp32 statistics as given; bn (fp32)
    against fp64 with the ROUNDED Wn in the mean term, as the header defines it."""
    from viewcrafter_amd import ops
    n, pix, C, N, eps = R.GN_FOLD
    x = R.gn_problem(n, pix, C, 610)["x"].to(DEV)
    stats = ops.group_norm_stats(x)
    w32, gamma, beta, bias = [t.to(DEV) for t in (R.randn((N, C), 611, C ** -0.5), 1 + 0.3 * R.randn((C,), 612), 0.5 * R.randn((C,), 613), R.randn((N,), 614))]
    wn, bn = ops.group_norm_fold_linear(w32, bias, gamma, beta, stats, eps)
    R.check_rounding("groupnorm_fold_linear", "wn", wn, R.gn_fold_wn_ref(w32, gamma, stats, eps))
    mean = stats[..., 0].double().repeat_interleave(C // 32, 1)                                  # [n, C]
    bn_ref = bias.double()[None] + (w32.double() @ beta.double())[None] - torch.einsum("noc,nc->no", wn.double(), mean)
    mag = bias.double().abs()[None] + (w32.double().abs() @ beta.double().abs())[None] + torch.einsum("noc,nc->no", wn.double().abs(), mean.abs())
    X.assert_elementwise(bn, bn_ref, ((C + 4) * 2.0 ** -24 * mag).cpu(), "groupnorm_fold_linear bn")


@pytest.mark.parametrize("C", sorted(R.LAYERNORM_CASES))
def test_layernorm_rounds_once(C):
    from viewcrafter_amd import ops
    p = dev(R.ln_problem(R.LAYERNORM_CASES[C], C, 620))
    R.check_rounding("layernorm", f"c{C}", ops.layer_norm(p["x"], p["gamma"], p["beta"], 1e-5), R.ln_ref(p))


@pytest.mark.parametrize("n", sorted(R.SOFTMAX_CASES))
def test_softmax_rows_rounds_once(n):
    from viewcrafter_amd import ops
    rows, ld = R.SOFTMAX_CASES[n]
    x = (R.randn((rows, ld), 630) * 3).half().to(DEV)
    y = x.clone()
    ops.softmax_rows_(y, n=n)
    R.check_rounding("softmax_rows", f"n{n}", y[:, :n].contiguous(), x[:, :n].double().softmax(-1))


def test_elementwise_kernels_round_once():
    """add_nchw_ (fp16 + fp32 in fp32, one rounding) and ncthw_to_nthwc with `scale` (one fp32 multiply, one rounding)."""
    from viewcrafter_amd import ops
    h = R.randn((2, 17, 19, 64), 650).half().to(DEV)
    feat = R.randn((2, 64, 17, 19), 651).to(DEV)
    ref = h.double() + feat.double().permute(0, 2, 3, 1)
    R.check_rounding("add_nchw", "2x17x19x64", ops.add_nchw_(h.clone(), feat), ref)
    src = R.randn((2, 8, 7, 17, 19), 652).to(DEV)
    scale = 1.0 / 0.18215
    dst = torch.zeros((2, 7, 17, 19, 8), dtype=torch.float16, device=DEV)
    ops.ncthw_to_nthwc(src, dst, 0, scale=scale)
    scale32 = float(torch.tensor(scale, dtype=torch.float32))                      # the fp32 value the kernel receives
    R.check_rounding("ncthw_to_nthwc", "scale", dst, (src.double() * scale32).permute(0, 2, 3, 4, 1).contiguous())


# ================================================================================================================ attention tier
def to_rows(t):
    """[G, heads, n, d] -> [G * n, heads * d]"""
    G, heads, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(G * n, heads * d).contiguous()


def from_rows(o, G, heads, n, d=64):
    return o.view(G, n, heads, d).permute(0, 2, 1, 3)


def flash_layout(k, v):
    """k, v [Gk, heads, nk, d] -> (K rows, V^T, kv_rows) with zero padding up to a multiple of 8 + 8 rows"""
    Gk, heads, nk, d = k.shape
    kv_rows = (nk + 7) // 8 * 8 + 8
    kd, vtd = kv_layout(k.permute(0, 2, 1, 3).reshape(Gk, nk, heads * d), v.permute(0, 2, 1, 3).reshape(Gk, nk, heads * d), kv_rows, 0.0, 0.0)
    return kd, vtd, kv_rows


def flash_run(q, k, v, *, log2, accumulate_into=None, scale=0.125):
    """One vcx_attn_flash_d64_f16 call on q [G, heads, nq, 64] (the operand as stored: already scaled for LOG2_LOGITS), k / v [G, heads, nk, 64]."""
    from viewcrafter_amd import ops
    G, heads, nq, _ = q.shape
    nk, C = k.shape[2], heads * 64
    kd, vtd, kv_rows = flash_layout(k, v)
    out = accumulate_into if accumulate_into is not None else torch.empty((G * nq, C), dtype=torch.float16, device=DEV)
    ops.flash_attn(to_rows(q).to(DEV), kd, vtd, out, n_groups=G, heads=heads, nq=nq, nk=nk, kv_rows=kv_rows, kv_div=1, ldq=C, ldk=C, ldvt=vtd.shape[1], ldo=C,
                   scale=0.0 if log2 else scale, log2_logits=log2, accumulate=accumulate_into is not None)
    torch.cuda.synchronize()
    return out


def part(q, k, v, log2, scale=0.125, mask=None, add=None):
    """The argument tuple of rounding_quality.attn_exact / attn_model on the GPU."""
    return (q.to(DEV), k.to(DEV), v.to(DEV), 1.0 if log2 else scale, log2, mask, add)


@pytest.mark.parametrize("gain", [1.0, 4.0])
@pytest.mark.parametrize("nk", [77, 256, 1024])
@pytest.mark.parametrize("log2", [False, True])
@pytest.mark.parametrize("qb", [1, 2])
def test_flash_d64_phased_kernel_against_its_model(qb, log2, nk, gain):
    """csrc/attention.hip flash_d64_kernel at FLASH_QB 1 and 2, plain and LOG2_LOGITS, 2 groups x 2 heads, nq = 128."""
    q, k, v = R.flash_problem(2, 2, 128, nk, gain, 700 + nk)
    if log2:
        q = R.log2_q(q, 0.125)
    with knobs(FLASH_IMPL=1, FLASH_QB=qb):
        out = flash_run(q, k, v, log2=log2)
    pt = part(q, k, v, log2)
    ref = R.attn_exact(*pt)[0]
    R.check_rounding("flash_d64", f"qb{qb}{'_log2' if log2 else ''}_nk{nk}_gain{gain:g}", from_rows(out, 2, 2, 128).contiguous(), ref,
                     e_model=R.model_E(R.attn_model("flash_d64", [pt]), ref))


@pytest.mark.parametrize("gain", [1.0, 4.0])
def test_flash_d64_v2_kernel_against_its_model(gain):
    """csrc/attention_v2.hip (FLASH_IMPL 2) at nk = 4096, nq = 64; 4 groups x 2 heads."""
    q, k, v = R.flash_problem(4, 2, 64, 4096, gain, 720)
    q = R.log2_q(q, 0.125)
    with knobs(FLASH_IMPL=2):
        out = flash_run(q, k, v, log2=True)
    with knobs(FLASH_IMPL=1):
        assert not torch.equal(flash_run(q, k, v, log2=True), out), "FLASH_IMPL 2 ran the phased kernel"
    pt = part(q, k, v, True)
    ref = R.attn_exact(*pt)[0]
    R.check_rounding("flash_d64_v2", f"nk4096_gain{gain:g}", from_rows(out, 4, 2, 64).contiguous(), ref, e_model=R.model_E(R.attn_model("flash_d64_v2", [pt]), ref))


@pytest.mark.parametrize("qb", [1, 2])
@pytest.mark.parametrize("gain", [1.0, 4.0])
@pytest.mark.parametrize("nk1,nk2", R.ACCUMULATE_CASES)
def test_flash_d64_accumulate_against_its_model(nk1, nk2, qb, gain):
    """VCX_ATTN_ACCUMULATE: fp16(fp16(o1) + o2) - the read-back rounding is documented (include/vcx.h: 'adds into O')."""
    q, k1, v1, k2, v2 = R.accumulate_problem(nk1, nk2, gain)
    with knobs(FLASH_IMPL=1, FLASH_QB=qb):
        out = flash_run(q, k2, v2, log2=False, accumulate_into=flash_run(q, k1, v1, log2=False))
    parts = [part(q, k1, v1, False), part(q, k2, v2, False)]
    ref = R.attn_exact(*parts[0])[0] + R.attn_exact(*parts[1])[0]
    R.check_rounding("flash_d64_accumulate", f"qb{qb}_{nk1}+{nk2}_gain{gain:g}", from_rows(out, 2, 2, 128).contiguous(), ref,
                     e_model=R.model_E(R.attn_model("flash_d64_accumulate", parts), ref))


DUAL_FORMS = {"flash_dual_qb1": dict(XATTN_RESIDENT=0, FLASH_QB=1), "flash_dual_qb2": dict(XATTN_RESIDENT=0, FLASH_QB=2),
              "xattn_resident": dict(XATTN_RESIDENT=2), "xattn_resident2": dict(XATTN_RESIDENT=1)}


@pytest.mark.parametrize("log2", [False, True])
@pytest.mark.parametrize("form,gain", [(f, g) for f in sorted(DUAL_FORMS) for g in R.DUAL_GAINS[f]])
def test_dual_cross_attention_against_its_model(form, log2, gain):
    """vcx_attn_flash_dual_d64_f16: the dual form of the flash kernel at one and two query blocks per wave and both LDS-resident forms;
    77 + 256 keys shared by the T = 2 frames of each of 2 videos, 2 heads, nq = 128.  With one query block per wave the first partial
    result stays in fp32; the other three keep it as packed fp16 (include/vcx.h; rounding_quality.MODELS; logit gains: DUAL_GAINS there)."""
    from viewcrafter_amd import ops
    B, T, heads, nq, (nk1, nk2) = 2, 2, 2, 128, R.DUAL_KEYS
    G, C = B * T, heads * 64
    q, k1, v1, k2, v2 = R.dual_problem(gain, B, T, heads, nq)
    if log2:
        q = R.log2_q(q, 0.125)
    k1d, vt1, r1 = flash_layout(k1, v1)
    k2d, vt2, r2 = flash_layout(k2, v2)
    out = torch.empty((G * nq, C), dtype=torch.float16, device=DEV)
    with knobs(**DUAL_FORMS[form]):
        ops.flash_attn_dual(to_rows(q).to(DEV), k1d, vt1, k2d, vt2, out, n_groups=G, heads=heads, nq=nq, nk1=nk1, kv_rows1=r1, kv_div1=T, ldk1=C, ldvt1=B * r1,
                            nk2=nk2, kv_rows2=r2, kv_div2=T, ldk2=C, ldvt2=B * r2, ldq=C, ldo=C, scale=0.125, log2_logits=log2)
    rep = lambda t: t.repeat_interleave(T, 0)
    parts = [part(q, rep(k1), rep(v1), log2), part(q, rep(k2), rep(v2), log2)]
    ref = R.attn_exact(*parts[0])[0] + R.attn_exact(*parts[1])[0]
    R.check_rounding(form, f"{'log2_' if log2 else ''}77+256_gain{gain:g}", from_rows(out, G, heads, nq).contiguous(), ref,
                     e_model=R.model_E(R.attn_model(form, parts), ref))


@pytest.mark.parametrize("n", [256, 135])
def test_flash_d512_against_its_model(n):
    from viewcrafter_amd import ops
    G, C = 2, 512
    q, k, v = R.flash_problem(G, 1, n, n, 1.0, 900 + n, d=512)
    kd, vtd, kv_rows = flash_layout(k, v)
    out = torch.empty((G * n, C), dtype=torch.float16, device=DEV)
    ops.flash_attn_d512(to_rows(q).to(DEV), kd, vtd, out, n_groups=G, nq=n, nk=n, kv_rows=kv_rows, ldq=C, ldk=C, ldvt=vtd.shape[1], ldo=C, scale=C ** -0.5)
    pt = part(q, k, v, False, scale=float(torch.tensor(C ** -0.5, dtype=torch.float32)))
    ref = R.attn_exact(*pt)[0]
    R.check_rounding("flash_d512", f"n{n}", from_rows(out, G, 1, n, d=512).contiguous(), ref, e_model=R.model_E(R.attn_model("flash_d512", [pt]), ref))


@pytest.mark.parametrize("T", sorted(R.TEMPORAL_CASES))
@pytest.mark.parametrize("causal", [False, True])
def test_temporal_attention_against_its_model(T, causal):
    """vcx_attn_temporal_d64[_masked]_f16 on both sides of the one-tile / 2 x 2-tile switch at 32 frames: unnormalised P in fp16, the fp32
    result scaled by 1 / l, one output rounding."""
    from viewcrafter_amd import ops
    B, P, heads = 1, R.TEMPORAL_CASES[T], 2
    C = heads * 64
    q, k, v = R.temporal_problem(B, T, P, heads, 1000 + T)
    qkv = torch.cat([t.reshape(B * T * P, C) for t in (q, k, v)], dim=1).contiguous().to(DEV)
    out = torch.empty((B * T * P, C), dtype=torch.float16, device=DEV)
    ops.temporal_attn(qkv, out, B=B, T=T, P=P, heads=heads, ld=3 * C, k_off=C, v_off=2 * C, ldo=C, scale=0.125, causal=causal)
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool, device=DEV)) if causal else None
    pt = part(R.temporal_split(q), R.temporal_split(k), R.temporal_split(v), False, mask=mask)
    ref = R.attn_exact(*pt)[0]
    R.check_rounding("temporal_d64", f"T{T}{'_causal' if causal else ''}", out, R.temporal_merge(ref), e_model=R.model_E(R.temporal_merge(R.attn_model("temporal_d64", [pt])), R.temporal_merge(ref)))


@pytest.mark.parametrize("T", sorted(R.TEMPORAL_REL_CASES))
@pytest.mark.parametrize("causal", [False, True])
def test_temporal_attention_with_relative_position_against_its_models(T, causal):
    """vcx_attn_temporal_d64_rel_f16: o and relp separately.  o: the temporal model with relg added to the logits; relp: P16 / l by
    clipped distance, inner slots rounded once more, end slots summed in fp32 and rounded; the slots beyond 2 R stay zero."""
    from viewcrafter_amd import ops
    P, Rr = R.TEMPORAL_REL_CASES[T]
    B, heads = 1, 2
    C, tokens = heads * 64, B * T * P
    q, k, v = R.temporal_problem(B, T, P, heads, 1100 + T)
    relg = (R.randn((B, T, P, heads, 64), 1200 + T) * 4).half()
    qkv = torch.cat([t.reshape(tokens, C) for t in (q, k, v)], dim=1).contiguous().to(DEV)
    out = torch.empty((tokens, C), dtype=torch.float16, device=DEV)
    relp = torch.zeros((tokens, heads, 64), dtype=torch.float16, device=DEV)
    ops.temporal_attn_rel(qkv, out, relg.reshape(tokens, heads, 64).to(DEV), relp, R=Rr, B=B, T=T, P=P, heads=heads, ld=3 * C, k_off=C, v_off=2 * C, ldo=C,
                          scale=0.125, causal=causal)
    qs, ks, vs, gs = [R.temporal_split(t).to(DEV) for t in (q, k, v, relg)]
    idx = R.rel_index(T, Rr, DEV).expand(qs.shape[:-2] + (T, T))
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool, device=DEV)) if causal else None
    pt = (qs, ks, vs, 0.125, False, mask, torch.gather(gs.double(), -1, idx))
    ref = R.temporal_merge(R.attn_exact(*pt)[0])
    case = f"T{T}_R{Rr}{'_causal' if causal else ''}"
    R.check_rounding("temporal_d64_rel", case, out, ref, e_model=R.model_E(R.temporal_merge(R.attn_model("temporal_d64", [pt])), ref))
    pref, pmodel = R.relp_ref_and_model(qs, ks, gs, Rr, 0.125, causal)                      # [B, P, heads, T, 2R + 1]
    slots = lambda t: t.permute(0, 3, 1, 2, 4).reshape(tokens, heads, 2 * Rr + 1)
    assert bool((relp[:, :, 2 * Rr + 1:] == 0).all())
    R.check_rounding("temporal_d64_relp", case, relp[:, :, :2 * Rr + 1].contiguous(), slots(pref), e_model=R.model_E(slots(pmodel), slots(pref)))


# ================================================================================================================ DDIM step against fp64
def _ddim_case(branch, B, n, offset=0.0):
    from viewcrafter_amd import ops
    coef, uncond, img, cfg_img, noise = R.DDIM_BRANCHES[branch]
    x, vc, vu, vi, nz = [t.to(DEV) for t in R.ddim_problem(B, n, 1300 + n, offset)]
    args = (x, vc, vu if uncond else None, nz if noise else None, coef)
    kw = dict(v_img=vi if img else None, cfg_img=cfg_img)
    got = ops.ddim_step(*args, **kw)
    ref = R.ddim_ref(*args, **kw)
    f32 = R.ddim_ref(*args, dtype=torch.float32, **kw)
    for what, g, r, f in zip(("x_prev", "pred_x0"), got, ref, f32):
        err, err32 = float((g.double() - r).abs().max()), float((f.double() - r).abs().max())
        bound = 4 * err32 + 4 * 2.0 ** -23 * float(r.abs().max())
        print(f"\n[ddim] {branch} B {B} n {n} offset {offset:g} {what}: err {err:.3e} fp32 torch form {err32:.3e} bound {bound:.3e}")
        assert torch.isfinite(g).all() and err <= bound, f"ddim {branch} B {B} n {n} offset {offset:g} {what}: max |err vs fp64| {err:.3e} > {bound:.3e} = 4 x {err32:.3e} (fp32 torch form) + 4 fp32 ulps"


@pytest.mark.parametrize("B,n", R.DDIM_SIZES)
@pytest.mark.parametrize("branch", sorted(R.DDIM_BRANCHES))
def test_ddim_step_against_fp64_on_every_branch(branch, B, n):
    """vcx_ddim_step3_f32 (vcx_ddim_step_f32 is its v_img = NULL form): no guidance, CFG and multi-condition guidance with rescale 0 / 0.7,
    eps-parameterisation, noise, sigma = 0 with a noise pointer, scale_ratio != 1; n = 65536 + 3 takes a second trip of the reduction's
    stride loop and a ragged last block; the samples have different standard deviations.  Bound: 4 x the error of the plain fp32 torch
    form in the same run + 4 fp32 ulps of max |ref|."""
    _ddim_case(branch, B, n)


@pytest.mark.parametrize("branch", ["cfg_rescale", "multicond_rescale"])
def test_ddim_step_with_a_common_offset_of_ten_standard_deviations(branch):
    """v_cond / v_uncond / v_img share an offset of 10 standard deviations: torch.std (the reference's rescale_noise_cfg) is robust to it;
    the kernel's sums of squares must be too."""
    _ddim_case(branch, 3, 65536 + 3, offset=10.0)
