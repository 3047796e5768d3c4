"""tests/rounding_quality.py on the CPU: the plain fp32 torch form of every case family of tests/test_rounding_gpu.py stays inside the
bound on the very inputs the GPU tests use (the reference alone passes), three planted defects fail it (the bound has teeth), and the
rounding-point models of the attention kernels stay below their cap and apart from a variant with one more rounding."""
import math

import pytest
import torch

from tests import rounding_quality as R


def E_of(out_f16, ref64):
    st = R.rounding_stats(out_f16, ref64)
    assert st["n"] >= R.N_MIN
    return st


def test_rounding_stats_of_the_correctly_rounded_result_and_of_a_shifted_one():
    ref = R.randn((256, 200), 1).double()
    st = R.rounding_stats(ref.half(), ref)
    assert st["E"] == 1.0 and st["mismatch"] == 0.0 and st["worst"] <= 0.5 and st["n"] == 51200
    # an extra error of d = 0.25 ulp16 of uniform sign on values in [1, 2): E^2 = 1 + 12 d^2 = 1.75
    ref = 1.0 + torch.rand((256, 200), generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 0.999
    sign = torch.where(torch.rand((256, 200), generator=torch.Generator().manual_seed(3)) < 0.5, -1.0, 1.0).double()
    shifted = ref + sign * 0.25 * 2.0 ** -10
    e = R.rounding_stats(shifted.half(), ref)["E"]
    # rounding a value moved by d: the error is uniform rounding noise + d, independent for a continuous value
    assert abs(e * e - 1.75) <= 0.05, e
    bad = ref.half().clone()
    bad[3, 5] = float("nan")
    assert R.rounding_stats(bad, ref)["E"] == float("inf")


@pytest.mark.parametrize("name", sorted(R.LINEAR_CASES) + ["ws_" + k for k in sorted(R.WS_CASES)])
def test_fp32_linear_reference_is_inside_the_bound(name):
    c = R.WS_CASES[name[3:]] if name.startswith("ws_") else R.LINEAR_CASES[name]
    p = R.lin_problem(c)
    st = E_of(R.lin_ref(c, p, torch.float32).half(), R.lin_ref(c, p))
    print(f"\n[rounding cpu] linear {name} E {st['E']:.6f} mismatch {100 * st['mismatch']:.3f} %")
    assert st["E"] <= R.E_BOUND and st["mismatch"] <= R.MISMATCH_CAP
    # OUT_F32: the fp32 result itself inside the summation-order bound
    if name in ("bias_residual_k64", "bias_residual_k1280"):
        err = (R.lin_ref(c, p, torch.float32).double() - R.lin_ref(c, p)).abs()
        assert bool((err <= R.lin_f32_bound(c, p)).all())


@pytest.mark.parametrize("name", sorted(R.GEGLU_CASES))
def test_fp32_geglu_and_lnfold_references_are_inside_the_bound(name):
    M, K, D = R.GEGLU_CASES[name]
    p = R.geglu_problem(M, K, D, 300)
    h32 = p["x"].float() @ p["w"].float().t() + p["bias"]
    h64 = p["x"].double() @ p["w"].double().t() + p["bias"].double()
    st = E_of(R.geglu_ref(h32, torch.float32).half(), R.geglu_ref(h64))
    print(f"\n[rounding cpu] geglu {name} E {st['E']:.6f}")
    assert st["E"] <= R.E_BOUND and st["mismatch"] <= R.MISMATCH_CAP
    # the defect of the issue: GEGLU formed from fp16-rounded halves
    a, g = h32.half().float().chunk(2, dim=-1)
    bad = (a * torch.nn.functional.gelu(g)).half()
    assert R.rounding_stats(bad, R.geglu_ref(h64))["E"] > R.E_BOUND


@pytest.mark.parametrize("name", sorted(R.LNFOLD_CASES))
def test_fp32_lnfold_reference_is_inside_the_bound(name):
    M, N, K, alpha, offset = R.LNFOLD_CASES[name]
    p = R.lnfold_problem(M, N, K, offset, 400)
    st32 = R.row_stats_f32(p["x"])
    st = E_of(R.lnfold_ref(p, st32, alpha, torch.float32).half(), R.lnfold_ref(p, st32, alpha))
    print(f"\n[rounding cpu] lnfold {name} E {st['E']:.6f}")
    assert st["E"] <= R.E_BOUND and st["mismatch"] <= R.MISMATCH_CAP


@pytest.mark.parametrize("name", sorted(R.CONV_CASES))
def test_fp32_conv2d_is_inside_the_bound_and_the_tap_loop_is_conv2d(name):
    c = R.CONV_CASES[name]
    p = R.conv_problem(c, 500)
    ref = R.conv_ref(c, p)
    y32 = R.conv_f32(c, p)
    assert tuple(ref.shape) == tuple(y32.shape)
    st = E_of(y32.half(), ref)
    print(f"\n[rounding cpu] conv {name} E {st['E']:.6f}")
    assert st["E"] <= R.E_BOUND and st["mismatch"] <= R.MISMATCH_CAP


def test_fp32_norms_and_softmax_are_inside_the_bound():
    for name, (n, pix, C, eps) in R.GROUPNORM_CASES.items():
        p = R.gn_problem(n, pix, C, 600)
        stats = R.gn_stats_f32(p["x"])
        for silu in (False, True):
            st = E_of(R.gn_ref(p["x"], stats, p["gamma"], p["beta"], eps, silu, torch.float32).half(), R.gn_ref(p["x"], stats, p["gamma"], p["beta"], eps, silu))
            print(f"\n[rounding cpu] groupnorm {name} silu {silu} E {st['E']:.6f}")
            assert st["E"] <= R.E_BOUND and st["mismatch"] <= R.MISMATCH_CAP
    n, pix, C, N, eps = R.GN_FOLD
    stats = R.gn_stats_f32(R.gn_problem(n, pix, C, 610)["x"])
    w32, gamma = R.randn((N, C), 611, C ** -0.5), 1 + 0.3 * R.randn((C,), 612)
    st = E_of(R.gn_fold_wn_ref(w32, gamma, stats, eps, torch.float32).half(), R.gn_fold_wn_ref(w32, gamma, stats, eps))
    assert st["E"] <= R.E_BOUND
    for C, rows in R.LAYERNORM_CASES.items():
        p = R.ln_problem(rows, C, 620)
        st = E_of(torch.nn.functional.layer_norm(p["x"].float(), (C,), p["gamma"], p["beta"], 1e-5).half(), R.ln_ref(p))
        print(f"\n[rounding cpu] layernorm C {C} E {st['E']:.6f}")
        assert st["E"] <= R.E_BOUND and st["mismatch"] <= R.MISMATCH_CAP
    for n, (rows, ld) in R.SOFTMAX_CASES.items():
        x = (R.randn((rows, ld), 630) * 3).half()
        st = E_of(x[:, :n].float().softmax(-1).half(), x[:, :n].double().softmax(-1))
        print(f"\n[rounding cpu] softmax n {n} E {st['E']:.6f}")
        assert st["E"] <= R.E_BOUND and st["mismatch"] <= R.MISMATCH_CAP


@pytest.mark.parametrize("K", [320, 1280, 2880])
def test_the_three_planted_defects_fail_the_bound_that_the_fp32_form_passes(K):
    """A 256 x 320 linear layer with bias and residual: fp32 accumulate + one rounding passes; the result rounded before the residual is
    added, the accumulator rounded after every 64-wide K slab, and a final conversion toward zero each fail - all three pass the
    rel-L2 <= 2e-3 of tests/test_kernels_gpu.py."""
    c = R.lin(256, 320, K, seed=90)
    p = R.lin_problem(c)
    ref = R.lin_ref(c, p)
    good = E_of(R.lin_ref(c, p, torch.float32).half(), ref)
    assert good["E"] <= R.E_BOUND and good["mismatch"] <= R.MISMATCH_CAP
    rel = lambda o: float((o.double() - ref).norm() / ref.norm())
    for name, fn, e_min in (("second rounding", R.defect_second_rounding, 1.25), ("slab rounding", R.defect_slab_rounding, 1.3), ("truncation", R.defect_truncation, 1.9)):
        out = fn(c, p)
        st = R.rounding_stats(out, ref)
        print(f"\n[rounding cpu] K {K} {name}: E {st['E']:.3f} mismatch {100 * st['mismatch']:.1f} % rel-L2 {rel(out):.2e} (fp32 form: E {good['E']:.7f} mismatch {100 * good['mismatch']:.2f} %)")
        assert st["E"] > e_min > R.E_BOUND and st["mismatch"] > 2 * R.MISMATCH_CAP, (name, st)
        assert rel(out) <= 2e-3, "the planted defect is meant to pass today's acceptance rule"
        with pytest.raises(AssertionError, match="excess-error ratio .* elements wrong; first at"):
            R.check_rounding("planted", name, out, ref)
        R.RECORD.pop()


# ------------------------------------------------------------------------------------------------------------------ attention models
def _flash_cases():
    return [(nk, gain) for nk in (77, 256, 1024) for gain in (1.0, 4.0)]


@pytest.mark.parametrize("nk,gain", _flash_cases())
def test_flash_models_stay_below_their_cap_and_apart_from_one_more_rounding(nk, gain):
    """At each flash case's shape: E of the model (unnormalised P in fp16, fp32 row sum, one output rounding) <= 1.45, the exact softmax with
    one rounding is 1; one more rounding point is at least 10 % worse than the model (a kernel is allowed 5 %), and normalising the
    probabilities BEFORE packing them is measurably worse than the exact-maximum form (with the deferred maximum the two are level at
    flat softmaxes: both then round numbers with full mantissas)."""
    q, k, v = R.flash_problem(2, 2, 128, nk, gain, 700 + nk)
    part = (q, k, v, 0.125, False, None, None)
    ref = R.attn_exact(*part)[0]
    e_model = R.model_E(R.attn_model("flash_d64", [part]), ref)
    e_norm = R.model_E(R.attn_model("flash_d64", [part], normalise_first=True), ref)
    e_exact = R.model_E(R.attn_model("flash_d64", [part], p16=False), ref)
    print(f"\n[rounding cpu] flash nk {nk} gain {gain}: E_model {e_model:.3f}  normalised-before-packing {e_norm:.3f}  exact {e_exact:.3f}")
    assert e_exact == 1.0
    e_exact_max = R.model_E(R.attn_model("flash_d64", [part], defer=None), ref)
    print(f"[rounding cpu] ... with the exact row maximum in place of the deferred one: {e_exact_max:.3f}")
    assert 1.0 < e_exact_max <= e_model * 1.001 <= R.E_MODEL_CAP
    e_extra = R.model_E(R.attn_model("flash_d64", [part], extra_rounding=True), ref)
    print(f"[rounding cpu] ... with one more rounding (P16 V to fp16 before 1 / l): {e_extra:.3f}")
    assert e_extra > e_model * 1.1 and e_norm > e_exact_max * 1.02, "the model cannot tell one more rounding"


@pytest.mark.parametrize("gain", [1.0, 4.0])
@pytest.mark.parametrize("nk1,nk2", R.ACCUMULATE_CASES)
def test_accumulate_model(nk1, nk2, gain):
    q, k1, v1, k2, v2 = R.accumulate_problem(nk1, nk2, gain)
    parts = [(q, k1, v1, 0.125, False, None, None), (q, k2, v2, 0.125, False, None, None)]
    ref = R.attn_exact(*parts[0])[0] + R.attn_exact(*parts[1])[0]
    e_model, e_fp32 = R.model_E(R.attn_model("flash_d64_accumulate", parts), ref), R.model_E(R.attn_model("flash_d64_accumulate", parts, readback=False), ref)
    e_extra = R.model_E(R.attn_model("flash_d64_accumulate", parts, extra_rounding=True), ref)
    print(f"\n[rounding cpu] accumulate {nk1}+{nk2} gain {gain}: E_model {e_model:.3f}  without the read-back rounding {e_fp32:.3f}  one more rounding {e_extra:.3f}")
    assert 1.0 < e_fp32 < e_model <= R.E_MODEL_CAP and e_extra > e_model * 1.1


@pytest.mark.parametrize("gain", [1.0, 4.0, 6.0])
@pytest.mark.parametrize("log2", [False, True])
def test_dual_models(log2, gain):
    """The dual forms: first half kept in fp32 (one query block per wave) against packed fp16 (the other three) - the two models differ
    by more than the 5 % a kernel is allowed over its own, so a kernel cannot pass under the wrong one; every model under the cap at the
    gains the GPU test uses for it (DUAL_GAINS); the others are printed."""
    q, k1, v1, k2, v2 = R.dual_problem(gain)
    if log2:
        q = R.log2_q(q, 0.125)
    rep = lambda t: t.repeat_interleave(2, 0)
    c = (1.0, True) if log2 else (0.125, False)
    parts = [(q, rep(k1), rep(v1)) + c + (None, None), (q, rep(k2), rep(v2)) + c + (None, None)]
    ref = R.attn_exact(*parts[0])[0] + R.attn_exact(*parts[1])[0]
    e = {f: R.model_E(R.attn_model(f, parts), ref) for f in R.DUAL_GAINS}
    assert all(R.model_E(R.attn_model(f, parts, extra_rounding=True), ref) > 1.1 * e[f] for f in e)
    print(f"\n[rounding cpu] dual 77+256 log2 {log2} gain {gain}: " + "  ".join(f"{f} {v:.3f}" for f, v in e.items()))
    assert e["flash_dual_qb2"] == e["xattn_resident"] and min(e["flash_dual_qb2"], e["xattn_resident2"]) > e["flash_dual_qb1"] * R.E_BOUND
    for f, gains in R.DUAL_GAINS.items():
        if gain in gains:
            assert 1.0 < e[f] <= R.E_MODEL_CAP, (f, e[f])


@pytest.mark.parametrize("gain", [1.0, 4.0])
def test_v2_model(gain):
    """The software-pipelined kernel's case: 4096 keys, 64 queries, base-2 logits; the two 32-row query blocks of a wave vote together."""
    q, k, v = R.flash_problem(4, 2, 64, 4096, gain, 720)
    part = (R.log2_q(q, 0.125), k, v, 1.0, True, None, None)
    ref = R.attn_exact(*part)[0]
    e_model, e_extra = R.model_E(R.attn_model("flash_d64_v2", [part]), ref), R.model_E(R.attn_model("flash_d64_v2", [part], extra_rounding=True), ref)
    print(f"\n[rounding cpu] v2 nk 4096 gain {gain}: E_model {e_model:.3f}  one more rounding {e_extra:.3f}")
    assert 1.0 < e_model <= R.E_MODEL_CAP and e_extra > e_model * 1.1


@pytest.mark.parametrize("nk", [256, 135])
def test_d512_model(nk):
    q, k, v = R.flash_problem(2, 1, nk, nk, 1.0, 900 + nk, d=512)
    part = (q, k, v, 512 ** -0.5, False, None, None)
    ref = R.attn_exact(*part)[0]
    e_model, e_extra = R.model_E(R.attn_model("flash_d512", [part]), ref), R.model_E(R.attn_model("flash_d512", [part], extra_rounding=True), ref)
    print(f"\n[rounding cpu] d512 nk {nk}: E_model {e_model:.3f}  one more rounding {e_extra:.3f}")
    assert 1.0 < e_model <= R.E_MODEL_CAP and e_extra > e_model * 1.1


@pytest.mark.parametrize("T", sorted(R.TEMPORAL_CASES))
@pytest.mark.parametrize("causal", [False, True])
def test_temporal_models(T, causal):
    P = R.TEMPORAL_CASES[T]
    q, k, v = [R.temporal_split(t) for t in R.temporal_problem(1, T, P, 2, 1000 + T)]
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool)) if causal else None
    part = (q, k, v, 0.125, False, mask, None)
    ref = R.attn_exact(*part)[0]
    e_model, e_norm = R.model_E(R.attn_model("temporal_d64", [part]), ref), R.model_E(R.attn_model("temporal_d64", [part], normalise_first=True), ref)
    print(f"\n[rounding cpu] temporal T {T} causal {causal}: E_model {e_model:.3f}  normalised-before-packing {e_norm:.3f}")
    e_extra = R.model_E(R.attn_model("temporal_d64", [part], extra_rounding=True), ref)
    assert 1.0 < e_model <= R.E_MODEL_CAP and e_norm > e_model * 1.1 and e_extra > e_model * 1.1
    if T in R.TEMPORAL_REL_CASES:
        P, Rr = R.TEMPORAL_REL_CASES[T]
        q, k, _ = [R.temporal_split(t) for t in R.temporal_problem(1, T, P, 2, 1100 + T)]
        relg = R.temporal_split((R.randn((1, T, P, 2, 64), 1200 + T) * 4).half())
        ref, model = R.relp_ref_and_model(q, k, relg, Rr, 0.125, causal)
        assert ref.numel() >= R.N_MIN
        e_relp = R.model_E(model, ref)
        print(f"[rounding cpu] temporal relp T {T} R {Rr} causal {causal}: E_model {e_relp:.3f}")
        assert 1.0 < e_relp <= R.E_MODEL_CAP
        assert bool(((ref.sum(-1) - 1).abs() < 1e-12).all())


def test_every_attention_kernel_has_its_rounding_points_with_source_lines():
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "viewcrafter_amd")
    lines = {f: open(os.path.join(root, "csrc", f)).read().splitlines() for f in ("attention.hip", "attention_v2.hip")}
    assert set(R.MODEL_POINTS) <= set(R.MODELS)
    for kernel, points in R.MODELS.items():
        assert points, kernel
        for what, where in points:
            m = re.match(r"csrc/(attention(?:_v2)?\.hip):(\d+)(?:-(\d+))?", where)
            assert m, (kernel, where)
            text = " ".join(lines[m.group(1)][int(m.group(2)) - 1:int(m.group(3) or m.group(2))])
            # a rounding point is a conversion to fp16 (or, where the point is 'kept in fp32', the line that keeps it)
            assert re.search(r"half_t|V_PACK|keep|inv|old|DEFER", text), f"{kernel}: {where} is not a rounding point: {text.strip()}"


# ------------------------------------------------------------------------------------------------------------------ DDIM
@pytest.mark.parametrize("branch", sorted(R.DDIM_BRANCHES))
def test_ddim_fp64_reference_against_the_fp32_form(branch):
    """ddim_ref in fp32 against itself in fp64 on every branch: the fp32 form's own error - what scales the GPU test's bound - is a few
    fp32 ulps of the result, and the branches really differ."""
    coef, uncond, img, cfg_img, noise = R.DDIM_BRANCHES[branch]
    x, vc, vu, vi, nz = R.ddim_problem(3, 257, 1300)
    args = (x, vc, vu if uncond else None, nz if noise else None, coef)
    kw = dict(v_img=vi if img else None, cfg_img=cfg_img)
    xp64, x064 = R.ddim_ref(*args, **kw)
    xp32, x032 = R.ddim_ref(*args, dtype=torch.float32, **kw)
    assert xp64.dtype == torch.float64 and xp32.dtype == torch.float32
    for a, b in ((xp32, xp64), (x032, x064)):
        assert float((a.double() - b).abs().max()) <= 64 * 2.0 ** -24 * float(b.abs().max())
    base = R.ddim_ref(x, vc, vu, None, R.DDIM_BRANCHES["cfg_rescale"][0])[0]
    if branch not in ("cfg_rescale", "sigma0_with_noise_pointer"):
        assert float((xp64 - base).abs().max()) > 1e-3
    else:
        assert torch.equal(xp64, base)          # sigma = 0: a noise pointer changes nothing
    assert math.isfinite(float(xp64.abs().max()))
