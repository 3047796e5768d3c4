"""Every attention kernel at every pitch, offset and alignment its front end accepts (tests/attn_layouts.py: the LAYOUTS table and the
assertions a - d; tests/test_attn_layouts_cpu.py shows on stand-ins that they reject a store tail that ignores ldo or the column offset, a
fetch that ignores k_off or runs past a row's width, and a write past the window).

Seven kernels compute a store address from ldo and fetch Q / K / V^T with code of their own - the phased flash kernel (one and two query
blocks per wave, plain and base-2 logits, accumulate, dual), the software-pipelined one, the two LDS-resident dual forms, d512, temporal
up to and beyond 32 frames (causal, relative position), the MXFP8 twins, the row softmax.  The rest of the suite passes them ldo = 64 heads,
o at column 0, ld = 3 D, k_off = D, v_off = 2 D.  Here each runs with its operands and its output as windows of wider, NaN- / sentinel-filled
buffers.  The shapes are those of tests/test_exact_gpu.py: the smallest that reach each kernel's tile loop and ragged tail.
"""
import pytest
import torch

from tests import attn_layouts as A
from tests import exact_inputs as X
from tests import mx_emulation as MX
from tests.test_exact_gpu import FLASH_IMPLS, dual_sets, flash_call, knobs, kv_layout, log2_q, temporal_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOG2, CAUSAL = 2, 4          # include/vcx.h VCX_ATTN_LOG2_LOGITS, VCX_ATTN_CAUSAL
POISON = 0xAB


# ================================================================================================================ flash d64 / d512
def flash_launch(impl):
    """One vcx_attn_flash_d64_f16 / _d512_f16 call under the knobs of FLASH_IMPLS[impl] ("default": none); the dense control goes through
    tests/test_exact_gpu.py flash_call, as that module's own tests do."""
    def launch(view, ld, o, ldo, geo):
        from viewcrafter_amd import ops
        C = geo["heads"] * geo["d"]
        kw = dict(n_groups=geo["n_groups"], nq=geo["nq"], nk=geo["nk"], kv_rows=geo["kv_rows"])
        with knobs(**FLASH_IMPLS.get(impl, {})):
            if (ld["q"], ld["k"], ld["vt"], ldo) == (C, C, view["vt"].shape[1], C) and not geo["accumulate"]:
                flash_call("d512" if geo["d"] == 512 else impl, view["q"], view["k"], view["vt"], o, G=geo["n_groups"], heads=geo["heads"], nq=geo["nq"], nk=geo["nk"],
                           kv_rows=geo["kv_rows"], kv_div=geo["kv_div"], scale=geo["scale"], log2=geo["log2"])
            elif geo["d"] == 512:
                ops.flash_attn_d512(view["q"], view["k"], view["vt"], o, ldq=ld["q"], ldk=ld["k"], ldvt=ld["vt"], ldo=ldo, scale=geo["scale"], **kw)
            else:
                ops.flash_attn(view["q"], view["k"], view["vt"], o, heads=geo["heads"], kv_div=geo["kv_div"], ldq=ld["q"], ldk=ld["k"], ldvt=ld["vt"], ldo=ldo,
                               scale=0.0 if geo["log2"] else geo["scale"], accumulate=geo["accumulate"], log2_logits=geo["log2"], **kw)
            torch.cuda.synchronize()
    return launch


# (variant, nq, nk, accumulate): heads 2, 4 query groups on 2 key groups (kv_div = 2), kv_rows = nk8 + 16; v2: three 64-key tiles
FLASH_VARIANTS = [("qb1", 100, 135, False), ("qb2", 300, 135, False), ("qb1_log2", 100, 77, False), ("qb2_log2", 300, 200, False), ("v2", 256, 192, False),
                  ("qb1", 100, 135, True)]


@pytest.mark.parametrize("layout", ["wide", "o8"])
@pytest.mark.parametrize("impl,nq,nk,accumulate", FLASH_VARIANTS, ids=[f"{i}{'_accumulate' if a else ''}" for i, _, _, a in FLASH_VARIANTS])
def test_flash_d64_in_every_layout(impl, nq, nk, accumulate, layout):
    """flash_d64_kernel<QB 1 / 2, plain / base-2 logits>, its VCX_ATTN_ACCUMULATE read-back (fp64 reference: no one-hot construction) and
    flash2_d64_kernel: a - d."""
    log2 = impl.endswith("log2") or impl == "v2"
    A.run_checks(A.flash_case(flash_launch(impl), layout, device=DEV, heads=2, Gk=2, kv_div=2, nq=nq, nk=nk, log2=log2, accumulate=accumulate, kv_layout=kv_layout))


@pytest.mark.parametrize("layout", ["wide", "o8"])
@pytest.mark.parametrize("nk,forced", [(1984, 1), (2048, 2)])
def test_flash_d64_on_both_sides_of_the_2048_key_switch_under_the_default_knobs(nk, forced, layout):
    """No knob set: 1984 keys (31 whole tiles) stay on the phased kernel, 2048 go to the software-pipelined one (flash_d64_run) - a - d in both;
    the dense result carries the bits of the kernel the switch should have picked (knob FLASH_IMPL = 1 / 2 on the same operands)."""
    from viewcrafter_amd import ops
    assert ops.tune_get("FLASH_IMPL") == 0 and ops.tune_get("FLASH_QB") == 0
    case = A.flash_case(flash_launch("default"), layout, device=DEV, heads=1, Gk=1, kv_div=1, nq=64, nk=nk, log2=True, kv_layout=kv_layout)
    A.run_checks(case)
    d = case["dense"]
    o = torch.full((64, 64), A.GUARD, dtype=torch.float16, device=DEV)
    with knobs(FLASH_IMPL=forced):
        ops.flash_attn(d.view["q"], d.view["k"], d.view["vt"], o, n_groups=1, heads=1, nq=64, nk=nk, kv_rows=nk + 16, kv_div=1, ldq=d.ld["q"], ldk=d.ld["k"],
                       ldvt=d.ld["vt"], ldo=64, scale=0.0, log2_logits=True)
    A.assert_same_bits(d.o, o, f"default knobs at {nk} keys against FLASH_IMPL = {forced}")


@pytest.mark.parametrize("layout", ["wide", "o8"])
def test_flash_d512_in_every_layout(layout):
    """flash_d512_kernel: 2 groups, 136 queries (one block of 128 + 8), 135 keys (four tiles of 32 + 7): a - d."""
    A.run_checks(A.flash_case(flash_launch("d512"), layout, device=DEV, heads=1, Gk=2, kv_div=1, nq=136, nk=135, d=512, kv_layout=kv_layout))


# ================================================================================================================ dual
DUAL_KNOBS = dict(resident=dict(XATTN_RESIDENT=1), resident_first=dict(XATTN_RESIDENT=2), flash_dual_qb1=dict(XATTN_RESIDENT=0, FLASH_QB=1),
                  flash_dual_qb2=dict(XATTN_RESIDENT=0, FLASH_QB=2), default={})
# form -> (T frames per video, nk1, nk2, nq, base-2 logits): tests/test_exact_gpu.py::test_dual_cross_attention_one_hot_and_poisoned_padding
DUAL_SHAPES = dict(resident=(3, 77, 256, 200, True), resident_first=(3, 77, 256, 200, True), flash_dual_qb1=(1, 77, 16, 100, True), flash_dual_qb2=(1, 77, 16, 300, False))


def dual_geo(T, nk1, nk2, nq, heads=2, B=2):
    return dict(n_groups=B * T, heads=heads, nq=nq, nk1=nk1, kv_rows1=(nk1 + 7) // 8 * 8 + 8, kv_div1=T, nk2=nk2, kv_rows2=(nk2 + 7) // 8 * 8 + 8, kv_div2=T)


def dual_operands(q, k1, v1, k2, v2, geo, log2):
    """q [G nq, C], k / v [B, nk, C] -> the logical operand matrices (padding: K rows NaN, V^T columns >= nk8 NaN, [nk, nk8) finite)"""
    k1d, vt1 = kv_layout(k1, v1, geo["kv_rows1"], A.NAN, A.NAN, X.PAD_FINITE)
    k2d, vt2 = kv_layout(k2, v2, geo["kv_rows2"], A.NAN, A.NAN, X.PAD_FINITE)
    return dict(q=log2_q(q, 0.125) if log2 else q, k1=k1d, vt1=vt1, k2=k2d, vt2=vt2)


def dual_problems(T, nk1, nk2, nq, log2, heads=2, B=2):
    """-> geo, the one-hot operands with (want, bound), N(0, 1) operands"""
    C, G = heads * 64, B * T
    geo = dual_geo(T, nk1, nk2, nq, heads, B)
    q, k1, v1, k2, v2, j1, j2 = dual_sets(nk1, nk2, B, heads, T * nq, seed=nk1 + nk2)
    assert min(X.one_hot_gap(q, k1, j1[:, None, :].expand(B, heads, T * nq), 0.125), X.one_hot_gap(q, k2, j2[:, None, :].expand(B, heads, T * nq), 0.125)) >= X.ONE_HOT_GAP_NATS
    want = torch.stack([v1[b, j1[b]].double() + v2[b, j2[b]].double() for b in range(B)]).reshape(G * nq, C)
    bound = torch.stack([v1[b, j1[b]].double().abs() + v2[b, j2[b]].double().abs() for b in range(B)]).reshape(G * nq, C) * 2.0 ** -10
    hot = dual_operands(q.reshape(G * nq, C), k1.reshape(B, nk1, C), v1.reshape(B, nk1, C), k2.reshape(B, nk2, C), v2.reshape(B, nk2, C), geo, log2)
    g = torch.Generator().manual_seed(nk1 + nk2 + nq)
    r = lambda *s: torch.randn(s, generator=g).half()
    rnd = dual_operands(r(G * nq, C), r(B, nk1, C), r(B, nk1, C), r(B, nk2, C), r(B, nk2, C), geo, log2)
    return geo, hot, want, bound, rnd


def dual_place(layout, operands, geo, log2, kn):
    from viewcrafter_amd import ops
    C = geo["heads"] * 64
    p = A.Placed(layout, operands, torch.full((geo["n_groups"] * geo["nq"], C), A.GUARD, dtype=torch.float16), DEV)
    with knobs(**kn):
        ops.flash_attn_dual(p.view["q"], p.view["k1"], p.view["vt1"], p.view["k2"], p.view["vt2"], p.o, ldk1=p.ld["k1"], ldvt1=p.ld["vt1"], ldk2=p.ld["k2"],
                            ldvt2=p.ld["vt2"], ldq=p.ld["q"], ldo=p.ldo, scale=0.125, log2_logits=log2, **geo)
        torch.cuda.synchronize()
    return p


def dual_check(form, layout, kn_strided, kn_dense):
    T, nk1, nk2, nq, log2 = DUAL_SHAPES[form]
    geo, hot_ops, want, bound, rnd = dual_problems(T, nk1, nk2, nq, log2)
    hot = dual_place(layout, hot_ops, geo, log2, kn_strided)
    dense, strided = dual_place("dense", rnd, geo, log2, kn_dense), dual_place(layout, rnd, geo, log2, kn_strided)
    X.assert_elementwise(hot.o, want, bound, f"dual one-hot {form}, layout {layout}")                                   # a
    A.assert_same_bits(strided.o, dense.o, f"dual {form}, layout {layout}")                                             # b
    for p in (hot, dense, strided):
        p.check_c()
        p.check_d()
    return strided


# (resident, o8) is the next test: with o at 8 bytes the front end itself leaves the second form
@pytest.mark.parametrize("form,layout", [(f, l) for f in DUAL_SHAPES for l in ("wide", "o8") if (f, l) != ("resident", "o8")])
def test_dual_in_every_layout(form, layout):
    """vcx_attn_flash_dual_d64_f16: the second-form resident kernel (16-byte buffer stores, 32-bit qrow * ldo offsets), the first form (knob
    XATTN_RESIDENT = 2) and the dual instantiations of the phased kernel with one and two query blocks per wave: one-hot in both key
    sets, O_i = V1[j1(i)] + V2[j2(i)] within 2^-10 (|v1| + |v2|); b - d."""
    dual_check(form, layout, DUAL_KNOBS[form], DUAL_KNOBS[form])


def test_dual_under_the_default_knob_picks_the_first_form_for_an_8_byte_aligned_output():
    """Layout o8 with NO knob set must run and be right: dual_kernel_choice has to leave the second-form resident kernel - its 16-byte
    stores need ldo % 8 == 0 and o 16-byte aligned - for the first form by itself.  Its bits are compared with the dense call under knob
    XATTN_RESIDENT = 2, which forces that same first-form kernel (xattn_resident_d64_kernel) on operands the second form would take."""
    from viewcrafter_amd import ops
    assert ops.tune_get("XATTN_RESIDENT") == 1
    strided = dual_check("resident", "o8", DUAL_KNOBS["default"], DUAL_KNOBS["resident_first"])
    assert strided.o.data_ptr() % 16 == 8 and strided.ldo % 8 == 4


# ================================================================================================================ temporal
def temporal_launch(qkv, ld, k_off, v_off, o, ldo, geo, relg, relp):
    from viewcrafter_amd import ops
    kw = dict(B=geo["B"], T=geo["T"], P=geo["P"], heads=geo["heads"], ld=ld, k_off=k_off, v_off=v_off, ldo=ldo, scale=geo["scale"], causal=geo["causal"])
    if geo["R"]:
        ops.temporal_attn_rel(qkv, o, relg, relp, R=geo["R"], **kw)
    else:
        ops.temporal_attn(qkv, o, **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("T", [25, 33, 64])
def test_temporal_attention_in_the_wide_layout(T, causal):
    """tattn_d64_kernel (T <= 32) and tattn64_d64_kernel, plain and causal, B 2, P 9, heads 2: qkv at column 16 of pitch 3 C + 40 with v in
    front of k and gaps between q, v and k; o at column 8 of pitch C + 24: a - d."""
    A.run_checks(A.temporal_case(temporal_launch, "temporal_wide", device=DEV, T=T, causal=causal))


@pytest.mark.parametrize("causal", [False, True])
def test_temporal_attention_with_relative_position_in_the_wide_layout(causal):
    """tattn_d64_kernel<.., REL>, T 25, R 3: o AND relp against the fp64 reference (no one-hot construction: relg shifts every logit), both
    bit-identical with the dense call; relg is not written."""
    A.run_checks(A.temporal_case(temporal_launch, "temporal_wide", device=DEV, T=25, causal=causal, R=3))


def test_the_dense_temporal_window_is_temporal_layout():
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn((2, 5, 3, 2, 64), generator=g).half() for _ in range(3))
    assert torch.equal(A.temporal_window(q, k, v, "temporal_dense"), temporal_layout(q, k, v).cpu())


# ================================================================================================================ row softmax
@pytest.mark.parametrize("n", [135, 512])
def test_softmax_rows_in_a_window(n):
    """vcx_softmax_rows_f16 in place, 37 rows at column 8 of pitch n8 + 24, NaN all around: a - d."""
    def launch(x, rows, n_, ld):
        from viewcrafter_amd import ops
        assert x.stride(0) == ld
        ops.softmax_rows_(x, n=n_)
        torch.cuda.synchronize()
    A.run_checks(A.softmax_case(launch, "softmax_rows", device=DEV, rows=37, n=n))


# ================================================================================================================ MXFP8 twins
# Input layouts only: the MX output pitch is fixed by the format.  a: the bytes are MX.quant of the fp16 entry's DENSE output on the one-hot
# problem (include/vcx.h: "byte for byte"), which is itself held to O_i = V[pi(i)]; b: element and scale bytes equal those of the
# dense-input call; c: guard rows around both output buffers; d: the operands are untouched.
def mx_out(rows, heads):
    kp = MX.kp_of(64 * heads)
    q = A.embed(torch.full((rows, kp), POISON, dtype=torch.uint8, device=DEV), pitch=kp, col=0, guard_rows=A.GUARD_ROWS, fill=POISON)
    s = A.embed(torch.full((rows, kp // 32), POISON, dtype=torch.uint8, device=DEV), pitch=kp // 32, col=0, guard_rows=A.GUARD_ROWS, fill=POISON)
    return q, s


def mx_checks(name, hot, o16, want, bound, dense, strided):
    """hot / dense / strided: (Placed operands, (oq buffer, oq window), (os buffer, os window)) of an MX call"""
    X.assert_elementwise(o16, want, bound, f"{name}: the fp16 entry on the one-hot problem")
    wq, ws = MX.quant(o16.cpu())
    assert torch.equal(hot[1][1].cpu(), wq) and torch.equal(hot[2][1].cpu(), ws), f"{name}: not the quantised fp16 result"             # a
    assert torch.equal(strided[1][1], dense[1][1]) and torch.equal(strided[2][1], dense[2][1]), f"{name}: bytes differ from the dense-input call"      # b
    for p, (qb, qw), (sb, sw) in (hot, dense, strided):
        A.assert_only_window_written(torch.full_like(qb, POISON), qb, qw.shape[0], 0, qw.shape[1], f"{name} element bytes")             # c
        A.assert_only_window_written(torch.full_like(sb, POISON), sb, sw.shape[0], 0, sw.shape[1], f"{name} scale bytes")
        A.assert_operands_untouched(p.before, p.buf)                                                                                   # d
    K = o16.shape[1]
    assert bool(torch.isfinite(MX.dequant(strided[1][1], strided[2][1], K)).all()), f"{name}: a value from outside an operand's window was used"


MX_FLASH = [("qb1", 100, 135), ("qb2", 300, 135), ("v2", 256, 192)]


@pytest.mark.parametrize("impl,nq,nk", MX_FLASH, ids=[v[0] for v in MX_FLASH])
def test_flash_mxfp8_reads_its_operands_in_the_wide_layout(impl, nq, nk):
    from viewcrafter_amd import _lib, ops
    heads, Gk, kv_div = 2, 2, 2
    G, C, kv_rows = Gk * kv_div, heads * 64, (nk + 7) // 8 * 8 + 16
    kn = dict(FLASH_IMPLS[impl])

    def run(layout, q, k, v):
        kd, vtd = kv_layout(k, v, kv_rows, A.NAN, A.NAN, X.PAD_FINITE)
        p = A.Placed(layout, dict(q=log2_q(q, 0.125), k=kd, vt=vtd), torch.zeros((1, 8), dtype=torch.float16), DEV)
        oq, os_ = mx_out(G * nq, heads)
        with knobs(**kn):
            ops.check(_lib.lib().vcx_attn_flash_d64_mxfp8(p.view["q"].data_ptr(), p.view["k"].data_ptr(), p.view["vt"].data_ptr(), oq[1].data_ptr(), os_[1].data_ptr(),
                                                          G, heads, nq, nk, kv_rows, kv_div, p.ld["q"], p.ld["k"], p.ld["vt"], 1.0, LOG2,
                                                          torch.cuda.current_stream().cuda_stream), "attn_flash_d64_mxfp8")
            torch.cuda.synchronize()
        return p, oq, os_

    q, k, v, want = A.flash_one_hot(Gk, kv_div, heads, nq, nk)
    hot = run("wide", q, k, v)
    d = A.Placed("dense", dict(hot[0].view), torch.full((G * nq, C), A.GUARD, dtype=torch.float16), DEV)
    with knobs(**kn):
        ops.flash_attn(d.view["q"], d.view["k"], d.view["vt"], d.o, n_groups=G, heads=heads, nq=nq, nk=nk, kv_rows=kv_rows, kv_div=kv_div, ldq=C, ldk=C,
                       ldvt=d.ld["vt"], ldo=C, scale=0.0, log2_logits=True)
        torch.cuda.synchronize()
    g = torch.Generator().manual_seed(nq + nk)
    r = lambda *s: torch.randn(s, generator=g).half()
    rq, rk, rv = r(G * nq, C), r(Gk, nk, C), r(Gk, nk, C)
    mx_checks(f"flash mxfp8 {impl}", hot, d.o, want, want.abs() * 2.0 ** -10, run("dense", rq, rk, rv), run("wide", rq, rk, rv))


MX_DUAL = [("resident", dict(XATTN_RESIDENT=1), 3, 77, 256, 200), ("flash_dual_qb1", dict(XATTN_RESIDENT=0, FLASH_QB=1), 1, 77, 16, 100),
           ("flash_dual_qb2", dict(XATTN_RESIDENT=0, FLASH_QB=2), 1, 77, 16, 300)]


@pytest.mark.parametrize("form,kn,T,nk1,nk2,nq", MX_DUAL, ids=[v[0] for v in MX_DUAL])
def test_flash_dual_mxfp8_reads_its_operands_in_the_wide_layout(form, kn, T, nk1, nk2, nq):
    """xattn_resident2_d64_kernel<MXQ> and the dual MXQ instantiations of the phased kernel (the first-form resident kernel has no MX tail)."""
    from viewcrafter_amd import _lib, ops
    geo, hot_ops, want, bound, rnd = dual_problems(T, nk1, nk2, nq, True)
    rows, heads = geo["n_groups"] * nq, geo["heads"]

    def run(layout, operands):
        p = A.Placed(layout, operands, torch.zeros((1, 8), dtype=torch.float16), DEV)
        oq, os_ = mx_out(rows, heads)
        with knobs(**kn):
            ops.check(_lib.lib().vcx_attn_flash_dual_d64_mxfp8(p.view["q"].data_ptr(), p.view["k1"].data_ptr(), p.view["vt1"].data_ptr(), p.view["k2"].data_ptr(),
                                                               p.view["vt2"].data_ptr(), oq[1].data_ptr(), os_[1].data_ptr(), geo["n_groups"], heads, nq, nk1,
                                                               geo["kv_rows1"], T, p.ld["k1"], p.ld["vt1"], nk2, geo["kv_rows2"], T, p.ld["k2"], p.ld["vt2"], p.ld["q"],
                                                               1.0, LOG2, torch.cuda.current_stream().cuda_stream), "attn_flash_dual_d64_mxfp8")
            torch.cuda.synchronize()
        return p, oq, os_

    hot = run("wide", hot_ops)
    d16 = dual_place("dense", hot_ops, geo, True, kn)
    mx_checks(f"dual mxfp8 {form}", hot, d16.o, want, bound, run("dense", rnd), run("wide", rnd))


@pytest.mark.parametrize("causal", [False, True])
def test_temporal_mxfp8_reads_qkv_in_the_wide_layout(causal):
    """tattn_d64_kernel<.., MXQ>, T 25, B 2, P 9, heads 2: qkv at column 16 of pitch 3 C + 40, v in front of k, gaps between the three."""
    from viewcrafter_amd import _lib, ops
    B, T, P, heads = 2, 25, 9, 2
    C, rows = heads * 64, B * T * P

    def run(layout, q, k, v):
        p = A.Placed(layout, dict(qkv=A.temporal_window(q, k, v, layout)), torch.zeros((1, 8), dtype=torch.float16), DEV)
        oq, os_ = mx_out(rows, heads)
        lay = A.LAYOUTS[layout]
        ops.check(_lib.lib().vcx_attn_temporal_d64_mxfp8(p.view["qkv"].data_ptr(), oq[1].data_ptr(), os_[1].data_ptr(), B, T, P, heads, p.ld["qkv"], lay["k_off"](C),
                                                         lay["v_off"](C), 0.125, CAUSAL if causal else 0, torch.cuda.current_stream().cuda_stream), "attn_temporal_d64_mxfp8")
        torch.cuda.synchronize()
        return p, oq, os_

    g = torch.Generator().manual_seed(25 + causal)
    q, k, codes, want = A.temporal_one_hot(B, T, P, heads, causal, g)
    hot = run("temporal_wide", q, k, codes)
    o16 = torch.full((rows, C), A.GUARD, dtype=torch.float16, device=DEV)
    ops.temporal_attn(temporal_layout(q, k, codes), o16, B=B, T=T, P=P, heads=heads, ld=3 * C, k_off=C, v_off=2 * C, ldo=C, scale=0.125, causal=causal)
    torch.cuda.synchronize()
    rq, rk, rv = (torch.randn((B, T, P, heads, 64), generator=g).half() for _ in range(3))
    mx_checks(f"temporal mxfp8 causal {causal}", hot, o16, want, want.abs() * 2.0 ** -10, run("temporal_dense", rq, rk, rv), run("temporal_wide", rq, rk, rv))
