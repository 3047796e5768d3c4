"""The MXFP8 temporal convolutions on the GPU (VCX_TCONV_MXFP8; include/vcx.h vcx_groupnorm_apply_mxfp8_f16 / vcx_conv_t3_mxfp8): the
quantising GroupNorm apply against quant(group_norm) byte for byte, the gathered convolution on operands with exactly known products
(every tap, frame edge, video boundary, padding block and ragged tile an exact mismatch when wrong), its rounding quality, its column
moments, row invariance, TemporalConvBlock against the chain of its ops, and the tiny UNet with the switch on and off."""
import pytest
import torch

from tests import mx_emulation as MX
from tests import rounding_quality as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xAB


def _first_diff(got, want):
    bad = torch.nonzero(got != want)
    return f"{bad.shape[0]} of {got.numel()} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}"


def _bytes_equal(got, want, name):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert torch.equal(got, want), f"{name}: {_first_diff(got, want)}"


def _pair(q, s):
    return q.to(DEV), s.to(DEV)


# ------------------------------------------------------------------------------------------------------------------ 1. apply + quantise
@pytest.mark.parametrize("stats_given", [False, True])
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("n_outer,pixels,C", [(2, 120, 64), (1, 130, 320), (2, 64, 1280), (3, 1, 128)])
def test_groupnorm_quantiser_is_the_quantised_groupnorm(n_outer, pixels, C, silu, stats_given):
    from viewcrafter_amd import _lib, ops
    x = (R.randn((n_outer, pixels, C), 10 + C) * 1.7 + 0.3).half()
    x[0, 0, 40:48] *= 60.0                                     # a loud chunk: its block's scale differs from the neighbours'
    gamma, beta = 1.0 + 0.3 * R.randn((C,), 11), 0.2 * R.randn((C,), 12)
    if not silu:
        gamma[32:64], beta[32:64] = 0.0, 0.0                   # a block of exact zeros: scale byte 0
    if stats_given:                                            # statistics that are not the tensor's own, and one non-finite input
        stats = torch.stack([0.3 + 0.1 * R.randn((n_outer, 32), 13), 2.0 + R.randn((n_outer, 32), 14).abs()], dim=-1).contiguous().to(DEV)
        x[n_outer - 1, pixels - 1, 5] = float("inf")
    x, gamma, beta = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    if not stats_given:
        stats = ops.group_norm_stats(x)
    rows, kp = n_outer * pixels, MX.kp_of(C)
    # one guard row in front and behind, everything poisoned: the kernel writes every byte of its rows (padding included) and no other
    q = torch.full((rows + 2, kp), POISON, dtype=torch.uint8, device=DEV)
    s = torch.full((rows + 2, kp // 32), POISON, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().vcx_groupnorm_apply_mxfp8_f16(x.data_ptr(), q[1].data_ptr(), s[1].data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                        n_outer, pixels, C, 32, 1e-5, 1 if silu else 0, torch.cuda.current_stream().cuda_stream))
    y = ops.group_norm(x, gamma, beta, 1e-5, silu, stats=stats)
    qr, sr = ops.quant_mxfp8(y.view(rows, C))
    q2, s2 = ops.group_norm_mxfp8(x, gamma, beta, 1e-5, silu, stats=stats if stats_given else None)
    torch.cuda.synchronize()
    _bytes_equal(q[1:-1], qr, "elements")
    _bytes_equal(s[1:-1], sr, "scales")
    for g in (q[0], q[-1], s[0], s[-1]):
        assert bool((g == POISON).all()), "a guard row was written"
    _bytes_equal(q2, qr, "ops.group_norm_mxfp8 elements")
    _bytes_equal(s2, sr, "ops.group_norm_mxfp8 scales")
    # ... and it is the format's definition applied to the fp16 tensor, padding included
    qe, se = MX.quant(y.view(rows, C).cpu())
    _bytes_equal(qr, qe, "elements against the torch definition")
    _bytes_equal(sr, se, "scales against the torch definition")
    assert not bool(q[1:-1, C:].any()) and bool((s[1:-1, C // 32:] == 127).all())
    if not silu:
        assert bool((s[1:-1, 1] == 0).all()) and not bool(q[1:-1, 32:64].any())
    if stats_given:
        assert int(s[rows, 0]) == 255 and bool((q[rows, :32] == 0x7F).all())


# ------------------------------------------------------------------------------------------------------------------ 2. convolution, exact data
def _shift(a, tau):
    """a [B, T, P, C] -> the frames t + tau - 1, zeros where that frame does not exist"""
    out = torch.zeros_like(a)
    if tau == 0:
        out[:, 1:] = a[:, :-1]
    elif tau == 1:
        out.copy_(a)
    else:
        out[:, :-1] = a[:, 1:]
    return out


def _conv_ref(a, w, bias, B, T, P, res=None):
    """fp64: a [B T P, Cin], w [N, 3, Cin] -> bias + sum over the taps (+ residual)"""
    cin = a.shape[1]
    a4 = a.view(B, T, P, cin)
    ref = bias.double().unsqueeze(0).expand(B * T * P, -1).clone()
    for tau in range(3):
        ref += _shift(a4, tau).view(B * T * P, cin) @ w[:, tau].t()
    return ref if res is None else ref + res.double()


def _exact_problem(B, T, P, cin, N):
    M = B * T * P
    aq, asc, a = MX.exact_operand(M, cin, 1000 + M + cin)
    wq, wsc, w = MX.exact_operand(3 * N, cin, 2000 + N + cin)
    g = torch.Generator().manual_seed(3000 + N)
    bias = torch.randint(-256, 257, (N,), generator=g).float() * MX.GRID
    res = (torch.randint(-256, 257, (M, N), generator=g).float() * MX.GRID).half()
    w = w.view(N, 3, cin)
    a4 = a.view(B, T, P, cin)
    assert all(not torch.equal(w[:, i], w[:, j]) for i, j in ((0, 1), (1, 2), (0, 2))), "the weights differ per tap"
    assert all(not torch.equal(a4[:, i], a4[:, i + 1]) for i in range(T - 1)) and (B == 1 or not torch.equal(a4[0], a4[1])), "the activations differ per frame and per video"
    return (aq, asc, a), (wq.view(N, -1), wsc.view(N, -1), w), bias, res


def _assert_exact_conditions(ref, cin):
    """|ref| < 65504, and every partial sum - in any order, bias and residual included - is a multiple of 2^-2 below 2^24 x 2^-2: exactly
    representable in fp32 (the condition of test_gemm_is_exact_on_the_integer_grid; on the inputs, not a tolerance)."""
    assert float(ref.abs().max()) < 65504
    assert 3 * cin * MX.PRODUCT_MAX + 2 * 64 < (1 << 24) * MX.GRID
    assert float(ref.abs().max()) < (1 << 24) * MX.GRID and torch.equal(ref / MX.GRID, (ref / MX.GRID).round())


def _assert_fp16_bits(out, ref64, name):
    got, want = out.cpu(), ref64.half()
    assert got.dtype == torch.float16 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{name}: {_first_diff(got, want)}"


EXACT_CASES = [(2, 3, 40, 320, 64), (1, 1, 70, 128, 320), (2, 2, 128, 64, 128), (1, 4, 33, 640, 72)]


@pytest.mark.parametrize("B,T,P,cin,N", EXACT_CASES)
def test_convolution_is_exact_on_the_integer_grid(B, T, P, cin, N):
    """out == fp16(bias + the three taps' sums) bit for bit: a swapped tap order, a row taken from the neighbouring video, a wrapped
    negative offset or a dropped padding block is an exact mismatch."""
    from viewcrafter_amd import ops
    (aq, asc, a), (wq, wsc, w), bias, _ = _exact_problem(B, T, P, cin, N)
    ref = _conv_ref(a, w, bias, B, T, P)
    _assert_exact_conditions(ref, cin)
    assert ops.temporal_conv3_mxfp8_ok(B, T, P, cin, N)
    out = ops.temporal_conv3_mxfp8(_pair(aq, asc), _pair(wq, wsc), bias.to(DEV), B=B, T=T, P=P, cin=cin)
    torch.cuda.synchronize()
    assert out.shape == (B, T, P, N)
    _assert_fp16_bits(out.view(B * T * P, N), ref, f"conv_t3_mxfp8 {B}x{T}x{P}x{cin}->{N}")


def test_convolution_with_a_residual_is_exact():
    from viewcrafter_amd import ops
    B, T, P, cin, N = EXACT_CASES[0]
    (aq, asc, a), (wq, wsc, w), bias, res = _exact_problem(B, T, P, cin, N)
    ref = _conv_ref(a, w, bias, B, T, P, res)
    _assert_exact_conditions(ref, cin)
    assert ops.temporal_conv3_mxfp8_ok(B, T, P, cin, N, residual=True)
    out = ops.temporal_conv3_mxfp8(_pair(aq, asc), _pair(wq, wsc), bias.to(DEV), B=B, T=T, P=P, cin=cin, residual=res.to(DEV))
    torch.cuda.synchronize()
    _assert_fp16_bits(out.view(B * T * P, N), ref, "conv_t3_mxfp8 + residual")


def test_convolution_into_a_wider_buffer_leaves_the_guard_columns_alone():
    from viewcrafter_amd import ops
    B, T, P, cin, N = EXACT_CASES[1]
    M, ldc = B * T * P, N + 24
    (aq, asc, a), (wq, wsc, w), bias, _ = _exact_problem(B, T, P, cin, N)
    ref = _conv_ref(a, w, bias, B, T, P)
    _assert_exact_conditions(ref, cin)
    buf = torch.full((M + 2, ldc), 777.0, dtype=torch.float16, device=DEV)          # + a guard row in front and behind
    assert ops.temporal_conv3_mxfp8_ok(B, T, P, cin, N, ldc=ldc)
    ops.temporal_conv3_mxfp8(_pair(aq, asc), _pair(wq, wsc), bias.to(DEV), B=B, T=T, P=P, cin=cin, out=buf[1:M + 1], ldc=ldc)
    torch.cuda.synchronize()
    _assert_fp16_bits(buf[1:M + 1, :N].contiguous(), ref, "conv_t3_mxfp8, ldc = N + 24")
    assert bool((buf[:, N:] == 777.0).all()), "a guard column was written"
    assert bool((buf[0] == 777.0).all()) and bool((buf[-1] == 777.0).all()), "a guard row was written"


# ------------------------------------------------------------------------------------------------------------------ 3. rounding quality
def _random_problem(B, T, P, cin, N, seed):
    """MXFP8 operands of N(0, 1) activations and N(0, 1) weights scaled to outputs of order one, bias N(0, 1)"""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv_t3_mxfp8
    a = ops.quant_mxfp8(R.randn((B * T * P, cin), seed + 1).half().to(DEV))
    w = pack_conv_t3_mxfp8(R.randn((N, cin, 3, 1, 1), seed + 2, (3 * cin) ** -0.5).to(DEV))
    return a, w, R.randn((N,), seed + 3).to(DEV)


def _dequant_w(w, N, cin):
    kp = MX.kp_of(cin)
    return torch.stack([MX.dequant(w[0][:, t * kp:(t + 1) * kp], w[1][:, t * kp // 32:(t + 1) * kp // 32], cin) for t in range(3)], dim=1)


@pytest.mark.parametrize("B,T,P,cin,N", [EXACT_CASES[0], EXACT_CASES[3]])
def test_convolution_rounds_once(B, T, P, cin, N):
    """Random N(0, 1) operands against the fp64 value of the dequantised operands: fp32 accumulation rounded once, E <= 1.05
    (tests/rounding_quality.py).  These shapes have 15360 / 9504 outputs - below the 32768 check_rounding asks for its 0.25 % noise
    figure; at 0.45 / sqrt(n) the noise of E is 0.36 % / 0.46 % here, a tenth of the bound's margin - so the bound and the mismatch
    cap are asserted on rounding_stats directly."""
    from viewcrafter_amd import ops
    a, w, bias = _random_problem(B, T, P, cin, N, 4000 + cin)
    res = R.randn((B * T * P, N), 4004).half().to(DEV)
    out = ops.temporal_conv3_mxfp8(a, w, bias, B=B, T=T, P=P, cin=cin, residual=res)
    torch.cuda.synchronize()
    ref = _conv_ref(MX.dequant(a[0], a[1], cin), _dequant_w(w, N, cin), bias.cpu(), B, T, P, res.cpu())
    st = R.rounding_stats(out.view(B * T * P, N).cpu(), ref)
    print(f"\n[rounding] conv_t3_mxfp8 {B}x{T}x{P}x{cin}->{N} E {st['E']:.4f} mismatch {100 * st['mismatch']:.2f} % worst {st['worst']:.2f} ulp n {st['n']}")
    assert st["E"] <= R.E_BOUND, f"E = {st['E']:.4f} > {R.E_BOUND}; mismatch {100 * st['mismatch']:.2f} %, worst {st['worst']:.2f} ulp"
    assert st["mismatch"] <= R.MISMATCH_CAP


# ------------------------------------------------------------------------------------------------------------------ 4. column moments
def _strip_moments_ok(cs, y):
    """(mean, M2) per 64-row strip and column against fp64 moments of the stored fp16 output: the function and the bounds the fp16 engine's
    VCX_GEMM_COLSTATS tests use (tests/test_batch_invariance_gpu.py)."""
    M, N = y.shape
    yd = y.double().view(M // 64, 64, N)
    mean = yd.mean(1)
    m2 = ((yd - mean.unsqueeze(1)) ** 2).sum(1)
    assert float((cs[..., 0].double() - mean).abs().max()) <= 2e-6 * (float(yd.abs().max()) + 1.0)
    assert rel_l2(cs[..., 1], m2) <= 2e-5


@pytest.mark.parametrize("N", [128, 320])
def test_column_moments_feed_the_groupnorm_behind_the_convolution(N):
    from viewcrafter_amd import ops
    B, T, P, cin = 2, 3, 64, 128
    M = B * T * P
    a, w, bias = _random_problem(B, T, P, cin, N, 5000 + N)
    res = R.randn((M, N), 5004, 0.5).half().to(DEV)
    assert ops.temporal_conv3_mxfp8_ok(B, T, P, cin, N, residual=True, colstats=True)
    guard = torch.full((M // 64 + 2, N, 2), 7.0, device=DEV)      # the moments buffer with two sentinel strips behind it
    cs = guard[:M // 64]
    y = ops.temporal_conv3_mxfp8(a, w, bias, B=B, T=T, P=P, cin=cin, residual=res, colstats=cs).view(M, N)
    plain = ops.temporal_conv3_mxfp8(a, w, bias, B=B, T=T, P=P, cin=cin, residual=res).view(M, N)
    torch.cuda.synchronize()
    assert torch.equal(y, plain), "the moments are a by-product: the output does not change"
    assert bool((guard[M // 64:] == 7.0).all()), "column moments written beyond the last strip"
    _strip_moments_ok(cs.cpu(), y.cpu())
    # per video (the inner norms of the block) and per frame (the norm behind it): group_norm_stats of the output, to the tolerance
    # tests/test_kernels_gpu.py holds statistics from moments to
    for n_outer, pixels in ((B, T * P), (B * T, P)):
        st = ops.group_norm_stats_from_colstats(cs, n_outer, pixels, N)
        direct = ops.group_norm_stats(y.view(n_outer, pixels, N))
        yd = y.double().view(n_outer, pixels, 32, N // 32)
        mean, var = yd.mean(dim=(1, 3)), yd.var(dim=(1, 3), unbiased=False)
        for other in (direct.double(), torch.stack([mean, var], dim=-1)):
            assert float((st[..., 0].double() - other[..., 0]).abs().max()) <= 2e-6 * float(mean.abs().max() + 1)
            assert rel_l2(st[..., 1], other[..., 1]) <= 2e-5
    if N == 128:
        # ... and once as the left part of a concat: data at ldc, moments at colstats_ld > N behind a column offset, partners untouched
        ld, col = N + 64, 32
        cat = torch.full((M, ld), 3.0, dtype=torch.float16, device=DEV)
        cat_cs = torch.full((M // 64, ld, 2), 5.0, device=DEV)
        assert ops.temporal_conv3_mxfp8_ok(B, T, P, cin, N, residual=True, ldc=ld, colstats=True, colstats_ld=ld, colstats_col=col)
        ops.temporal_conv3_mxfp8(a, w, bias, B=B, T=T, P=P, cin=cin, residual=res, out=cat, ldc=ld, colstats=cat_cs, colstats_ld=ld, colstats_col=col)
        torch.cuda.synchronize()
        assert torch.equal(cat[:, :N], y) and bool((cat[:, N:] == 3.0).all())
        assert torch.equal(cat_cs[:, col:col + N], cs), "the same moments, bit for bit, wherever they are written"
        assert bool((cat_cs[:, :col] == 5.0).all()) and bool((cat_cs[:, col + N:] == 5.0).all())


# ------------------------------------------------------------------------------------------------------------------ 5. row invariance
@pytest.mark.parametrize("residual", [False, True])
def test_a_row_does_not_depend_on_the_call(residual):
    from viewcrafter_amd import ops
    B, T, P, cin, N = 2, 3, 40, 320, 136
    a, w, bias = _random_problem(B, T, P, cin, N, 6000)
    res = R.randn((B * T * P, N), 6004).half().to(DEV)
    V = T * P
    run = lambda aa, rr, b: ops.temporal_conv3_mxfp8(aa, w, bias, B=b, T=T, P=P, cin=cin, residual=rr if residual else None).view(b * V, N)
    both = run(a, res, 2)
    again = run(a, res, 2)
    ones = [run((a[0][i * V:(i + 1) * V].contiguous(), a[1][i * V:(i + 1) * V].contiguous()), res[i * V:(i + 1) * V].contiguous(), 1) for i in range(2)]
    torch.cuda.synchronize()
    assert torch.isfinite(both).all() and float(both.float().abs().max()) > 0.5
    assert torch.equal(again, both), "the same call twice"
    assert torch.equal(ones[0], both[:V]), f"M = 240: {int((ones[0] != both[:V]).sum())} elements of the first 120 rows differ from video 0 run alone"
    assert torch.equal(torch.cat(ones), both), f"B = 2 differs from two B = 1 calls in {int((torch.cat(ones) != both).sum())} elements"


# ------------------------------------------------------------------------------------------------------------------ 6. TemporalConvBlock
def _block(C):
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    torch.manual_seed(C)
    blk = U.TemporalConvBlock(C).eval()
    with torch.no_grad():
        for seq in (blk.conv1, blk.conv2, blk.conv3, blk.conv4):
            seq[0].weight.copy_(1.0 + 0.2 * torch.randn(C))
            seq[0].bias.copy_(0.1 * torch.randn(C))
            seq[-1].weight.copy_(torch.randn(C, C, 3, 1, 1) * (3 * C) ** -0.5)
            seq[-1].bias.copy_(0.1 * torch.randn(C))
    return U, blk.to(DEV)


@pytest.mark.parametrize("want", [False, True])
@pytest.mark.parametrize("C", [64, 128, 320])
def test_block_on_the_mx_route_is_the_composition_of_its_ops(C, want, monkeypatch):
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv_t3_mxfp8
    U, blk = _block(C)
    B, T, P = 2, 3, 64
    x = (R.randn((B, T, P, C), 7000 + C) * 1.3).half().to(DEV)
    with torch.no_grad():
        y16, cs16 = blk(x, want_colstats=want)
        monkeypatch.setattr(U, "TCONV_MXFP8", True)
        monkeypatch.setattr(U, "TCONV_MXFP8_SKIP_DIMS", frozenset())
        ymx, csmx = blk(x, want_colstats=want)
        # the chain, written out: statistics of the first norm computed, of the other three from the previous convolution's moments
        y, cs = x, None
        for i, seq in enumerate((blk.conv1, blk.conv2, blk.conv3, blk.conv4)):
            gn, conv = seq[0], seq[-1]
            stats = None if cs is None else ops.group_norm_stats_from_colstats(cs, B, T * P, C)
            a = ops.group_norm_mxfp8(y.reshape(B, T * P, C), gn.weight.detach().float(), gn.bias.detach().float(), gn.eps, True, stats=stats)
            last = i == 3
            cs = ops.colstats_buffer(B * T * P, C, DEV) if (not last or want) else None
            y = ops.temporal_conv3_mxfp8(a, pack_conv_t3_mxfp8(conv.weight.detach()), conv.bias.detach().float(), B=B, T=T, P=P, cin=C,
                                         residual=x.view(B * T * P, C) if last else None, colstats=cs)
    torch.cuda.synchronize()
    assert torch.equal(ymx, y), f"the block differs from the chain of its ops in {int((ymx != y).sum())} elements"
    assert (csmx is None) == (not want) and (cs16 is None) == (not want)
    if want:
        assert torch.equal(csmx, cs)
    assert torch.isfinite(ymx).all() and not torch.equal(ymx, y16), "the MX route did not run"
    print(f"\n[mxfp8] TemporalConvBlock({C}): rel-L2(MX - fp16) of the branch = {rel_l2(ymx.float() - x.float(), y16.float() - x.float()):.3e}")


def test_block_keeps_fp16_at_a_skipped_width(monkeypatch):
    U, blk = _block(128)
    x = (R.randn((2, 3, 64, 128), 7500) * 1.3).half().to(DEV)
    with torch.no_grad():
        y16, _ = blk(x)
        monkeypatch.setattr(U, "TCONV_MXFP8", True)
        monkeypatch.setattr(U, "TCONV_MXFP8_SKIP_DIMS", frozenset([128]))
        kept, _ = blk(x)
        assert blk._mx is None, "an MX pack was built at a skipped width"
        monkeypatch.setattr(U, "TCONV_MXFP8_SKIP_DIMS", frozenset())
        ymx, _ = blk(x)
    torch.cuda.synchronize()
    assert torch.equal(kept, y16) and blk._mx is not None
    assert torch.isfinite(ymx).all() and not torch.equal(ymx, y16)


# ------------------------------------------------------------------------------------------------------------------ 7. tiny UNet
def _tiny_unet():
    from tests.tiny_config import TINY_UNET
    from tests.util import load_synth
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    return m.to(DEV), TINY_UNET


def test_tiny_unet_with_the_switch_on_and_off(monkeypatch):
    from oracle.weights import synth_input
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    m, cfg = _tiny_unet()
    t, h, w, L = 4, 16, 32, 77 + 64
    x = synth_input("mx_x", (2, 8, t, h, w)).to(DEV)
    x[1] = x[0]
    ctx = synth_input("mx_ctx", (2, L, cfg["context_dim"])).to(DEV)
    ts, fs = torch.tensor([799, 799], device=DEV), torch.tensor([10, 10], device=DEV)
    with torch.no_grad():
        before = m._forward(x, ts, context=ctx, fs=fs)             # the module flag has never been touched
        monkeypatch.setattr(U, "TCONV_MXFP8", True)
        monkeypatch.setattr(U, "TCONV_MXFP8_SKIP_DIMS", frozenset())
        on = m._forward(x, ts, context=ctx, fs=fs)
        ones = torch.cat([m._forward(x[i:i + 1].contiguous(), ts[:1], context=ctx[i:i + 1].contiguous(), fs=fs[:1]) for i in range(2)])
        shared = m._forward(x[:1].contiguous(), ts[:1], context=ctx, fs=fs[:1], cfg_repeat=2)
        monkeypatch.setattr(U, "TCONV_MXFP8", False)
        off = m._forward(x, ts, context=ctx, fs=fs)
    torch.cuda.synchronize()
    assert sum(b._mx is not None for b in m.modules() if isinstance(b, U.TemporalConvBlock)) > 0
    assert torch.isfinite(on).all()
    assert not torch.equal(on, before), "the switch changed nothing: the MX route did not run"
    assert torch.equal(ones, on), f"B = 2 differs from two B = 1 forwards in {int((ones != on).sum())} elements"
    assert torch.equal(shared, on), f"the shared CFG prefix differs from the replicated batch in {int((shared != on).sum())} elements"
    assert torch.equal(off, before), f"switch off: {int((off != before).sum())} elements differ from the run before it was ever on"
    print(f"\n[mxfp8] tiny UNet, temporal convolutions: rel-L2(on - off) = {rel_l2(on, off):.3e}")


def test_tiny_unet_with_the_switch_on_replays_from_a_captured_graph(monkeypatch):
    """The MX route is capturable: the packs (host code) are built by the warm-up forward ahead of the capture, the predicate touches no
    device, nothing on the path synchronises.  The replay is bit-equal to the eager forward, also with new inputs."""
    from oracle.weights import synth_input
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    m, cfg = _tiny_unet()
    monkeypatch.setattr(U, "TCONV_MXFP8", True)
    monkeypatch.setattr(U, "TCONV_MXFP8_SKIP_DIMS", frozenset())
    T, h, w = 4, 16, 32
    ctx = synth_input("mxg_ctx", (2, 77 + 16 * T, cfg["context_dim"])).to(DEV)
    fs = torch.tensor([10, 10], device=DEV)
    try:
        for k, tval in enumerate((999, 479)):
            x = synth_input(f"mxg_x{k}", (2, cfg["in_channels"], T, h, w)).to(DEV)
            t = torch.full((2,), tval, device=DEV, dtype=torch.long)
            m.use_hip_graph = False
            with torch.no_grad():
                eager = m(x, t, context=ctx, fs=fs).clone()
            m.use_hip_graph = True
            with torch.no_grad():
                graphed = m(x, t, context=ctx, fs=fs).clone()
            assert torch.isfinite(eager).all() and torch.equal(eager, graphed), f"replay {k} differs from eager"
        assert len(m._graphs) == 1
    finally:
        m.use_hip_graph = False
        m._graphs.clear()
