"""The MXFP8 ResBlock convolutions on the GPU (VCX_RESCONV_MXFP8; include/vcx.h vcx_groupnorm_apply2_mxfp8_f16 / vcx_conv3x3_mxfp8): the
quantising GroupNorm apply over a split concat against quant(group_norm(x, x2=...)) byte for byte, the gathered 3x3 convolution on
operands with exactly known products (every tap, image edge, frame boundary, padding block and ragged tile an exact mismatch when wrong),
its epilogues, its rounding quality, its column moments, row invariance, ResBlock against the chain of its ops, and the tiny UNet with the
switch on and off."""
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


# ------------------------------------------------------------------------------------------------------------------ 1. apply2 + quantise
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("n_outer,pixels,c1,c2", [(2, 120, 64, 64), (1, 130, 320, 640), (3, 1, 40, 88)])
def test_split_concat_quantiser_is_the_quantised_split_concat_groupnorm(n_outer, pixels, c1, c2, silu):
    """(3, 1, 40, 88): channels 32 .. 63 are one MX block with 8 channels from x1 and 24 from x2."""
    from viewcrafter_amd import _lib, ops
    C = c1 + c2
    x1 = (R.randn((n_outer, pixels, c1), 10 + C) * 1.7 + 0.3).half()
    x2 = (R.randn((n_outer, pixels, c2), 20 + C) * 0.6 - 0.2).half()
    x1[0, 0, 32:40] *= 60.0                                    # a loud chunk: its block's scale differs from the neighbours'
    x2[0, 0, 8:16] *= 40.0
    gamma, beta = 1.0 + 0.3 * R.randn((C,), 11), 0.2 * R.randn((C,), 12)
    if not silu:
        gamma[C - 32:], beta[C - 32:] = 0.0, 0.0               # a block of exact zeros in the right half: scale byte 0
    x1, x2, gamma, beta = x1.to(DEV), x2.to(DEV), gamma.to(DEV), beta.to(DEV)
    stats = ops.group_norm_stats(torch.cat([x1, x2], dim=2).contiguous())
    rows, kp = n_outer * pixels, MX.kp_of(C)
    # one guard row in front and behind, everything poisoned: the kernel writes every byte of its rows (padding included) and no other
    q = torch.full((rows + 2, kp), POISON, dtype=torch.uint8, device=DEV)
    s = torch.full((rows + 2, kp // 32), POISON, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().vcx_groupnorm_apply2_mxfp8_f16(x1.data_ptr(), c1, x2.data_ptr(), q[1].data_ptr(), s[1].data_ptr(), stats.data_ptr(), gamma.data_ptr(),
                                                         beta.data_ptr(), n_outer, pixels, C, 32, 1e-5, 1 if silu else 0, torch.cuda.current_stream().cuda_stream))
    y = ops.group_norm(x1, gamma, beta, 1e-5, silu, stats=stats, x2=x2)
    qr, sr = ops.quant_mxfp8(y.view(rows, C))
    q2, s2 = ops.group_norm_mxfp8(x1, gamma, beta, 1e-5, silu, stats=stats, x2=x2)
    torch.cuda.synchronize()
    _bytes_equal(q[1:-1], qr, "elements")
    _bytes_equal(s[1:-1], sr, "scales")
    for g in (q[0], q[-1], s[0], s[-1]):
        assert bool((g == POISON).all()), "a guard row was written"
    _bytes_equal(q2, qr, "ops.group_norm_mxfp8(x2=) elements")
    _bytes_equal(s2, sr, "ops.group_norm_mxfp8(x2=) scales")
    qe, se = MX.quant(y.view(rows, C).cpu())
    _bytes_equal(qr, qe, "elements against the torch definition")
    _bytes_equal(sr, se, "scales against the torch definition")
    assert not bool(q[1:-1, C:].any()) and bool((s[1:-1, C // 32:] == 127).all()), "padding: element bytes 0x00, scale bytes 127 up to Kp"
    if not silu:
        assert bool((s[1:-1, C // 32 - 1] == 0).all()) and not bool(q[1:-1, C - 32:C].any())


# ------------------------------------------------------------------------------------------------------------------ 2. convolution, exact data
def _shift2(a, ky, kx):
    """a [n, H, W, C] -> the pixels (y + ky - 1, x + kx - 1) of the same frame, zeros where they do not exist"""
    n, H, W, _ = a.shape
    out = torch.zeros_like(a)
    dy, dx = ky - 1, kx - 1
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[:, yd, xd] = a[:, ys, xs]
    return out


def _conv_ref(a, w, bias, n, H, W, rowadd=None, rowadd_div=0, res=None):
    """fp64: a [n H W, Cin], w [N, 9, Cin] -> bias + sum over the nine taps (+ rowadd[m / rowadd_div]) (+ residual)"""
    cin, M = a.shape[1], n * H * W
    a4 = a.view(n, H, W, cin)
    ref = bias.double().unsqueeze(0).expand(M, -1).clone()
    for tap in range(9):
        ref += _shift2(a4, tap // 3, tap % 3).reshape(M, cin) @ w[:, tap].t()
    if rowadd is not None:
        ref += rowadd.double()[torch.arange(M) // rowadd_div]
    return ref if res is None else ref + res.double()


def _slab_major(q, s, N):
    """[N * 9, Kp] / [N * 9, Kp / 32] (one row per (n, tap)) -> the kernel's [N, Kp / 128, 9, 128] / [N, Kp / 128, 9, 4]"""
    slabs = q.shape[1] // 128
    return (q.view(N, 9, slabs, 128).permute(0, 2, 1, 3).reshape(N, -1).contiguous(), s.view(N, 9, slabs, 4).permute(0, 2, 1, 3).reshape(N, -1).contiguous())


def _exact_problem(n, H, W, cin, N, rowadd_div=0):
    M = n * H * W
    aq, asc, a = MX.exact_operand(M, cin, 1000 + M + cin)
    wq, wsc, w = MX.exact_operand(9 * N, cin, 2000 + N + cin)
    g = torch.Generator().manual_seed(3000 + N)
    bias = torch.randint(-256, 257, (N,), generator=g).float() * MX.GRID
    res = (torch.randint(-256, 257, (M, N), generator=g).float() * MX.GRID).half()
    rowadd = torch.randint(-256, 257, ((M + rowadd_div - 1) // rowadd_div, N), generator=g).float() * MX.GRID if rowadd_div else None
    w = w.view(N, 9, cin)
    a4 = a.view(n, H, W, cin)
    assert all(not torch.equal(w[:, i], w[:, j]) for i in range(9) for j in range(i)), "the weights differ per tap"
    assert n == 1 or all(not torch.equal(a4[i], a4[i + 1]) for i in range(n - 1)), "the activations differ per frame"
    assert H == 1 or not torch.equal(a4[:, 0], a4[:, 1]), "... per image row"
    assert W == 1 or not torch.equal(a4[:, :, 0], a4[:, :, 1]), "... and per pixel"
    wq, wsc = _slab_major(wq, wsc, N)
    return (aq, asc, a), (wq, wsc, w), bias, rowadd, res


def _assert_exact_conditions(ref, cin):
    """|ref| < 65504, and every partial sum - in any order, bias, addend and residual included - is a multiple of 2^-2 below 2^24 x 2^-2
    = 2^22: exactly representable in fp32 (on the inputs, not a tolerance)."""
    assert float(ref.abs().max()) < 65504
    assert 9 * cin * MX.PRODUCT_MAX + 3 * 64 < (1 << 24) * MX.GRID
    assert float(ref.abs().max()) < (1 << 24) * MX.GRID and torch.equal(ref / MX.GRID, (ref / MX.GRID).round())


def _assert_fp16_bits(out, ref64, name):
    got, want = out.cpu(), ref64.half()
    assert got.dtype == torch.float16 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{name}: {_first_diff(got, want)}"


# one partial tile, two frames | tile edges mid-image-row, three column tiles | a single pixel | H = 1 | W = 1 | five slabs, ragged N
EXACT_CASES = [(2, 5, 7, 320, 64), (3, 9, 16, 128, 320), (1, 1, 1, 64, 128), (1, 1, 130, 64, 128), (2, 40, 1, 64, 72), (2, 3, 50, 640, 72)]


@pytest.mark.parametrize("n,H,W,cin,N", EXACT_CASES)
def test_convolution_is_exact_on_the_integer_grid(n, H, W, cin, N):
    """out == fp16(bias + the nine taps' sums) bit for bit: a swapped tap, a row from the neighbouring frame or image row, a wrapped
    offset or a dropped padding block is an exact mismatch."""
    from viewcrafter_amd import ops
    (aq, asc, a), (wq, wsc, w), bias, _, _ = _exact_problem(n, H, W, cin, N)
    ref = _conv_ref(a, w, bias, n, H, W)
    _assert_exact_conditions(ref, cin)
    assert ops.conv3x3_mxfp8_ok(n, H, W, cin, N)
    out = ops.conv3x3_mxfp8(_pair(aq, asc), _pair(wq, wsc), bias.to(DEV), n=n, H=H, W=W, cin=cin)
    torch.cuda.synchronize()
    assert out.shape == (n, H, W, N)
    _assert_fp16_bits(out.view(n * H * W, N), ref, f"conv3x3_mxfp8 {n}x{H}x{W}x{cin}->{N}")


def test_pack_feeds_the_kernel_the_order_it_reads():
    """packing.pack_conv3x3_mxfp8 of the exact weights (every value an exact MXFP8 value: the pack is lossless) gives the same output bits."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv3x3_mxfp8
    n, H, W, cin, N = EXACT_CASES[0]
    (aq, asc, a), (_, _, w), bias, _, _ = _exact_problem(n, H, W, cin, N)
    w4 = w.view(N, 3, 3, cin).permute(0, 3, 1, 2).contiguous().float()          # [N, Cin, 3, 3]
    ref = _conv_ref(a, w, bias, n, H, W)
    out = ops.conv3x3_mxfp8(_pair(aq, asc), _pair(*pack_conv3x3_mxfp8(w4)), bias.to(DEV), n=n, H=H, W=W, cin=cin)
    torch.cuda.synchronize()
    _assert_fp16_bits(out.view(n * H * W, N), ref, "conv3x3_mxfp8 on pack_conv3x3_mxfp8's weights")


# ------------------------------------------------------------------------------------------------------------------ 3. epilogues, exact data
# (case, rowadd_div or 0, residual): two videos of two frames with one addend row per video - 288 rows: tiles 0 and 1 lie in one video, tile 2
# straddles both -; one addend row per 35 rows: every tile is split; residual alone; both
EPI_CASES = [((4, 9, 16, 128, 320), 2 * 9 * 16, False), ((2, 5, 7, 320, 64), 35, False), ((2, 5, 7, 320, 64), 0, True), ((4, 9, 16, 128, 320), 2 * 9 * 16, True),
             ((2, 5, 7, 320, 64), 50, True)]


@pytest.mark.parametrize("case,div,residual", EPI_CASES)
def test_convolution_with_rowadd_and_residual_is_exact(case, div, residual):
    from viewcrafter_amd import ops
    n, H, W, cin, N = case
    (aq, asc, a), (wq, wsc, w), bias, rowadd, res = _exact_problem(n, H, W, cin, N, rowadd_div=div)
    ref = _conv_ref(a, w, bias, n, H, W, rowadd, div, res if residual else None)
    _assert_exact_conditions(ref, cin)
    assert ops.conv3x3_mxfp8_ok(n, H, W, cin, N, rowadd=bool(div), rowadd_div=div, residual=residual)
    out = ops.conv3x3_mxfp8(_pair(aq, asc), _pair(wq, wsc), bias.to(DEV), n=n, H=H, W=W, cin=cin, rowadd=rowadd.to(DEV) if div else None, rowadd_div=div,
                            residual=res.to(DEV) if residual else None)
    torch.cuda.synchronize()
    _assert_fp16_bits(out.view(n * H * W, N), ref, f"conv3x3_mxfp8 rowadd_div={div} residual={residual}")


def test_rowadd_as_a_column_slice_of_a_wider_matrix_is_exact():
    """The embedding of all ResBlocks is one projection: a block's addend is a column slice, rowadd_ld > N."""
    from viewcrafter_amd import ops
    n, H, W, cin, N = 4, 9, 16, 128, 320
    div = 2 * H * W
    (aq, asc, a), (wq, wsc, w), bias, rowadd, _ = _exact_problem(n, H, W, cin, N, rowadd_div=div)
    wide = torch.full((rowadd.shape[0], N + 72), 1e4, device=DEV)
    wide[:, 40:40 + N] = rowadd.to(DEV)
    ref = _conv_ref(a, w, bias, n, H, W, rowadd, div)
    out = ops.conv3x3_mxfp8(_pair(aq, asc), _pair(wq, wsc), bias.to(DEV), n=n, H=H, W=W, cin=cin, rowadd=wide[:, 40:40 + N], rowadd_div=div)
    torch.cuda.synchronize()
    _assert_fp16_bits(out.view(n * H * W, N), ref, "conv3x3_mxfp8, rowadd_ld = N + 72")


def test_convolution_into_a_wider_buffer_leaves_the_guard_columns_alone():
    from viewcrafter_amd import ops
    n, H, W, cin, N = 4, 9, 16, 128, 320
    div = 2 * H * W
    M, ldc = n * H * W, N + 24
    (aq, asc, a), (wq, wsc, w), bias, rowadd, res = _exact_problem(n, H, W, cin, N, rowadd_div=div)
    ref = _conv_ref(a, w, bias, n, H, W, rowadd, div, res)
    _assert_exact_conditions(ref, cin)
    buf = torch.full((M + 2, ldc), 777.0, dtype=torch.float16, device=DEV)          # + a guard row in front and behind
    assert ops.conv3x3_mxfp8_ok(n, H, W, cin, N, rowadd=True, rowadd_div=div, residual=True, ldc=ldc)
    ops.conv3x3_mxfp8(_pair(aq, asc), _pair(wq, wsc), bias.to(DEV), n=n, H=H, W=W, cin=cin, rowadd=rowadd.to(DEV), rowadd_div=div, residual=res.to(DEV),
                      out=buf[1:M + 1], ldc=ldc)
    torch.cuda.synchronize()
    _assert_fp16_bits(buf[1:M + 1, :N].contiguous(), ref, "conv3x3_mxfp8, ldc = N + 24")
    assert bool((buf[:, N:] == 777.0).all()), "a guard column was written"
    assert bool((buf[0] == 777.0).all()) and bool((buf[-1] == 777.0).all()), "a guard row was written"


# ------------------------------------------------------------------------------------------------------------------ 4. rounding quality
def _random_problem(n, H, W, cin, N, seed):
    """MXFP8 operands of N(0, 1) activations and N(0, 1) weights scaled to outputs of order one, bias N(0, 1)"""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv3x3_mxfp8
    a = ops.quant_mxfp8(R.randn((n * H * W, cin), seed + 1).half().to(DEV))
    w = pack_conv3x3_mxfp8(R.randn((N, cin, 3, 3), seed + 2, (9 * cin) ** -0.5).to(DEV))
    return a, w, R.randn((N,), seed + 3).to(DEV)


def _dequant_w(w, N, cin):
    """the packed pair -> fp64 [N, 9, cin]"""
    slabs = MX.kp_of(cin) // 128
    q = w[0].cpu().view(N, slabs, 9, 128).permute(0, 2, 1, 3).reshape(N * 9, slabs * 128)
    s = w[1].cpu().view(N, slabs, 9, 4).permute(0, 2, 1, 3).reshape(N * 9, slabs * 4)
    return MX.dequant(q.contiguous(), s.contiguous(), cin).view(N, 9, cin)


@pytest.mark.parametrize("n,H,W,cin,N", [(2, 9, 16, 320, 136), (3, 5, 7, 640, 320)])
def test_convolution_rounds_once(n, H, W, cin, N):
    """Random N(0, 1) operands against the fp64 value of the dequantised operands: fp32 accumulation rounded once - E <= 1.05, mismatch
    <= 10 %, n >= 32768 (tests/rounding_quality.check_rounding; 39168 and 33600 outputs)."""
    from viewcrafter_amd import ops
    a, w, bias = _random_problem(n, H, W, cin, N, 4000 + cin)
    M = n * H * W
    res = R.randn((M, N), 4004).half().to(DEV)
    out = ops.conv3x3_mxfp8(a, w, bias, n=n, H=H, W=W, cin=cin, residual=res)
    torch.cuda.synchronize()
    ref = _conv_ref(MX.dequant(a[0], a[1], cin), _dequant_w(w, N, cin), bias.cpu(), n, H, W, res=res.cpu())
    R.check_rounding("conv3x3_mxfp8", f"{n}x{H}x{W}x{cin}->{N}", out.view(M, N).cpu(), ref)


# ------------------------------------------------------------------------------------------------------------------ 5. column moments
@pytest.mark.parametrize("N", [128, 320])
def test_column_moments_feed_the_groupnorm_behind_the_convolution(N):
    from tests.test_mxfp8_tconv_gpu import _strip_moments_ok
    from viewcrafter_amd import ops
    n, H, W, cin = 2, 8, 16, 128
    M = n * H * W
    a, w, bias = _random_problem(n, H, W, cin, N, 5000 + N)
    rowadd = R.randn((n, N), 5005).to(DEV)
    res = R.randn((M, N), 5004, 0.5).half().to(DEV)
    kw = dict(n=n, H=H, W=W, cin=cin, rowadd=rowadd, rowadd_div=H * W, residual=res)
    assert ops.conv3x3_mxfp8_ok(n, H, W, cin, N, rowadd=True, rowadd_div=H * W, residual=True, colstats=True)
    guard = torch.full((M // 64 + 2, N, 2), 7.0, device=DEV)      # the moments buffer with two sentinel strips behind it
    cs = guard[:M // 64]
    y = ops.conv3x3_mxfp8(a, w, bias, colstats=cs, **kw).view(M, N)
    plain = ops.conv3x3_mxfp8(a, w, bias, **kw).view(M, N)
    torch.cuda.synchronize()
    assert torch.equal(y, plain), "the moments are a by-product: the output does not change"
    assert bool((guard[M // 64:] == 7.0).all()), "column moments written beyond the last strip"
    _strip_moments_ok(cs.cpu(), y.cpu())
    # per frame (the norm behind the convolution) and per video: group_norm_stats of the output, to the tolerance the temporal
    # convolution's test holds statistics from moments to
    for n_outer, pixels in ((n, H * W), (1, n * H * W)):
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
        assert ops.conv3x3_mxfp8_ok(n, H, W, cin, N, rowadd=True, rowadd_div=H * W, residual=True, ldc=ld, colstats=True, colstats_ld=ld, colstats_col=col)
        ops.conv3x3_mxfp8(a, w, bias, out=cat, ldc=ld, colstats=cat_cs, colstats_ld=ld, colstats_col=col, **kw)
        torch.cuda.synchronize()
        assert torch.equal(cat[:, :N], y) and bool((cat[:, N:] == 3.0).all())
        assert torch.equal(cat_cs[:, col:col + N], cs), "the same moments, bit for bit, wherever they are written"
        assert bool((cat_cs[:, :col] == 5.0).all()) and bool((cat_cs[:, col + N:] == 5.0).all())


# ------------------------------------------------------------------------------------------------------------------ 6. row invariance
@pytest.mark.parametrize("residual", [False, True])
def test_a_row_does_not_depend_on_the_call(residual):
    from viewcrafter_amd import ops
    n, H, W, cin, N = 2, 5, 8, 320, 136
    F = H * W
    a, w, bias = _random_problem(5, H, W, cin, N, 6000)          # five frames: the two under test are frames 1 and 2 of them
    res = R.randn((5 * F, N), 6004).half().to(DEV)
    rows = lambda t, f0, f1: t[f0 * F:f1 * F].contiguous()
    run = lambda f0, f1, ww=w, bb=bias, cols=N: ops.conv3x3_mxfp8((rows(a[0], f0, f1), rows(a[1], f0, f1)), ww, bb, n=f1 - f0, H=H, W=W, cin=cin,
                                                                  residual=rows(res, f0, f1)[:, :cols].contiguous() if residual else None).view((f1 - f0) * F, cols)
    both = run(1, 3)
    again = run(1, 3)
    ones = [run(1, 2), run(2, 3)]
    five = run(0, 5)                                            # 200 rows: another tile holds them
    narrow = run(1, 3, (w[0][:72].contiguous(), w[1][:72].contiguous()), bias[:72].contiguous(), 72)      # one column tile instead of two
    torch.cuda.synchronize()
    assert torch.isfinite(both).all() and float(both.float().abs().max()) > 0.5
    assert torch.equal(again, both), "the same call twice"
    assert torch.equal(torch.cat(ones), both), f"n = 2 differs from the two n = 1 calls in {int((torch.cat(ones) != both).sum())} elements"
    assert torch.equal(five[F:3 * F], both), f"inside n = 5: {int((five[F:3 * F] != both).sum())} elements differ"
    assert torch.equal(narrow, both[:, :72]), f"with one column tile: {int((narrow != both[:, :72]).sum())} elements differ"


# ------------------------------------------------------------------------------------------------------------------ 7. ResBlock
EMB = 64


def _block(cin, cout, temporal=False):
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    torch.manual_seed(cin + cout)
    blk = U.ResBlock(cin, EMB, 0.0, out_channels=cout, use_temporal_conv=temporal).eval()
    with torch.no_grad():
        for gn in (blk.in_layers[0], blk.out_layers[0]):
            gn.weight.copy_(1.0 + 0.2 * torch.randn(gn.weight.shape))
            gn.bias.copy_(0.1 * torch.randn(gn.bias.shape))
        for conv in (blk.in_layers[2], blk.out_layers[3]):
            conv.weight.copy_(torch.randn(conv.weight.shape) * (9 * conv.in_channels) ** -0.5)
            conv.bias.copy_(0.1 * torch.randn(conv.bias.shape))
        if temporal:
            for seq in (blk.temopral_conv.conv1, blk.temopral_conv.conv2, blk.temopral_conv.conv3, blk.temopral_conv.conv4):
                seq[-1].weight.copy_(torch.randn(seq[-1].weight.shape) * (3 * cout) ** -0.5)
                seq[-1].bias.copy_(0.1 * torch.randn(cout))
    return U, blk.to(DEV)


def _host_colstats(x):
    """(mean, M2) per 64-row strip and column of x [M, C] - the moments a producing layer's epilogue would have written"""
    M, C = x.shape
    xd = x.double().view(M // 64, 64, C)
    mean = xd.mean(1)
    return torch.stack([mean, ((xd - mean.unsqueeze(1)) ** 2).sum(1)], dim=-1).float().contiguous()


BLOCKS = {"identity": (64, 0, 64, False), "skip_conv": (64, 0, 128, False), "split_concat": (64, 64, 64, False), "temporal": (64, 0, 64, True)}
# (block, RESCONV_MXFP8_KEEP_FOLD): the policy only enters where there is a skip convolution
BLOCK_POLICIES = [("identity", True), ("skip_conv", True), ("skip_conv", False), ("split_concat", True), ("split_concat", False), ("temporal", True)]


@pytest.mark.parametrize("call", ["plain", "target", "want_colstats"])
@pytest.mark.parametrize("kind,keep_fold", BLOCK_POLICIES)
def test_block_on_the_mx_route_is_the_composition_of_its_ops(kind, keep_fold, call, monkeypatch):
    from viewcrafter_amd import ops
    from viewcrafter_amd.lvdm.modules.flow import CatTarget
    from viewcrafter_amd.packing import pack_conv3x3_mxfp8
    c1, c2, cout, temporal = BLOCKS[kind]
    cin = c1 + c2
    U, blk = _block(cin, cout, temporal)
    B, fpv, H, W = 2, 2, 8, 8
    n, M = B * fpv, B * fpv * H * W
    x = (R.randn((n, H, W, c1), 7000 + cin) * 1.3).half().to(DEV)
    x2 = (R.randn((n, H, W, c2), 7001 + cin) * 0.8 + 0.2).half().to(DEV) if c2 else None
    emb = R.randn((B, EMB), 7002).half().to(DEV)
    cs_in = _host_colstats(torch.cat([x, x2], dim=-1).view(M, cin).cpu()).to(DEV) if c2 else None
    want = call == "want_colstats"
    mk_target = lambda: CatTarget(M, cout, 32, DEV, with_moments=True) if call == "target" else None
    kwargs = lambda t: dict(batch_size=B, want_colstats=want, colstats=cs_in, target=t, x2=x2)
    with torch.no_grad():
        t16 = mk_target()
        y16, cs16 = blk(x, emb, **kwargs(t16))
        y16 = y16.clone()
        monkeypatch.setattr(U, "RESCONV_MXFP8", True)
        monkeypatch.setattr(U, "RESCONV_MXFP8_SKIP_DIMS", frozenset())
        monkeypatch.setattr(U, "RESCONV_MXFP8_KEEP_FOLD", keep_fold)
        tmx = mk_target()
        ymx, csmx = blk(x, emb, **kwargs(tmx))
        # the chain, written out
        pk = blk.packed()
        tch = mk_target()
        stats_in = None if cs_in is None else ops.group_norm_stats_from_colstats(cs_in, n, H * W, cin)
        a = ops.group_norm_mxfp8(x.view(n, H * W, c1), *pk["g1"], True, stats=stats_in, x2=None if x2 is None else x2.view(n, H * W, c2))
        emb_out = ops.linear(emb, pk["we"], pk["be"], out_f32=True)
        cs1 = ops.colstats_buffer(M, cout, DEV)
        h = ops.conv3x3_mxfp8(a, pack_conv3x3_mxfp8(blk.in_layers[2].weight.detach()), pk["b1"], n=n, H=H, W=W, cin=cin, rowadd=emb_out, rowadd_div=fpv * H * W,
                              colstats=cs1)
        stats = ops.group_norm_stats_from_colstats(cs1, n, H * W, cout)
        if temporal:
            kw2 = dict(colstats=ops.colstats_buffer(M, cout, DEV))
        elif tch is not None:
            kw2 = tch.kwargs(cout, M)
        else:
            kw2 = dict(colstats=ops.colstats_buffer(M, cout, DEV)) if want else {}
        conv2_mx = kind in ("identity", "temporal") or (kind == "skip_conv" and not keep_fold)
        if conv2_mx:
            a = ops.group_norm_mxfp8(h.view(n, H * W, cout), *pk["g2"], True, stats=stats)
            res = x.reshape(M, cout) if "ws" not in pk else ops.conv2d(x, pk["ws"], pk["bs"], kh=1, kw=1).view(M, cout)
            y = ops.conv3x3_mxfp8(a, pack_conv3x3_mxfp8(blk.out_layers[3].weight.detach()), pk["b2"], n=n, H=H, W=W, cin=cout, residual=res, **kw2)
        else:
            a = ops.group_norm(h.view(n, H * W, cout), *pk["g2"], True, stats=stats)
            y = ops.conv2d(a.view(n, H, W, cout), pk["w2s"], pk["b2s"], kh=3, kw=3, tail=[x.reshape(M, -1)] + ([] if x2 is None else [x2.reshape(M, -1)]), **kw2)
        cs = kw2.get("colstats")
        if temporal:
            y, cs = blk.temopral_conv(y.view(B, fpv, H * W, cout), colstats=cs, want_colstats=want, target=tch)
            y = y.view(n, H, W, -1)
    torch.cuda.synchronize()
    assert ymx.shape == y.shape == y16.shape
    ymx, y, y16 = ymx[..., :cout], y[..., :cout], y16[..., :cout]          # (a concat target's right columns are not this block's)
    assert torch.equal(ymx, y), f"the block differs from the chain of its ops in {int((ymx != y).sum())} elements"
    assert (csmx is None) == (cs is None) == (cs16 is None)
    if cs is not None:
        assert torch.equal(csmx[:, :cout], cs[:, :cout])
    if call == "target":
        assert ymx.data_ptr() == tmx.data.data_ptr() and csmx is tmx.moments and ymx.stride(2) == tmx.data_ld
    assert sorted(blk._mx) == (["w1", "w2"] if conv2_mx else ["w1"])
    assert torch.isfinite(ymx).all() and not torch.equal(ymx, y16), "the MX route did not run"
    print(f"\n[mxfp8] ResBlock {kind} keep_fold={keep_fold} {call}: rel-L2(MX - fp16) of the output = {rel_l2(ymx.float(), y16.float()):.3e}")


def test_block_keeps_fp16_at_a_skipped_width(monkeypatch):
    U, blk = _block(64, 64)
    x = (R.randn((4, 8, 8, 64), 7500) * 1.3).half().to(DEV)
    emb = R.randn((2, EMB), 7502).half().to(DEV)
    with torch.no_grad():
        y16, _ = blk(x, emb, batch_size=2)
        monkeypatch.setattr(U, "RESCONV_MXFP8", True)
        monkeypatch.setattr(U, "RESCONV_MXFP8_SKIP_DIMS", frozenset([64]))
        kept, _ = blk(x, emb, batch_size=2)
        assert blk._mx == {}, "an MX pack was built at a skipped width"
        monkeypatch.setattr(U, "RESCONV_MXFP8_SKIP_DIMS", frozenset())
        ymx, _ = blk(x, emb, batch_size=2)
    torch.cuda.synchronize()
    assert torch.equal(kept, y16) and sorted(blk._mx) == ["w1", "w2"]
    assert torch.isfinite(ymx).all() and not torch.equal(ymx, y16)


# ------------------------------------------------------------------------------------------------------------------ 8. tiny UNet
def _tiny_unet():
    from tests.tiny_config import TINY_UNET
    from tests.util import load_synth
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    return m.to(DEV), TINY_UNET


def _tiny_inputs(cfg, tag):
    from oracle.weights import synth_input
    t, h, w, L = 4, 16, 32, 77 + 64
    x = synth_input(f"{tag}_x", (2, 8, t, h, w)).to(DEV)
    x[1] = x[0]
    ctx = synth_input(f"{tag}_ctx", (2, L, cfg["context_dim"])).to(DEV)
    return x, ctx, torch.tensor([799, 799], device=DEV), torch.tensor([10, 10], device=DEV)


@pytest.mark.parametrize("keep_fold", [True, False])
def test_tiny_unet_with_the_switch_on_and_off(monkeypatch, keep_fold):
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    m, cfg = _tiny_unet()
    x, ctx, ts, fs = _tiny_inputs(cfg, "rmx")
    with torch.no_grad():
        before = m._forward(x, ts, context=ctx, fs=fs)             # the module flag has never been touched
        monkeypatch.setattr(U, "RESCONV_MXFP8", True)
        monkeypatch.setattr(U, "RESCONV_MXFP8_SKIP_DIMS", frozenset())
        monkeypatch.setattr(U, "RESCONV_MXFP8_KEEP_FOLD", keep_fold)
        on = m._forward(x, ts, context=ctx, fs=fs)
        ones = torch.cat([m._forward(x[i:i + 1].contiguous(), ts[:1], context=ctx[i:i + 1].contiguous(), fs=fs[:1]) for i in range(2)])
        shared = m._forward(x[:1].contiguous(), ts[:1], context=ctx, fs=fs[:1], cfg_repeat=2)
        monkeypatch.setattr(U, "RESCONV_MXFP8", False)
        off = m._forward(x, ts, context=ctx, fs=fs)
    torch.cuda.synchronize()
    blocks = [b for b in m.modules() if isinstance(b, U.ResBlock)]
    assert sum(bool(b._mx) for b in blocks) > 0
    assert torch.isfinite(on).all()
    assert not torch.equal(on, before), "the switch changed nothing: the MX route did not run"
    assert torch.equal(ones, on), f"B = 2 differs from two B = 1 forwards in {int((ones != on).sum())} elements"
    assert torch.equal(shared, on), f"the shared CFG prefix differs from the replicated batch in {int((shared != on).sum())} elements"
    assert torch.equal(off, before), f"switch off: {int((off != before).sum())} elements differ from the run before it was ever on"
    print(f"\n[mxfp8] tiny UNet, ResBlock convolutions (keep_fold={keep_fold}): rel-L2(on - off) = {rel_l2(on, off):.3e}")


def test_tiny_unet_with_all_three_mx_switches(monkeypatch):
    from viewcrafter_amd.lvdm.modules import attention as A
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    m, cfg = _tiny_unet()
    x, ctx, ts, fs = _tiny_inputs(cfg, "rmx3")
    for mod, name in ((U, "RESCONV_MXFP8"), (U, "TCONV_MXFP8"), (A, "FF_MXFP8")):
        monkeypatch.setattr(mod, name, True)
        monkeypatch.setattr(mod, name + "_SKIP_DIMS", frozenset())
    with torch.no_grad():
        on = m._forward(x, ts, context=ctx, fs=fs)
        ones = torch.cat([m._forward(x[i:i + 1].contiguous(), ts[:1], context=ctx[i:i + 1].contiguous(), fs=fs[:1]) for i in range(2)])
    torch.cuda.synchronize()
    assert torch.isfinite(on).all()
    assert torch.equal(ones, on), f"B = 2 differs from two B = 1 forwards in {int((ones != on).sum())} elements"


def test_tiny_unet_with_the_switch_on_replays_from_a_captured_graph(monkeypatch):
    """The MX route is capturable: the packs (host code) are built by the warm-up forward ahead of the capture, the predicate touches no
    device, nothing on the path synchronises.  The replay is bit-equal to the eager forward, also with new inputs."""
    from oracle.weights import synth_input
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    m, cfg = _tiny_unet()
    monkeypatch.setattr(U, "RESCONV_MXFP8", True)
    monkeypatch.setattr(U, "RESCONV_MXFP8_SKIP_DIMS", frozenset())
    T, h, w = 4, 16, 32
    ctx = synth_input("rmxg_ctx", (2, 77 + 16 * T, cfg["context_dim"])).to(DEV)
    fs = torch.tensor([10, 10], device=DEV)
    try:
        for k, tval in enumerate((999, 479)):
            x = synth_input(f"rmxg_x{k}", (2, cfg["in_channels"], T, h, w)).to(DEV)
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
