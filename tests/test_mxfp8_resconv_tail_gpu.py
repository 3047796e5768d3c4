"""The ResBlock skip convolution as a K tail of the MXFP8 3x3 convolution on the GPU (VCX_RESCONV_MXFP8_TAIL; include/vcx.h
vcx_groupnorm_apply(2)_mxfp8_raw_f16 / vcx_conv3x3_tail_mxfp8): the raw second output of the quantising GroupNorm apply byte for byte, the
tailed convolution on operands with exactly known products (a tail read from a neighbouring row, a scale byte from the wrong part or a
dropped padding block is an exact mismatch), its identities against the untailed kernels, both tile configurations, its rounding quality,
pitches, moments, a tail source past 2^31 bytes, ResBlock against the chain of its ops, and the tiny UNet with the switch on and off."""
import os
import subprocess
import sys

import pytest
import torch

from tests import cpu_kernels_mx_tail as CT
from tests import mx_emulation as MX
from tests import mxfp8_resconv_tail_cases as C
from tests import rounding_quality as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xAB
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_pair = C.pair


def _first_diff(got, want):
    bad = torch.nonzero(got != want)
    return f"{bad.shape[0]} of {got.numel()} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}"


def _bytes_equal(got, want, name):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert torch.equal(got, want), f"{name}: {_first_diff(got, want)}"


def _assert_fp16_bits(out, ref64, name):
    got, want = out.cpu(), ref64.half()
    assert got.dtype == torch.float16 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{name}: {_first_diff(got, want)}"


def _same_bits(a, b, name):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, name
    view = torch.int16 if a.dtype == torch.float16 else torch.int32
    assert torch.equal(a.view(view), b.view(view)), f"{name}: {int((a != b).sum())} of {a.numel()} elements differ"


# ------------------------------------------------------------------------------------------------------------------ 1. the raw quantiser
# (n_outer, pixels, c1, c2): Kp 128 with 32 padding bytes | 320 | an MX block (channels 32 .. 63) straddles the halves | 64 | 256
RAW_CASES = [(2, 37, 96, 0), (3, 64, 320, 0), (2, 37, 40, 56), (2, 50, 64, 256)]


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("n_outer,pixels,c1,c2", RAW_CASES)
def test_raw_quantiser_writes_the_parents_bytes_and_the_quantised_input(n_outer, pixels, c1, c2, silu):
    """(q, s): the non-raw entry point's bytes.  (rq, rs): ops.quant_mxfp8 of the (concatenated) input, padding included.  The input carries
    the format's boundary blocks (tests/mx_emulation.plant_boundaries: powers of two, the clamp, subnormals, inf, NaN) and an all-zero block;
    the statistics are those of the tensor before the blocks were planted, so that the normalised values stay finite elsewhere."""
    from viewcrafter_amd import _lib, ops
    C_ = c1 + c2
    rows, kp = n_outer * pixels, MX.kp_of(C_)
    x = (R.randn((n_outer, pixels, C_), 10 + C_ + pixels) * 1.7 + 0.3).half()
    stats = ops.group_norm_stats(x.to(DEV))
    where = MX.plant_boundaries(x.view(rows, C_))
    x.view(rows, C_)[rows - 1, C_ - 32:] = 0.0                        # an all-zero block in the last row: scale byte 0
    assert len(where) == len(MX.boundary_blocks()) and "nan" in where
    gamma, beta = (1.0 + 0.3 * R.randn((C_,), 11)).to(DEV), (0.2 * R.randn((C_,), 12)).to(DEV)
    x1 = x[..., :c1].contiguous().to(DEV)
    x2 = x[..., c1:].contiguous().to(DEV) if c2 else None
    # one guard row in front and behind each of the four outputs, everything poisoned
    bufs = [torch.full((rows + 2, w), POISON, dtype=torch.uint8, device=DEV) for w in (kp, kp // 32, kp, kp // 32)]
    q, s, rq, rs = bufs
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    if c2:
        _lib.check(L.vcx_groupnorm_apply2_mxfp8_raw_f16(x1.data_ptr(), c1, x2.data_ptr(), q[1].data_ptr(), s[1].data_ptr(), rq[1].data_ptr(), rs[1].data_ptr(),
                                                        stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), n_outer, pixels, C_, 32, 1e-5, 1 if silu else 0, st))
    else:
        _lib.check(L.vcx_groupnorm_apply_mxfp8_raw_f16(x1.data_ptr(), q[1].data_ptr(), s[1].data_ptr(), rq[1].data_ptr(), rs[1].data_ptr(), stats.data_ptr(),
                                                       gamma.data_ptr(), beta.data_ptr(), n_outer, pixels, C_, 32, 1e-5, 1 if silu else 0, st))
    pq, ps = ops.group_norm_mxfp8(x1, gamma, beta, 1e-5, silu, stats=stats, x2=x2)
    xq, xs = ops.quant_mxfp8(x.view(rows, C_).to(DEV))
    (oq, os_), (orq, ors) = ops.group_norm_mxfp8_raw(x1, gamma, beta, 1e-5, silu, stats=stats, x2=x2)
    torch.cuda.synchronize()
    _bytes_equal(q[1:-1], pq, "elements against the non-raw entry point")
    _bytes_equal(s[1:-1], ps, "scales against the non-raw entry point")
    _bytes_equal(rq[1:-1], xq, "raw elements against quant_mxfp8 of the input")
    _bytes_equal(rs[1:-1], xs, "raw scales against quant_mxfp8 of the input")
    for b in bufs:
        assert bool((b[0] == POISON).all()) and bool((b[-1] == POISON).all()), "a guard row was written"
    for got, want, name in ((oq, pq, "q"), (os_, ps, "s"), (orq, xq, "rq"), (ors, xs, "rs")):
        _bytes_equal(got, want, f"ops.group_norm_mxfp8_raw {name}")
    # ... and the raw pair against the torch definition: boundary blocks, the zero block and the padding
    eq, es = MX.quant(x.view(rows, C_))
    _bytes_equal(xq, eq, "raw elements against the torch definition")
    _bytes_equal(xs, es, "raw scales against the torch definition")
    assert not bool(rq[1:-1, C_:].any()) and bool((rs[1:-1, C_ // 32:] == 127).all()), "padding: element bytes 0x00, scale bytes 127 up to Kp"
    assert int(rs[rows, C_ // 32 - 1]) == 0 and not bool(rq[rows, C_ - 32:C_].any()), "the all-zero block"
    r, b = where["nan"]
    assert int(rs[1 + r, b]) == 255 and bool((rq[1 + r, 32 * b:32 * b + 32] == 0x7F).all())


# ------------------------------------------------------------------------------------------------------------------ 2. exact arithmetic
# M = 105 < one tile, two tail K-steps of which the second is three-quarters padding, ragged N | three row tiles (the last ragged), two
# slabs, the wide tile | the same geometry with one and a half square tiles
EXACT_CASES = [(3, 5, 7, 32, 160, 24), (2, 9, 16, 160, 96, 320), (2, 9, 16, 160, 96, 192)]


@pytest.mark.parametrize("n,H,W,cin,ct,N", EXACT_CASES)
def test_tailed_convolution_is_exact_on_the_integer_grid(n, H, W, cin, ct, N):
    """out == fp16(bias + the nine taps' sums + the tail's sum) bit for bit.  The tail rows are distinct per row: a tail read from row
    m +- 1, m +- W or the neighbouring frame - or zeroed by a tap's validity bits - shows at the image corners and at frame boundaries."""
    from viewcrafter_amd import ops
    a, t, w9, wt, w, bias = C.exact_problem(n, H, W, cin, ct, N)
    ref = CT.conv_tail_ref(a[2], w9[2], t[2], wt[2], bias, n, H, W)
    assert float(ref.abs().max()) < 65504 and torch.equal(ref / MX.GRID, (ref / MX.GRID).round())
    assert ops.conv3x3_tail_mxfp8_ok(n, H, W, cin, ct, N)
    out = ops.conv3x3_tail_mxfp8(_pair(a), _pair(t), _pair(w), bias.to(DEV), n=n, H=H, W=W, cin=cin, ct=ct)
    torch.cuda.synchronize()
    assert out.shape == (n, H, W, N)
    _assert_fp16_bits(out.view(n * H * W, N), ref, f"conv3x3_tail_mxfp8 {n}x{H}x{W} {cin}+{ct}->{N}")
    # the emulation the other tests compare with is the same function
    emu = CT.conv3x3_tail_mxfp8((a[0], a[1]), (t[0], t[1]), w, bias, n=n, H=H, W=W, cin=cin, ct=ct)
    assert torch.equal(emu.view(-1, N), ref.half())


def test_pack_feeds_the_kernel_the_order_it_reads():
    """packing.pack_conv3x3_tail_mxfp8 of the exact weights (every value an exact MXFP8 value: the pack is lossless) gives the same bits."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv3x3_tail_mxfp8
    n, H, W, cin, ct, N = EXACT_CASES[0]
    a, t, w9, wt, _, bias = C.exact_problem(n, H, W, cin, ct, N)
    w3 = w9[2].view(N, 3, 3, cin).permute(0, 3, 1, 2).contiguous().float()
    w1 = wt[2].view(N, ct, 1, 1).float()
    ref = CT.conv_tail_ref(a[2], w9[2], t[2], wt[2], bias, n, H, W)
    out = ops.conv3x3_tail_mxfp8(_pair(a), _pair(t), _pair(pack_conv3x3_tail_mxfp8(w3, w1)), bias.to(DEV), n=n, H=H, W=W, cin=cin, ct=ct)
    torch.cuda.synchronize()
    _assert_fp16_bits(out.view(n * H * W, N), ref, "conv3x3_tail_mxfp8 on pack_conv3x3_tail_mxfp8's weights")


# ------------------------------------------------------------------------------------------------------------------ 3. identities
def _zeros_like_pair(p):
    return torch.zeros_like(p[0]), torch.full_like(p[1], 127)


@pytest.mark.parametrize("N", [136, 320])
def test_zero_tail_weights_give_the_untailed_convolution_and_zero_main_weights_the_linear_gemm(N):
    from viewcrafter_amd import ops
    n, H, W, cin, ct = 2, 8, 16, 160, 96
    M, kp = n * H * W, MX.kp_of(cin)
    a, t, w, bias = C.random_problem(n, H, W, cin, ct, N, 300 + N)
    main = (w[0][:, :9 * kp].contiguous(), w[1][:, :9 * kp // 32].contiguous())
    tail = (w[0][:, 9 * kp:].contiguous(), w[1][:, 9 * kp // 32:].contiguous())
    kw = dict(n=n, H=H, W=W, cin=cin)
    a_, t_, b_ = _pair(a), _pair(t), bias.to(DEV)
    cs, cs0 = torch.zeros((M // 64, N, 2), device=DEV), torch.zeros((M // 64, N, 2), device=DEV)
    y = ops.conv3x3_tail_mxfp8(a_, t_, _pair(CT.join_weight(main, _zeros_like_pair(tail))), b_, ct=ct, colstats=cs, **kw)
    y0 = ops.conv3x3_mxfp8(a_, _pair(main), b_, colstats=cs0, **kw)
    z = ops.conv3x3_tail_mxfp8(a_, t_, _pair(CT.join_weight(_zeros_like_pair(main), tail)), b_, ct=ct, **kw)
    z0 = ops.linear_mxfp8(t_, _pair(tail), b_, K=ct)
    full = ops.conv3x3_tail_mxfp8(a_, t_, _pair(w), b_, ct=ct, **kw)
    torch.cuda.synchronize()
    assert float(y0.float().abs().max()) > 0.5 and float(z0.float().abs().max()) > 0.5
    _same_bits(y.view(M, N), y0.view(M, N), "zero tail weights against vcx_conv3x3_mxfp8")
    _same_bits(cs, cs0, "... and their moments")
    _same_bits(z.view(M, N), z0.view(M, N), "zero main weights against vcx_gemm_mxfp8 on (t, tail weights)")
    assert not torch.equal(full, y) and not torch.equal(full, z), "both parts enter the tailed convolution"


def _child(path, cfg):
    env = {k: v for k, v in os.environ.items() if k != "VCX_GEMM_MX_CFG"}
    env["VCX_GEMM_MX_CFG"] = cfg
    r = subprocess.run([sys.executable, "-m", "tests.mxfp8_resconv_tail_cases", str(path)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(str(path))


def test_both_tile_configurations_give_the_same_bytes(tmp_path):
    """VCX_GEMM_MX_CFG is read once per process: one child per forced configuration (tests/mxfp8_resconv_tail_cases.py), as
    tests/test_mxfp8_widetile_gpu.py forces them."""
    narrow, wide = _child(tmp_path / "cfg0.pt", "0"), _child(tmp_path / "cfg1.pt", "1")
    assert sorted(narrow) == sorted(wide) and len(narrow) == 4 * len(C.CFG_CASES) + 1
    for k in narrow:
        if k.endswith(" cfg"):
            assert narrow[k].item() == 0 and wide[k].item() == 1, "the knob forces the configuration"
            continue
        _same_bits(narrow[k], wide[k], k)
        b = wide[k]
        if k.endswith("moments"):
            N = int(k.split(" N")[1].split()[0])
            assert bool((b[:, :32] == 5.0).all()) and bool((b[:, 32 + N:] == 5.0).all()), f"{k}: moments written outside their columns"
            assert bool(torch.isfinite(b[:, 32:32 + N]).all()) and not bool((b[:, 32:32 + N, 0] == 5.0).all()), f"{k}: moments not written"
        elif k.startswith("tail") and not k.endswith("plain"):
            N = int(k.split(" N")[1].split()[0])
            assert bool((b[0] == C.GUARD).all()) and bool((b[-1] == C.GUARD).all()) and bool((b[:, N:] == C.GUARD).all()), f"{k}: a guard element was written"
            assert bool(torch.isfinite(b).all()) and not bool((b[1:-1, :N] == C.GUARD).any()) and float(b[1:-1, :N].float().abs().max()) > 0.1, k
            _same_bits(b[1:-1, :N], wide[k + " plain"], f"{k}: the strided output against the dense one")
    n, H, W, cin, ct, N = 2, 9, 16, 160, 96, 320
    a, t, w9, wt, _, bias = C.exact_problem(n, H, W, cin, ct, N)
    _assert_fp16_bits(wide["exact"], CT.conv_tail_ref(a[2], w9[2], t[2], wt[2], bias, n, H, W), "the wide tile on exact operands")


@pytest.mark.parametrize("N", [72, 320])
def test_the_first_frames_of_a_longer_call_are_the_shorter_call(N):
    from viewcrafter_amd import ops
    n, H, W, cin, ct = 3, 8, 8, 64, 160                          # 192 rows; the 2 n-frame call has 384: other tiles hold the same rows
    F, M = H * W, n * H * W
    a, t, w, bias = C.random_problem(2 * n, H, W, cin, ct, N, 400 + N)
    w_, b_ = _pair(w), bias.to(DEV)
    rows = lambda p, m: (p[0][:m].contiguous().to(DEV), p[1][:m].contiguous().to(DEV))
    cs2, cs1 = torch.zeros((2 * M // 64, N, 2), device=DEV), torch.zeros((M // 64, N, 2), device=DEV)
    both = ops.conv3x3_tail_mxfp8(rows(a, 2 * M), rows(t, 2 * M), w_, b_, n=2 * n, H=H, W=W, cin=cin, ct=ct, colstats=cs2).view(2 * M, N)
    half = ops.conv3x3_tail_mxfp8(rows(a, M), rows(t, M), w_, b_, n=n, H=H, W=W, cin=cin, ct=ct, colstats=cs1).view(M, N)
    one = ops.conv3x3_tail_mxfp8(rows(a, F), rows(t, F), w_, b_, n=1, H=H, W=W, cin=cin, ct=ct).view(F, N)
    torch.cuda.synchronize()
    assert torch.isfinite(both).all() and float(both.float().abs().max()) > 0.5
    _same_bits(both[:M], half, "the first n frames of the 2 n-frame call")
    _same_bits(cs2[:M // 64], cs1, "... and their moment strips")
    _same_bits(half[:F], one, "the first frame alone")


# ------------------------------------------------------------------------------------------------------------------ 4. one rounding
@pytest.mark.parametrize("N", [64, 160])
def test_tailed_convolution_rounds_once(N):
    """Random MXFP8 operands against the fp64 value of the dequantised operands: fp32 accumulation over main and tail, rounded once -
    E <= 1.05 (tests/rounding_quality.check_rounding; 65536 and 163840 outputs)."""
    from viewcrafter_amd import ops
    n, H, W, cin, ct = 2, 16, 32, 64, 128
    M = n * H * W
    a, t, w, bias = C.random_problem(n, H, W, cin, ct, N, 500 + N, spread=1)
    out = ops.conv3x3_tail_mxfp8(_pair(a), _pair(t), _pair(w), bias.to(DEV), n=n, H=H, W=W, cin=cin, ct=ct)
    torch.cuda.synchronize()
    w9, wt = CT.split_weight(w, cin, ct)
    ref = CT.conv_tail_ref(MX.dequant(a[0], a[1], cin), w9, MX.dequant(t[0], t[1], ct), wt, bias, n, H, W)
    R.check_rounding("conv3x3_tail_mxfp8", f"{n}x{H}x{W} {cin}+{ct}->{N}", out.view(M, N).cpu(), ref)


# ------------------------------------------------------------------------------------------------------------------ 5. pitches
def test_output_into_a_wider_buffer_leaves_the_guard_columns_alone():
    from viewcrafter_amd import ops
    n, H, W, cin, ct, N = EXACT_CASES[1]
    M, ldc = n * H * W, N + 24
    a, t, w9, wt, w, bias = C.exact_problem(n, H, W, cin, ct, N)
    ref = CT.conv_tail_ref(a[2], w9[2], t[2], wt[2], bias, n, H, W)
    buf = torch.full((M + 2, ldc), 777.0, dtype=torch.float16, device=DEV)          # + a guard row in front and behind
    assert ops.conv3x3_tail_mxfp8_ok(n, H, W, cin, ct, N, ldc=ldc)
    ops.conv3x3_tail_mxfp8(_pair(a), _pair(t), _pair(w), bias.to(DEV), n=n, H=H, W=W, cin=cin, ct=ct, out=buf[1:M + 1], ldc=ldc)
    torch.cuda.synchronize()
    _assert_fp16_bits(buf[1:M + 1, :N].contiguous(), ref, "conv3x3_tail_mxfp8, ldc = N + 24")
    assert bool((buf[:, N:] == 777.0).all()), "a guard column was written"
    assert bool((buf[0] == 777.0).all()) and bool((buf[-1] == 777.0).all()), "a guard row was written"


@pytest.mark.parametrize("N", [128, 320])
def test_column_moments_feed_the_groupnorm_behind_the_tailed_convolution(N):
    """Moments at ldcs > N behind a first column: the statistics from them against group_norm_stats of the output and against fp64, to the
    tolerances of test_column_moments_feed_the_groupnorm_behind_the_convolution (2e-6 of the mean's magnitude, 2e-5 rel-L2 of the variance)."""
    from tests.test_mxfp8_tconv_gpu import _strip_moments_ok
    from viewcrafter_amd import ops
    n, H, W, cin, ct = 2, 8, 16, 128, 96
    M, ld, col = n * H * W, N + 64, 32
    a, t, w, bias = C.random_problem(n, H, W, cin, ct, N, 600 + N)
    a_, t_, w_, b_ = _pair(a), _pair(t), _pair(w), bias.to(DEV)
    kw = dict(n=n, H=H, W=W, cin=cin, ct=ct)
    assert ops.conv3x3_tail_mxfp8_ok(n, H, W, cin, ct, N, ldc=ld, colstats=True, colstats_ld=ld, colstats_col=col)
    cat = torch.full((M, ld), 3.0, dtype=torch.float16, device=DEV)
    guard = torch.full((M // 64 + 2, ld, 2), 5.0, device=DEV)      # the moments buffer with two sentinel strips behind it
    cat_cs = guard[:M // 64]
    ops.conv3x3_tail_mxfp8(a_, t_, w_, b_, out=cat, ldc=ld, colstats=cat_cs, colstats_ld=ld, colstats_col=col, **kw)
    cs = torch.zeros((M // 64, N, 2), device=DEV)
    y = ops.conv3x3_tail_mxfp8(a_, t_, w_, b_, colstats=cs, **kw).view(M, N)
    plain = ops.conv3x3_tail_mxfp8(a_, t_, w_, b_, **kw).view(M, N)
    torch.cuda.synchronize()
    assert torch.equal(y, plain), "the moments are a by-product: the output does not change"
    assert torch.equal(cat[:, :N], y) and bool((cat[:, N:] == 3.0).all())
    assert torch.equal(cat_cs[:, col:col + N], cs), "the same moments, bit for bit, wherever they are written"
    assert bool((cat_cs[:, :col] == 5.0).all()) and bool((cat_cs[:, col + N:] == 5.0).all()) and bool((guard[M // 64:] == 5.0).all())
    _strip_moments_ok(cs.cpu(), y.cpu())
    for n_outer, pixels in ((n, H * W), (1, n * H * W)):
        st = ops.group_norm_stats_from_colstats(cat_cs[:, col:col + N].contiguous(), n_outer, pixels, N)
        direct = ops.group_norm_stats(y.view(n_outer, pixels, N))
        yd = y.double().view(n_outer, pixels, 32, N // 32)
        mean, var = yd.mean(dim=(1, 3)), yd.var(dim=(1, 3), unbiased=False)
        for other in (direct.double(), torch.stack([mean, var], dim=-1)):
            assert float((st[..., 0].double() - other[..., 0]).abs().max()) <= 2e-6 * float(mean.abs().max() + 1)
            assert rel_l2(st[..., 1], other[..., 1]) <= 2e-5


# ------------------------------------------------------------------------------------------------------------------ 6. extents
def test_a_tail_source_past_2_31_bytes():
    """(1, 1100, 2048), Cin 32, Ct 1024, N 8: the tail source holds 2 306 867 200 bytes (> 2^31, < 2^32).  One call on integer-grid operands;
    the rows of the first and of the last row tile equal the emulation, computed on the two image rows they need."""
    from viewcrafter_amd import ops
    n, H, W, cin, ct, N = 1, 1100, 2048, 32, 1024, 8
    M, period = n * H * W, 2 * W
    assert (1 << 31) < M * ct < (1 << 32) and M % period == 0 and M % 128 == 0
    assert ops.conv3x3_tail_mxfp8_ok(n, H, W, cin, ct, N)
    # two image rows = `period` rows of operands, repeated down the frame; the last two image rows get operands of their own, so that a tail
    # offset that wrapped modulo 2^31 or 2^32 cannot land on equal bytes (the weights are the same draws: the seed moves the sources only)
    a, t, w9, wt, w, bias = C.exact_problem(1, 2, W, cin, ct, N)
    a2, t2, _, _, _, _ = C.exact_problem(1, 2, W, cin, ct, N, seed=7)
    assert not torch.equal(t[0], t2[0]) and not torch.equal(a[0], a2[0])
    aq, asc = (p.to(DEV).repeat(M // period, 1) for p in a[:2])
    tq, tsc = (p.to(DEV).repeat(M // period, 1) for p in t[:2])
    aq[M - period:], asc[M - period:] = a2[0].to(DEV), a2[1].to(DEV)
    tq[M - period:], tsc[M - period:] = t2[0].to(DEV), t2[1].to(DEV)
    out = ops.conv3x3_tail_mxfp8((aq, asc), (tq, tsc), _pair(w), bias.to(DEV), n=n, H=H, W=W, cin=cin, ct=ct).view(M, N)
    torch.cuda.synchronize()
    first, last = out[:128].cpu(), out[M - 128:].cpu()
    del aq, asc, tq, tsc, out
    # image row 0 of the frame: its lower neighbour is row 1 of the period; image row H - 1: its upper neighbour is row 0 of the last period
    _assert_fp16_bits(first, CT.conv_tail_ref(a[2], w9[2], t[2], wt[2], bias, 1, 2, W)[:128], "the first row tile")
    _assert_fp16_bits(last, CT.conv_tail_ref(a2[2], w9[2], t2[2], wt[2], bias, 1, 2, W)[period - 128:], "the last row tile")


# ------------------------------------------------------------------------------------------------------------------ 7. ResBlock
from tests.test_mxfp8_resconv_gpu import BLOCKS, EMB, _block, _host_colstats, _tiny_inputs, _tiny_unet      # noqa: E402


def _switches(monkeypatch, U, resconv, tail, keep_fold=False):
    monkeypatch.setattr(U, "RESCONV_MXFP8", resconv)
    monkeypatch.setattr(U, "RESCONV_MXFP8_SKIP_DIMS", frozenset())
    monkeypatch.setattr(U, "RESCONV_MXFP8_KEEP_FOLD", keep_fold)
    monkeypatch.setattr(U, "RESCONV_MXFP8_TAIL", tail)


@pytest.mark.parametrize("call", ["plain", "target", "want_colstats"])
@pytest.mark.parametrize("kind", ["skip_conv", "split_concat"])
def test_block_on_the_tail_route_is_the_composition_of_its_ops(kind, call, monkeypatch):
    from viewcrafter_amd import ops
    from viewcrafter_amd.lvdm.modules.flow import CatTarget
    from viewcrafter_amd.packing import pack_conv3x3_mxfp8, pack_conv3x3_tail_mxfp8
    c1, c2, cout, _ = BLOCKS[kind]
    cin = c1 + c2
    U, blk = _block(cin, cout)
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
        y16, cs16 = blk(x, emb, **kwargs(mk_target()))
        y16 = y16.clone()
        _switches(monkeypatch, U, True, False)
        ymx, _ = blk(x, emb, **kwargs(mk_target()))
        ymx = ymx.clone()
        blk._mx = {}
        _switches(monkeypatch, U, True, True)
        ttl = mk_target()
        ytl, cstl = blk(x, emb, **kwargs(ttl))
        packs = sorted(blk._mx)
        # the chain, written out
        pk = blk.packed()
        tch = mk_target()
        stats_in = None if cs_in is None else ops.group_norm_stats_from_colstats(cs_in, n, H * W, cin)
        a, xq = ops.group_norm_mxfp8_raw(x.view(n, H * W, c1), *pk["g1"], True, stats=stats_in, x2=None if x2 is None else x2.view(n, H * W, c2))
        emb_out = ops.linear(emb, pk["we"], pk["be"], out_f32=True)
        cs1 = ops.colstats_buffer(M, cout, DEV)
        h = ops.conv3x3_mxfp8(a, pack_conv3x3_mxfp8(blk.in_layers[2].weight.detach()), pk["b1"], n=n, H=H, W=W, cin=cin, rowadd=emb_out, rowadd_div=fpv * H * W,
                              colstats=cs1)
        stats = ops.group_norm_stats_from_colstats(cs1, n, H * W, cout)
        kw2 = tch.kwargs(cout, M) if tch is not None else (dict(colstats=ops.colstats_buffer(M, cout, DEV)) if want else {})
        a2 = ops.group_norm_mxfp8(h.view(n, H * W, cout), *pk["g2"], True, stats=stats)
        w2s = pack_conv3x3_tail_mxfp8(blk.out_layers[3].weight.detach(), blk.skip_connection.weight.detach())
        y = ops.conv3x3_tail_mxfp8(a2, tail=xq, w=w2s, bias=pk["b2s"], n=n, H=H, W=W, cin=cout, ct=cin, **kw2)
        cs = kw2.get("colstats")
        # the raw pair is the quantised (concatenated) input
        xcat = x if x2 is None else torch.cat([x, x2], dim=-1)
        xq_ref = ops.quant_mxfp8(xcat.reshape(M, cin).contiguous())
    torch.cuda.synchronize()
    assert ytl.shape == y.shape == y16.shape
    ytl, y, y16, ymx = ytl[..., :cout], y[..., :cout], y16[..., :cout], ymx[..., :cout]          # (a concat target's right columns are not this block's)
    assert torch.equal(ytl, y), f"the block differs from the chain of its ops in {int((ytl != y).sum())} elements"
    assert (cstl is None) == (cs is None) == (cs16 is None)
    if cs is not None:
        assert torch.equal(cstl[:, :cout], cs[:, :cout])
    if call == "target":
        assert ytl.data_ptr() == ttl.data.data_ptr() and cstl is ttl.moments and ytl.stride(2) == ttl.data_ld
    assert packs == ["w1", "w2s"]
    assert torch.equal(xq[0], xq_ref[0]) and torch.equal(xq[1], xq_ref[1])
    assert torch.isfinite(ytl).all() and not torch.equal(ytl, y16) and not torch.equal(ytl, ymx), "the tail route did not run"
    e16, emx = rel_l2(ytl.float(), y16.float()), rel_l2(ytl.float(), ymx.float())
    print(f"\n[mxfp8] ResBlock {kind} {call}, skip convolution as the K tail: rel-L2 against the fp16 block {e16:.3e}, against the shipped MX block {emx:.3e}")


# ------------------------------------------------------------------------------------------------------------------ 8. tiny UNet
def test_tiny_unet_with_the_tail_switch_on_and_off(monkeypatch):
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    m, cfg = _tiny_unet()
    x, ctx, ts, fs = _tiny_inputs(cfg, "rmxt")
    with torch.no_grad():
        _switches(monkeypatch, U, True, False)
        before = m._forward(x, ts, context=ctx, fs=fs)             # RESCONV_MXFP8 alone; the new flag has never been touched
        blocks = [b for b in m.modules() if isinstance(b, U.ResBlock)]
        assert not any("w2s" in b._mx for b in blocks)
        _switches(monkeypatch, U, True, True)
        on = m._forward(x, ts, context=ctx, fs=fs)
        ones = torch.cat([m._forward(x[i:i + 1].contiguous(), ts[:1], context=ctx[i:i + 1].contiguous(), fs=fs[:1]) for i in range(2)])
        shared = m._forward(x[:1].contiguous(), ts[:1], context=ctx, fs=fs[:1], cfg_repeat=2)
        _switches(monkeypatch, U, True, False)
        off = m._forward(x, ts, context=ctx, fs=fs)
    torch.cuda.synchronize()
    tailed = [b for b in blocks if "w2s" in b._mx]
    assert tailed and all(not isinstance(b.skip_connection, torch.nn.Identity) for b in tailed)
    assert torch.isfinite(on).all()
    assert not torch.equal(on, before), "the switch changed nothing: the tail route did not run"
    assert torch.equal(ones, on), f"B = 2 differs from two B = 1 forwards in {int((ones != on).sum())} elements"
    assert torch.equal(shared, on), f"the shared CFG prefix differs from the replicated batch in {int((shared != on).sum())} elements"
    assert torch.equal(off, before), f"switch off again: {int((off != before).sum())} elements differ from the run before it was ever on"
    print(f"\n[mxfp8] tiny UNet, skip convolutions as K tails: rel-L2(on - RESCONV_MXFP8 alone) = {rel_l2(on, before):.3e}")


def test_tiny_unet_with_every_mx_switch_and_the_tail(monkeypatch):
    from viewcrafter_amd.lvdm.modules import attention as A
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    m, cfg = _tiny_unet()
    x, ctx, ts, fs = _tiny_inputs(cfg, "rmxt5")
    for mod, name in ((U, "RESCONV"), (U, "TCONV"), (A, "FF"), (A, "TATTN"), (A, "SATTN")):
        monkeypatch.setattr(mod, name + "_MXFP8", True)
        monkeypatch.setattr(mod, name + "_MXFP8_SKIP_DIMS", frozenset())
    monkeypatch.setattr(U, "RESCONV_MXFP8_TAIL", True)
    with torch.no_grad():
        on = m._forward(x, ts, context=ctx, fs=fs)
        ones = torch.cat([m._forward(x[i:i + 1].contiguous(), ts[:1], context=ctx[i:i + 1].contiguous(), fs=fs[:1]) for i in range(2)])
    torch.cuda.synchronize()
    assert any("w2s" in b._mx for b in m.modules() if isinstance(b, U.ResBlock))
    assert torch.isfinite(on).all()
    assert torch.equal(ones, on), f"B = 2 differs from two B = 1 forwards in {int((ones != on).sum())} elements"


def test_tiny_unet_with_the_tail_switch_replays_from_a_captured_graph(monkeypatch):
    """The tail route is capturable: the packs (host code) are built by the warm-up forward ahead of the capture, the predicates touch no
    device, nothing on the path synchronises.  The replay is bit-equal to the eager forward, also with new inputs."""
    from oracle.weights import synth_input
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    m, cfg = _tiny_unet()
    _switches(monkeypatch, U, True, True)
    T, h, w = 4, 16, 32
    ctx = synth_input("rmxtg_ctx", (2, 77 + 16 * T, cfg["context_dim"])).to(DEV)
    fs = torch.tensor([10, 10], device=DEV)
    try:
        for k, tval in enumerate((999, 479)):
            x = synth_input(f"rmxtg_x{k}", (2, cfg["in_channels"], T, h, w)).to(DEV)
            t = torch.full((2,), tval, device=DEV, dtype=torch.long)
            m.use_hip_graph = False
            with torch.no_grad():
                eager = m(x, t, context=ctx, fs=fs).clone()
            m.use_hip_graph = True
            with torch.no_grad():
                graphed = m(x, t, context=ctx, fs=fs).clone()
            assert torch.isfinite(eager).all() and torch.equal(eager, graphed), f"replay {k} differs from eager"
        assert len(m._graphs) == 1 and any("w2s" in b._mx for b in m.modules() if isinstance(b, U.ResBlock))
    finally:
        m.use_hip_graph = False
        m._graphs.clear()
