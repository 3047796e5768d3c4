"""Every kernel family where byte offsets pass 2 GiB and 4 GiB, against a reference.

Production reaches two regimes that the per-kernel suite stays below: tensors whose byte offsets lie in [2 GiB, lim) - the 32-bit
kernels (DMA engine, weight-stationary kernels, shared epilogue) compute them in `unsigned` and rely on a descriptor range check
that must not wrap - and operands at or past lim = 0xFFFF0000 (csrc/gemm.hip), where the dispatcher changes to the register-staged
kernel with 64-bit indexing.  Test ids name the regime: `2g` (offsets in [2 GiB, lim)), `lim` (within a tile of the limit),
`past_lim` (an operand or the output at or beyond it).

Rule of the module: every output element of a large call is covered by (1) a plain fp32 / fp64 PyTorch reference of the same
operation formed in chunks (check_rows), or (2) equality with the same entry point called on a slice whose offsets stay below
2 GiB.  Inputs are random and different everywhere (one device generator per tensor, never a tiled block: a read from
`offset mod 2^32` must fetch other values).  Tolerances are the ones tests/test_kernels_gpu.py states for the same operation.
"""
import math
import time

import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import _check_rowstats, _ln_linear_ref, attn_ref, check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIM = 0xFFFF0000
FPIX = 576 * 1024              # pixels of one decoded frame
V = 25 * 72 * 128              # latent rows of one video
GIB = 1 << 30


@pytest.fixture(autouse=True)
def _memory_report(request):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"\n[large-extent] {request.node.name}: peak {torch.cuda.max_memory_allocated() / GIB:.2f} GiB, {time.time() - t0:.1f} s")
    torch.cuda.empty_cache()


def need(gib):
    """skip only when the device cannot hold the case"""
    free, total = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"needs {gib} GiB of device memory, {free / GIB:.1f} of {total / GIB:.1f} GiB free")


def _t(shape, seed, scale=1.0, shift=0.0, dtype=torch.float16):
    """N(shift, scale^2) drawn on the device straight into the target type, 2^28 elements at a time (no full-size fp32 temporary)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.empty(shape, dtype=dtype, device=DEV)
    flat = t.view(-1)
    for i in range(0, flat.numel(), 1 << 28):
        flat[i:i + (1 << 28)].normal_(shift, scale, generator=g)
    return t


def edges(rows, row_bytes, span=4096):
    """row ranges that are always reference-checked: the first rows, the ranges straddling byte offsets 2^31 and 2^32 (where the tensor
    is that long) and the last rows"""
    out = [(0, min(span, rows))]
    for b in (1 << 31, 1 << 32):
        r = b // row_bytes
        if r + span // 2 < rows:
            out.append((max(0, r - span // 2), r + span // 2))
    out.append((max(0, rows - span), rows))
    return out


def check_all(out, ref_rows, tol=2e-3, name="", chunk=65536, block=1 << 18):
    """check_rows over blocks of rows (its finiteness test makes an fp32 copy of what it is given: a block, not 5 GB); the bound then
    holds per block"""
    for r0 in range(0, out.shape[0], block):
        check_rows(out[r0:r0 + block], lambda a, b: ref_rows(r0 + a, r0 + b), tol=tol, name=f"{name} rows {r0}...", chunk=chunk)


def lin_ref(x, w, b=None, res=None, rowadd=None, rowadd_div=1):
    def f(r0, r1):
        ref = x[r0:r1].float() @ w.float().t()
        if b is not None:
            ref = ref + b
        if rowadd is not None:
            ref = ref + rowadd[torch.arange(r0, r1, device=DEV) // rowadd_div]
        if res is not None:
            ref = ref + res[r0:r1].float()
        return ref
    return f


def geglu_ref(x, w, b, nh):
    def f(r0, r1):
        y = x[r0:r1].float() @ w.float().t() + b
        return y[:, :nh] * F.gelu(y[:, nh:])
    return f


def guard_ok(big, M, N, sentinel=3.0):
    return bool((big[M:] == sentinel).all()) and bool((big[:, N:] == sentinel).all())


# ------------------------------------------------------------------------------------------------------------------ GEMM, linear mode
@pytest.mark.parametrize("kind", ["2g_f16_bias_residual", "2g_f32", "2g_geglu"])
def test_gemm_tiled_dma_output_between_2g_and_lim(kind):
    """Tiled DMA engine, M = 2 V rows, K = 64: output (and residual) of 2.36 GB in a padded buffer - 256x320 / 256x256 tiles and the
    tail split; every row against fp32, and the guard band (5 rows, 8 columns) untouched: rows >= M are dropped by the output
    descriptor's range check only while (M + 256) ldc esz has not wrapped."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_geglu
    need(12)
    M, K = 2 * V, 64
    x = _t((M, K), 11)
    if kind == "2g_f16_bias_residual":
        N = 2560
        w, b, res = _t((N, K), 12, 1 / math.sqrt(K)), _t((N,), 13, dtype=torch.float32), _t((M, N), 14)
        big = torch.full((M + 5, N + 8), 3.0, device=DEV, dtype=torch.float16)
        ops.gemm(x, w, M=M, N=N, K=K, lda=K, out=big, ldc=N + 8, bias=b, residual=res, ldr=N)
        assert 2 * M * (N + 8) > 1 << 31 and guard_ok(big, M, N)
        check_all(big[:M, :N], lin_ref(x, w, b, res), name=kind)
    elif kind == "2g_f32":
        N = 1280
        w, b = _t((N, K), 12, 1 / math.sqrt(K)), _t((N,), 13, dtype=torch.float32)
        big = torch.full((M + 5, N + 8), 3.0, device=DEV, dtype=torch.float32)
        ops.gemm(x, w, M=M, N=N, K=K, lda=K, out=big, ldc=N + 8, bias=b, out_f32=True)
        assert 4 * M * (N + 8) > 1 << 31 and guard_ok(big, M, N)
        check_all(big[:M, :N], lin_ref(x, w, b), tol=1e-4, name=kind)
    else:
        Nh = 2560
        w, b = _t((2 * Nh, K), 12, 1 / math.sqrt(K)), _t((2 * Nh,), 13, dtype=torch.float32)
        wg, bg = pack_geglu(w, b)
        big = torch.full((M + 5, Nh + 8), 3.0, device=DEV, dtype=torch.float16)
        ops.gemm(x, wg, M=M, N=2 * Nh, K=K, lda=K, out=big, ldc=Nh + 8, bias=bg, geglu=True)
        assert guard_ok(big, M, Nh)
        check_all(big[:M, :Nh], geglu_ref(x, w, b, Nh), name=kind)


def test_gemm_operand_through_the_row_stride_lim_and_past_lim():
    """A reached through a 4096-element row stride: M = 524000 rows (a_ext 4.2926e9 < lim, DMA engine, row offsets up to 2^32 - 2.4 MB)
    and M = 524400 (a_ext >= lim: the register-staged kernel on a > 4 GiB operand).  Both against fp32 on every row, their common rows
    against each other within the cross-kernel bound."""
    from viewcrafter_amd import ops
    need(8)
    lda, K, N = 4096, 128, 128
    Ma, Mb = 524000, 524400
    assert 2 * ((Ma - 1) * lda + K) < LIM <= 2 * ((Mb - 1) * lda + K)
    buf = _t((Mb, lda), 21)
    w, b = _t((N, K), 22, 1 / math.sqrt(K)), _t((N,), 23, dtype=torch.float32)
    outs = {}
    for tag, M in (("lim", Ma), ("past_lim", Mb)):
        x = buf[:M, :K]
        outs[tag] = ops.linear(x, w, b)
        check_all(outs[tag], lin_ref(x, w, b), name=f"A through lda, {tag}")
    d = outs["lim"].double() - outs["past_lim"][:Ma].double()
    assert float(d.norm() / outs["lim"].double().norm()) <= 5e-4


@pytest.mark.parametrize("kind", ["past_lim_f16_residual_rowadd", "past_lim_f32"])
def test_gemm_output_past_lim_runs_on_the_register_staged_kernel(kind):
    """Output of 5.1 GB (fp16, M = 1 000 000 x 2560) / 4.6 GB (fp32, M = 900 000 x 1280): the register-staged kernel's 64-bit epilogue
    with residual, per-image addend and bias; every row against fp32."""
    from viewcrafter_amd import ops
    need(16)
    K = 64
    if kind == "past_lim_f16_residual_rowadd":
        M, N = 1_000_000, 2560
        x, w, b = _t((M, K), 31), _t((N, K), 32, 1 / math.sqrt(K)), _t((N,), 33, dtype=torch.float32)
        res, ra = _t((M, N), 34), _t((M // 40000, N), 35, dtype=torch.float32)
        assert 2 * M * N >= LIM
        out = ops.linear(x, w, b, residual=res, rowadd=ra, rowadd_div=40000)
        check_all(out, lin_ref(x, w, b, res, ra, 40000), name=kind)
    else:
        M, N = 900_000, 1280
        x, w, b = _t((M, K), 31), _t((N, K), 32, 1 / math.sqrt(K)), _t((N,), 33, dtype=torch.float32)
        assert 4 * M * N >= LIM
        out = ops.linear(x, w, b, out_f32=True)
        check_all(out, lin_ref(x, w, b), tol=1e-4, name=kind)


@pytest.mark.parametrize("videos,regime", [(7, "lim_cap"), (8, "past_lim")])
def test_gemm_clip_batch_cap_geglu_and_the_layer_behind_it(videos, regime):
    """The tensor max_videos_per_forward is sized for: the level-0 feed-forward of a 7-video forward, K = 320 -> GEGLU N = 2560 packed
    (weight-stationary; output 7 V x 1280 = 4.13 GB) and the layer behind it, K = 1280 -> N = 320 reading that operand with bias +
    residual.  With 8 videos the calls must leave the 32-bit routes cleanly and still be right.  Every row against fp32."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_geglu
    need(14)
    M, K, Nh = videos * V, 320, 1280
    assert (2 * (M + 256) * Nh < LIM) == (videos == 7)
    x = _t((M, K), 41)
    w, b = _t((2 * Nh, K), 42, 1 / math.sqrt(K)), _t((2 * Nh,), 43, dtype=torch.float32)
    wg, bg = pack_geglu(w, b)
    h = ops.linear(x, wg, bg, geglu=True)
    check_all(h, geglu_ref(x, w, b, Nh), name=f"GEGLU {regime}")
    w2, b2 = _t((K, Nh), 44, 1 / math.sqrt(Nh)), _t((K,), 45, dtype=torch.float32)
    y = ops.linear(h, w2, b2, residual=x)
    check_all(y, lin_ref(h, w2, b2, x), name=f"FF out {regime}")


@pytest.mark.parametrize("variant", ["2g_bias_residual", "2g_colstats", "2g_rowstats", "2g_units"])
def test_gemm_weight_stationary_320_past_2g(variant):
    """N = K = 320 weight-stationary kernels with 2.18 GB in and out (M = 3 400 000 + 17; 3400 units of 1024 rows for
    vcx_gemm_units_f16): fp32 on every row, the tiled engine (GEMM_WS = 0) bit for bit, column moments / row statistics against fp64
    of the stored tensor."""
    from viewcrafter_amd import ops
    need(12)
    N = K = 320
    M = {"2g_bias_residual": 3_400_000 + 17, "2g_rowstats": 3_400_000 + 17, "2g_colstats": 3_400_064, "2g_units": 3400 * 1024}[variant]
    assert 2 * M * K > 1 << 31
    x, w, b = _t((M, K), 51), _t((N, K), 52, 1 / math.sqrt(K)), _t((N,), 53, dtype=torch.float32)
    if variant == "2g_units":
        units = M // 1024
        wn, bn = _t((units, N, K), 54, 1 / math.sqrt(K)), _t((units, N), 55, dtype=torch.float32)
        out = ops.gemm_units(x, wn, bn, unit_rows=1024)
        for r0, r1 in edges(M, 2 * K, span=4096):
            u0, u1 = r0 // 1024, (r1 + 1023) // 1024
            ref = torch.baddbmm(bn[u0:u1, None].float(), x[u0 * 1024:u1 * 1024].view(-1, 1024, K).float(), wn[u0:u1].float().transpose(1, 2)).view(-1, N)
            check_rows(out[u0 * 1024:u1 * 1024], lambda a, c: ref[a:c], name=f"units rows {r0}")
        # rule (2): every unit equals the same entry point on a block of 200 units (131 MB, offsets far below 2 GiB)
        for u in range(0, units, 200):
            s = slice(u * 1024, (u + 200) * 1024)
            assert torch.equal(out[s], ops.gemm_units(x[s], wn[u:u + 200], bn[u:u + 200], unit_rows=1024)), u
        return
    res = _t((M, N), 56) if variant != "2g_colstats" else None
    kw = dict(residual=res)
    cs = rs = None
    if variant == "2g_colstats":
        guard = torch.full((M // 64 + 4, N, 2), 7.0, device=DEV)
        cs = guard[:M // 64]
        kw["colstats"] = cs
    if variant == "2g_rowstats":
        assert ops.rowstats_ok(M, N, K, ldr=N)
        rs = ops.rowstats_buffer(M, DEV)
        kw["rowstats"] = rs
    out = ops.linear(x, w, b, **kw)
    prev = ops.tune_set("GEMM_WS", 0)
    try:
        tiled = ops.linear(x, w, b, residual=res)
        torch.cuda.synchronize()
    finally:
        ops.tune_set("GEMM_WS", prev)
    assert torch.equal(out, tiled), f"weight-stationary and tiled results differ in {int((out != tiled).sum())} elements"
    del tiled
    check_all(out, lin_ref(x, w, b, res), name=variant)
    if cs is not None:
        assert bool((guard[M // 64:] == 7.0).all()), "column moments written beyond the last strip"
        stats = ops.group_norm_stats_from_colstats(cs, 2, M // 2, N)          # two statistics units of 1 700 032 rows
        for i in range(2):
            yd = out[i * (M // 2):(i + 1) * (M // 2)].double().view(-1, 32, N // 32)
            mean, var = yd.mean(dim=(0, 2)), yd.var(dim=(0, 2), unbiased=False)
            del yd
            assert float((stats[i, :, 0].double() - mean).abs().max()) <= 2e-6 * float(mean.abs().max() + 1), i
            assert float((stats[i, :, 1].double() - var).norm() / var.norm()) <= 2e-5, i
    if rs is not None:
        _check_rowstats(rs, out, 1e-5, variant)


def test_gemm_lnfold_weight_stationary_7_videos_2g():
    """q | k | v projection of a 7-video forward: LayerNorm folded, K = 320 -> N = 960, output 3.1 GB; against fp64 LayerNorm -> Linear."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import fold_layernorm
    need(10)
    M, K, N = 7 * V, 320, 960
    x = _t((M, K), 61, 2.0, 0.4)
    w32, b = _t((N, K), 62, 1 / math.sqrt(K), dtype=torch.float32), _t((N,), 63, 0.2, dtype=torch.float32)
    gamma, beta = 1 + _t((K,), 64, 0.3, dtype=torch.float32), _t((K,), 65, 0.2, dtype=torch.float32)
    wf, colsum, bias_f = fold_layernorm(w32, gamma, beta, None)
    assert ops.lnfold_ok(M, N, K)
    st = ops.row_stats(x, 1e-5)
    out = ops.linear(x, wf, bias_f + b, ln_stats=st, ln_colsum=colsum)
    assert 2 * M * N > 1 << 31
    check_all(out, lambda r0, r1: _ln_linear_ref(x[r0:r1], gamma, beta, w32, None) + b.double(), tol=1e-3, name="LNFOLD 7V vs fp64", chunk=32768)


def test_gemm_lnfold_one_row_below_lim_is_taken_and_at_lim_is_rejected():
    """The Python mirror and the dispatcher on real buffers at the limit itself: 524280 rows of 4096 elements end 8 KB below lim -
    ops.lnfold_ok says yes, so vcx_gemm_f16 must TAKE the flagged call (DMA engine, row offsets up to 2^32 - 73 KB) and be right; one
    row more and both say no."""
    from viewcrafter_amd import ops
    from viewcrafter_amd._lib import VcxError
    from viewcrafter_amd.packing import fold_layernorm
    need(8)
    lda, K, N = 4096, 64, 64
    M = (LIM // 2 - K) // lda + 1
    assert 2 * ((M - 1) * lda + K) < LIM <= 2 * (M * lda + K) and ops.lnfold_ok(M, N, K, lda=lda) and not ops.lnfold_ok(M + 1, N, K, lda=lda)
    buf = _t((M + 1, lda), 71, 2.0, 0.4)
    w32 = _t((N, K), 72, 1 / math.sqrt(K), dtype=torch.float32)
    gamma, beta = 1 + _t((K,), 73, 0.3, dtype=torch.float32), _t((K,), 74, 0.2, dtype=torch.float32)
    wf, colsum, bias_f = fold_layernorm(w32, gamma, beta, None)
    x = buf[:M, :K]
    st = ops.row_stats(x.contiguous(), 1e-5)
    out = ops.linear(x, wf, bias_f, ln_stats=st, ln_colsum=colsum)
    check_all(out, lambda r0, r1: _ln_linear_ref(x[r0:r1], gamma, beta, w32, None), tol=1e-3, name="LNFOLD one row below lim")
    st1 = torch.cat([st, st[-1:]])
    with pytest.raises(VcxError, match="LNFOLD"):
        ops.linear(buf[:, :K], wf, bias_f, ln_stats=st1, ln_colsum=colsum)


# ------------------------------------------------------------------------------------------------------------------ convolutions
def conv_frame_ref(xf, w, b, ups=0):
    """F.conv2d in fp32 of one channels-last frame [H, W, C] -> rows [Ho * Wo, Cout]"""
    xi = xf.float().permute(2, 0, 1)[None]
    if ups:
        xi = F.interpolate(xi, scale_factor=2, mode="nearest")
    y = F.conv2d(xi, w.float(), b, padding=1)
    return y[0].permute(1, 2, 0).reshape(-1, w.shape[0])


@pytest.mark.parametrize("cin,cout,ups,regime", [(128, 128, 0, "2g_dma"), (256, 128, 0, "past_lim_input"), (128, 3, 0, "2g_conv_out_n3"),
                                                 (256, 256, 1, "past_lim_output_upsample")])
def test_conv_vae_decoder_25_frames_576x1024(cin, cout, ups, regime):
    """The VAE decoder's convolutions on all 25 frames of 576 x 1024 in one call, as LatentDiffusion._frames_per_call issues them:
    128 -> 128 (3.77 GB in / out, DMA engine, frame 14 straddles 2^31), 256 -> 128 (7.5 GB input: register-staged gather), 128 -> 3
    (conv_out, N % 8 != 0) and the fused-upsample 256 -> 256 from 288 x 512 (1.9 GB in, 7.5 GB out).  Every frame against F.conv2d in
    fp32, one frame at a time."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv
    need(22)
    n = 25
    H, W = (288, 512) if ups else (576, 1024)
    x = _t((n, H, W, cin), 81)
    wt = _t((cout, cin, 3, 3), 82, 1 / math.sqrt(9 * cin))
    b = _t((cout,), 83, 0.1, dtype=torch.float32)
    y = ops.conv2d(x, pack_conv(wt), b, kh=3, kw=3, ups=ups)
    assert y.shape == (n, 576, 1024, cout)
    for f in range(n):
        ref = conv_frame_ref(x[f], wt, b, ups)
        check_rows(y[f].reshape(-1, cout), lambda a, c: ref[a:c], name=f"conv {cin}->{cout} {regime} frame {f}", chunk=FPIX)
        del ref


def test_conv_unet_level0_7_videos_rowadd_colstats_2g():
    """UNet level 0 of a 7-video forward: 175 frames of 72 x 128, 960 -> 320 over a 3.1 GB input with per-frame addend and column
    moments; output per frame against F.conv2d in fp32, moments -> GroupNorm statistics against fp64 of the stored tensor."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv
    need(10)
    n, H, W, cin, cout = 175, 72, 128, 960, 320
    M = n * H * W
    x = _t((n, H, W, cin), 91)
    wt = _t((cout, cin, 3, 3), 92, 1 / math.sqrt(9 * cin))
    b, ra = _t((cout,), 93, 0.1, dtype=torch.float32), _t((n, cout), 94, 0.2, dtype=torch.float32)
    assert 2 * M * cin > 1 << 31 and ops.colstats_ok(M, H * W, cin, cout, in_rows=M)
    guard = torch.full((M // 64 + 4, cout, 2), 7.0, device=DEV)
    cs = guard[:M // 64]
    y = ops.conv2d(x, pack_conv(wt), b, kh=3, kw=3, rowadd=ra, rowadd_div=H * W, colstats=cs)
    assert bool((guard[M // 64:] == 7.0).all()), "column moments written beyond the last strip"
    for f in range(n):
        ref = conv_frame_ref(x[f], wt, b) + ra[f]
        check_rows(y[f].reshape(-1, cout), lambda a, c: ref[a:c], name=f"conv 960->320 frame {f}", chunk=H * W)
    stats = ops.group_norm_stats_from_colstats(cs, n, H * W, cout)
    yd = y.double().reshape(n, H * W, 32, cout // 32)
    mean, var = yd.mean(dim=(1, 3)), yd.var(dim=(1, 3), unbiased=False)
    assert float((stats[..., 0].double() - mean).abs().max()) <= 2e-6 * float(mean.abs().max() + 1)
    assert float((stats[..., 1].double() - var).norm() / var.norm()) <= 2e-5


# ------------------------------------------------------------------------------------------------------------------ GroupNorm / LayerNorm
@pytest.mark.parametrize("n,pixels,C,offset,regime", [(25, FPIX, 128, 0.0, "2g_vae_128"), (25, FPIX, 256, 0.0, "past_lim_vae_256"),
                                                      (7, V, 1280, 0.0, "lim_7_videos_1280"), (25, FPIX, 128, 60.0, "2g_vae_128_common_offset")])
def test_groupnorm_statistics_and_apply(n, pixels, C, offset, regime):
    """Statistics against fp64 per statistics unit (mean 2e-6 (|mean| + 1), variance rel-L2 2e-5), apply + SiLU against F.group_norm in
    fp64 per unit; one case with |mean| >> std (tolerance of test_groupnorm_large_common_offset)."""
    from viewcrafter_amd import ops
    need(20)
    x = _t((n, pixels, C), 101, 0.05 if offset else 2.0, offset if offset else 0.5)
    g, b = 1 + _t((C,), 102, 0.2, dtype=torch.float32), _t((C,), 103, 0.1, dtype=torch.float32)
    stats = ops.group_norm_stats(x)
    silu = not offset
    out = ops.group_norm(x, g, b, 1e-5, silu, stats=stats)
    for i in range(n):
        xd = x[i].double().view(pixels, 32, C // 32)
        mean, var = xd.mean(dim=(0, 2)), xd.var(dim=(0, 2), unbiased=False)
        del xd
        assert float((stats[i, :, 0].double() - mean).abs().max()) <= 2e-6 * float(mean.abs().max() + 1), (regime, i)
        assert float((stats[i, :, 1].double() - var).norm() / var.norm()) <= 2e-5, (regime, i)
        ref = F.group_norm(x[i].double().t()[None], 32, g.double(), b.double(), 1e-5)[0].t()
        if silu:
            ref = F.silu(ref)
        check_rows(out[i], lambda a, c: ref[a:c], tol=3e-3 if offset else 2e-3, name=f"groupnorm {regime} unit {i}", chunk=1 << 18)
        del ref


def test_layernorm_and_rowstats_7_videos_1280_lim():
    """vcx_layernorm_f16 / vcx_rowstats_f16 over the 4.13 GB feed-forward hidden state of a 7-video forward, every row against fp64."""
    from viewcrafter_amd import ops
    need(12)
    rows, C = 7 * V, 1280
    x = _t((rows, C), 111, 3.0, 1.0)
    g, b = 1 + _t((C,), 112, 0.2, dtype=torch.float32), _t((C,), 113, 0.1, dtype=torch.float32)
    st = ops.row_stats(x, 1e-5)
    for r0 in range(0, rows, 65536):
        xd = x[r0:r0 + 65536].double()
        mu, var = xd.mean(-1), xd.var(-1, unbiased=False)
        assert float((st[r0:r0 + 65536, 0].double() - mu).abs().max()) <= 1e-5 * float(mu.abs().max() + 1), r0
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        assert float((st[r0:r0 + 65536, 1].double() - rstd).norm() / rstd.norm()) <= 1e-6, r0
    out = ops.layer_norm(x, g, b)
    check_all(out, lambda r0, r1: F.layer_norm(x[r0:r1].double(), (C,), g.double(), b.double(), 1e-5), name="layernorm 7V x 1280", chunk=32768)


# ------------------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("impl,regime", [(0, "2g_pipelined"), (1, "2g_phased")])
def test_flash_spatial_self_attention_of_a_7_video_forward(impl, regime):
    """n_groups = 175 frames, 5 heads, nq = nk = 9216, q | k in one [7 V][960] buffer (3.1 GB, of which q | k are the first 640 columns),
    V^T [320][7 V], base-2 logits: the software-pipelined kernel, and once the phased one (FLASH_IMPL = 1).  Groups 0, the one that
    straddles byte offset 2^31 of the q | k buffer and the last against fp32; every group equal, bit for bit, to the same entry point
    called on its own video (25 groups, offsets below 0.5 GB)."""
    from viewcrafter_amd import ops
    need(10)
    G, heads, n, C, ld = 175, 5, 9216, 320, 960
    qkv = _t((G * n, ld), 121)
    qkv[:, :C] *= 0.125 * ops.LOG2E                     # scale * log2(e) folded into q: Q K^T is the base-2 logit
    vt = _t((C, G * n), 122)
    out = torch.zeros(G * n, C, device=DEV, dtype=torch.float16)
    kw = dict(heads=heads, nq=n, nk=n, kv_rows=n, kv_div=1, ldq=ld, ldk=ld, ldo=C, scale=1.0, log2_logits=True)
    prev = ops.tune_set("FLASH_IMPL", impl)
    try:
        ops.flash_attn(qkv, qkv[:, C:], vt, out, n_groups=G, ldvt=G * n, **kw)
        for v0 in range(0, G, 25):                      # rule (2): one video at a time
            s = slice(v0 * n, (v0 + 25) * n)
            part = torch.zeros(25 * n, C, device=DEV, dtype=torch.float16)
            ops.flash_attn(qkv[s], qkv[s][:, C:], vt[:, s].contiguous(), part, n_groups=25, ldvt=25 * n, **kw)
            assert torch.equal(out[s], part), f"{regime}: video {v0 // 25} differs from its own call"
        torch.cuda.synchronize()
    finally:
        ops.tune_set("FLASH_IMPL", prev)
    g31 = (1 << 31) // (2 * ld * n)
    assert g31 * n * ld * 2 < 1 << 31 < (g31 + 1) * n * ld * 2
    for g in (0, g31, G - 1):
        rows = slice(g * n, (g + 1) * n)
        q = qkv[rows, :C].view(n, heads, 64).permute(1, 0, 2)
        k = qkv[rows, C:2 * C].view(n, heads, 64).permute(1, 0, 2)
        vv = vt[:, rows].reshape(heads, 64, n).permute(0, 2, 1)
        ref = attn_ref(q, k, vv, math.log(2.0)).permute(1, 0, 2).reshape(n, C)
        check_rows(out[rows], lambda a, c: ref[a:c], tol=3e-3, name=f"flash {regime} group {g}")


# ------------------------------------------------------------------------------------------------------------------ element-wise / layout
def test_copy2d_into_a_wide_destination_2g_and_past_lim():
    from viewcrafter_amd import ops
    need(12)
    rows = 7 * V
    src = _t((rows, 320), 131)
    dst = torch.zeros(rows, 960, device=DEV, dtype=torch.float16)
    ops.copy2d(src, dst[:, 320:], rows, 320, 320, 960)
    assert torch.equal(dst[:, 320:640], src) and not bool(dst[:, :320].any()) and not bool(dst[:, 640:].any())
    del dst
    wide = torch.zeros(rows, 1600, device=DEV, dtype=torch.float16)            # rows x ldd = 5.2 GB: past 2^32 bytes
    assert 2 * rows * 1600 > 1 << 32
    ops.copy2d(src, wide[:, 1280:], rows, 320, 320, 1600)
    assert torch.equal(wide[:, 1280:], src) and not bool(wide[:, :1280].any())


def test_casts_and_gelu_past_2g_elements():
    from viewcrafter_amd import ops
    need(20)
    n = (1 << 31) + 4099
    x32 = _t((n,), 141, dtype=torch.float32)
    h = ops.to_f16(x32)
    for i in range(0, n, 1 << 28):
        assert torch.equal(h[i:i + (1 << 28)], x32[i:i + (1 << 28)].half()), i
    del x32
    back = ops.to_f32(h)
    for i in range(0, n, 1 << 28):
        assert torch.equal(back[i:i + (1 << 28)], h[i:i + (1 << 28)].float()), i
    del back
    n = (1 << 31) + 4096
    x = h[:n].clone()
    del h
    # rule (2): every block of 2^27 elements equals the same entry point called on that block alone (offsets below 256 MB), and each
    # block call is checked against the fp32 erf form with the bounds of test_gelu_f16_exact_erf
    y = ops.gelu_(x.clone())
    for i in range(0, n, 1 << 27):
        part = ops.gelu_(x[i:i + (1 << 27)].clone())
        assert torch.equal(y[i:i + (1 << 27)], part), i
        ref = F.gelu(x[i:i + (1 << 27)].float())
        d = part.float() - ref
        assert float(d.abs().max()) <= 2e-3 * max(1.0, float(ref.abs().max())) and float(d.double().norm() / ref.double().norm()) <= 1e-3, i


def test_upsample2x_and_avgpool2x2_past_lim():
    from viewcrafter_amd import ops
    need(12)
    x = _t((25, 288, 512, 256), 151)
    up = ops.upsample2x(x)
    assert up.numel() * 2 > 1 << 32
    for f in range(25):
        assert torch.equal(up[f], x[f].repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)), f
    assert torch.equal(ops.avgpool2x2(up), x)           # the mean of four equal fp16 values is that value


@pytest.mark.parametrize("src_f32", [0, 1])
def test_layout_ncthw_nthwc_past_lim(src_f32):
    """(B, C, T, HW) = (7, 4, 25, 9216), ldc = 2048, c_off = 1000: the channels-last index passes 2^32 bytes (6.6 GB destination)."""
    from viewcrafter_amd import ops
    need(16)
    B, C, T, HW, ldc, c_off = 7, 4, 25, 9216, 2048, 1000
    src = _t((B, C, T, 72, 128), 161, dtype=torch.float32)
    want = src.half().permute(0, 2, 3, 4, 1)            # [B, T, H, W, C]
    if not src_f32:
        dst = torch.zeros(B, T, 72, 128, ldc, device=DEV, dtype=torch.float16)
        assert dst.numel() * 2 > 1 << 32
        ops.ncthw_to_nthwc(src, dst, c_off=c_off)
        assert torch.equal(dst[..., c_off:c_off + C], want)
        assert not bool(dst[..., :c_off].any()) and not bool(dst[..., c_off + C:].any())
        lead = torch.zeros(B, T, 72, 128, ldc, device=DEV, dtype=torch.float16)
        del dst
        lead[..., :C] = want
        assert torch.equal(ops.nthwc_to_ncthw(lead, C=C), src.half().float())
    else:
        lead = torch.zeros(B, T, 72, 128, ldc // 2, device=DEV, dtype=torch.float32)      # fp32 source: 1024 columns x 4 bytes, the same 6.6 GB
        assert lead.numel() * 4 > 1 << 32
        lead[..., :C] = src.permute(0, 2, 3, 4, 1)
        assert torch.equal(ops.nthwc_to_ncthw(lead, C=C), src)


# ------------------------------------------------------------------------------------------------------------------ more of the 7-video forward
def test_conv_unet_level0_7_videos_k_tail_2g():
    """The folded skip convolution of an up-path ResBlock in a 7-video forward: 3x3 over 960 channels (3.1 GB image) + a K tail of
    640 + 320 columns read row for row from two linear sources (2.06 GB and 1.03 GB); per frame against F.conv2d + the 1x1 in fp32."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv
    need(12)
    n, H, W, cin, cout, tails = 175, 72, 128, 960, 320, (640, 320)
    M = n * H * W
    a = _t((n, H, W, cin), 171)
    w3 = _t((cout, cin, 3, 3), 172, 1 / math.sqrt(9 * cin))
    srcs = [_t((M, k), 173 + j) for j, k in enumerate(tails)]
    w1 = _t((cout, sum(tails)), 176, 1 / math.sqrt(sum(tails)))
    b = _t((cout,), 177, 0.1, dtype=torch.float32)
    assert 2 * M * cin > 1 << 31 and ops.conv_tail_ok(M, cin, cout, 9, list(tails))
    wcat = torch.cat([pack_conv(w3), w1], dim=1).contiguous()
    guard = torch.full((M + 64, cout), 7.0, device=DEV, dtype=torch.float16)
    y = ops.conv2d(a, wcat, b, kh=3, kw=3, tail=srcs, out=guard[:M]).reshape(n, H * W, cout)
    assert bool((guard[M:] == 7.0).all())
    for f in range(n):
        r = slice(f * H * W, (f + 1) * H * W)
        ref = conv_frame_ref(a[f], w3, b) + torch.cat([s_[r].float() for s_ in srcs], dim=1) @ w1.float().t()
        check_rows(y[f], lambda p, q: ref[p:q], name=f"conv 960->320 + K tail, frame {f}", chunk=H * W)


def test_groupnorm_over_a_split_concat_7_videos_2g():
    """vcx_groupnorm_apply2_f16 at (175, 9216, 640 + 320): 3.1 GB out, the halves read in place; every frame against F.group_norm in
    fp64 of the concatenated frame, and the same bits as the norm of the materialised concat."""
    from viewcrafter_amd import ops
    need(14)
    n, pix, c1, c2 = 175, 9216, 640, 320
    C = c1 + c2
    x1, x2 = _t((n, pix, c1), 181, 2.0, 0.3), _t((n, pix, c2), 182, 0.5, -1.0)
    g, b = 1 + _t((C,), 183, 0.2, dtype=torch.float32), _t((C,), 184, 0.1, dtype=torch.float32)
    xc = torch.cat([x1, x2], dim=2)
    st = ops.group_norm_stats(xc)
    guard = torch.full((n * pix + 8, C), 7.0, device=DEV, dtype=torch.float16)
    got = ops.group_norm(x1, g, b, 1e-5, True, stats=st, x2=x2, out=guard[:n * pix].view(n, pix, C))
    assert 2 * n * pix * C > 1 << 31 and bool((guard[n * pix:] == 7.0).all())
    assert torch.equal(got, ops.group_norm(xc, g, b, 1e-5, True, stats=st))
    for i in range(n):
        ref = F.silu(F.group_norm(xc[i].double().t()[None], 32, g.double(), b.double(), 1e-5))[0].t()
        check_rows(got[i], lambda p, q: ref[p:q], name=f"groupnorm over a split concat, frame {i}")


def test_flash_dual_cross_attention_of_a_7_video_forward_2g():
    """vcx_attn_flash_dual_d64_f16 with the Q / O buffers of the 7-video forward (q in the [7 V][960] buffer, 3.1 GB) and one text (+)
    image key set per video (kv_div = 25): every group against fp32."""
    from viewcrafter_amd import ops
    need(8)
    G, heads, n, C, ld, nk1, kr1, nk2 = 175, 5, 9216, 320, 960, 77, 80, 256
    q = _t((G * n, ld), 191)
    k1, v1 = _t((7 * kr1, C), 192), _t((7 * kr1, C), 193)
    k2, v2 = _t((7 * nk2, C), 194), _t((7 * nk2, C), 195)
    out = torch.zeros(G * n, C, device=DEV, dtype=torch.float16)
    ops.flash_attn_dual(q, k1, v1.t().contiguous(), k2, v2.t().contiguous(), out, n_groups=G, heads=heads, nq=n, nk1=nk1, kv_rows1=kr1, kv_div1=25,
                        ldk1=C, ldvt1=7 * kr1, nk2=nk2, kv_rows2=nk2, kv_div2=25, ldk2=C, ldvt2=7 * nk2, ldq=ld, ldo=C, scale=0.125)
    hd = lambda t: t.view(-1, heads, 64).permute(1, 0, 2)
    for g in range(G):
        rows, v = slice(g * n, (g + 1) * n), g // 25
        qq = hd(q[rows, :C])
        ref = attn_ref(qq, hd(k1[v * kr1:v * kr1 + nk1]), hd(v1[v * kr1:v * kr1 + nk1]), 0.125) + attn_ref(qq, hd(k2[v * nk2:(v + 1) * nk2]), hd(v2[v * nk2:(v + 1) * nk2]), 0.125)
        ref = ref.permute(1, 0, 2).reshape(n, C)
        check_rows(out[rows], lambda p, r: ref[p:r], tol=3e-3, name=f"dual flash group {g}")


def test_temporal_attention_of_a_7_video_forward_2g():
    """Temporal attention B = 7, T = 25, P = 9216, 5 heads on the [7 V][960] q | k | v buffer (3.1 GB); every pixel against fp32."""
    from viewcrafter_amd import ops
    need(8)
    B, T, P, heads, C, ld = 7, 25, 9216, 5, 320, 960
    qkv = _t((B * T * P, ld), 201)
    out = torch.zeros(B * T * P, C, device=DEV, dtype=torch.float16)
    ops.temporal_attn(qkv, out, B=B, T=T, P=P, heads=heads, ld=ld, k_off=C, v_off=2 * C, ldo=C, scale=0.125)
    x5, o4 = qkv.view(B, T, P, 3, heads, 64), out.view(B, T, P, C)
    for bi in range(B):
        for p0 in range(0, P, 1024):
            blk = x5[bi, :, p0:p0 + 1024].permute(2, 1, 3, 0, 4).reshape(3, -1, T, 64)          # [q|k|v][(pixel, head)][T][64]
            ref = attn_ref(blk[0], blk[1], blk[2], 0.125).view(1024, heads, T, 64).permute(2, 0, 1, 3).reshape(T * 1024, C)
            check_rows(o4[bi, :, p0:p0 + 1024].reshape(T * 1024, C), lambda p, r: ref[p:r], tol=3e-3, name=f"temporal attention video {bi} pixels {p0}...")
