"""A sample's bits do not depend on the batch it runs in - checked where the promise can break: at full width.

The tiny UNet of test_model_gpu.py never reaches a batch-dependent decision of the host graph or of the GEMM dispatcher - they are keyed
to the C = 320 level and to row counts of thousands.  Here every comparison straddles such a decision:

  * kernel level: a call over 2 m rows against a call over its first m rows, with m chosen so that the dispatcher's choice changes
    between the two (tile configuration and large-tile / small-tail split of the tiled engine, the weight-stationary kernel from
    M = 8192 on, vcx_gemm_units_f16 with one unit against two) - output, column moments and row statistics compared with torch.equal;
  * module level: the level-0 ResBlock / SpatialTransformer / TemporalTransformer (C = 320) and one C = 640 transformer of the real
    512 model, B = 2 against two B = 1 calls and the shared CFG prefix (cfg_repeat 2 / 3) against the replicated input, at latents on
    both sides of the 8192-row and 16 MiB thresholds; the temporal block also against its fp32 oracle;
  * model level: the 1.44 B UNet at config 1's 16 x 40 x 64, at T = 3 and T = 6, and once at 25 x 72 x 128, plus the sampler's own
    two guidance routes (DDIMSampler._apply_batched with share_cfg_prefix on and off).

tests/test_host_logic.py::test_batch_routes_* checks the same rule on the host side without a GPU.
"""
import math

import pytest
import torch

from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rnd(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale + offset


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tiled_route(M, N):
    """The tile rule of csrc/gemm.hip (tiled engine, no GEGLU): (configuration, first row of the small-tile tail or None)."""
    cfg = 1 if N % 160 == 0 else 0
    big_bn = 320 if N % 320 == 0 else (256 if (N % 256 == 0 or N >= 1024) else 0)
    if big_bn and ((M + 255) // 256) * ((N + big_bn - 1) // big_bn) >= 384:
        cfg = 3 if big_bn == 320 else 2
    if cfg < 2:
        return cfg, None
    tbn = 256 if cfg == 2 else 320
    tiles_m, tiles_n = (M + 255) // 256, (N + tbn - 1) // tbn
    full, rem = divmod(tiles_m * tiles_n, _cus())
    if full >= 1 and rem > 0 and rem * 10 < _cus() * 7:
        m1 = (full * _cus() // tiles_n) * 256
        if 0 < m1 < M:
            return cfg, m1
    return cfg, None


def _strip_moments_ok(cs, y):
    """(mean, M2) per 64-row strip and column against fp64 moments of the stored fp16 output (the neighbouring tests' tolerance)."""
    M, N = y.shape
    yd = y.double().view(M // 64, 64, N)
    mean = yd.mean(1)
    m2 = ((yd - mean.unsqueeze(1)) ** 2).sum(1)
    assert float((cs[..., 0].double() - mean).abs().max()) <= 2e-6 * (float(yd.abs().max()) + 1.0)
    assert rel_l2(cs[..., 1], m2) <= 2e-5


# ------------------------------------------------------------------------------------------------------------------ A: kernel level
@pytest.mark.parametrize("kind,N,K,m", [
    ("linear", 320, 640, 64 * 1500),      # 375 tiles of 256 x 320 (128 x 160 tiles) | 750 (256 x 320, no tail)
    ("linear", 320, 640, 230400),         # one video of 25 x 72 x 128: 900 tiles with a small-tile tail | 1800 tiles, another split row
    ("linear", 640, 640, 57600),          # 450 tiles (256 x 320, no tail) | 900 (256 x 320 + small-tile tail)
    ("linear", 1280, 640, 14400),         # 57 x 4 = 228 tiles (128 x 160) | 452 (256 x 320 + tail)
    ("conv", 320, 320, 2560 * 38),        # 3 x 3 convolution over 38 frames of 40 x 64, K = 2880: 380 tiles | 760
    ("conv_tail", 320, 320, 230400),      # ... with the skip convolution as a K tail (K = 2880 + 320): the ResBlock's second convolution
])
def test_tiled_engine_rows_do_not_depend_on_the_call_size(kind, N, K, m):
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv
    M = 2 * m
    routes = (_tiled_route(m, N), _tiled_route(M, N))
    if kind == "linear":
        x = _rnd((M, K), 11).half()
        w = (_rnd((N, K), 12) / math.sqrt(K)).half()
        b = _rnd((N,), 13, 0.1)

        def run(rows):
            cs = ops.colstats_buffer(rows, N, DEV)
            return ops.linear(x[:rows], w, b, colstats=cs), cs
    else:
        Hh, Ww = (40, 64) if m % 9216 else (72, 128)
        frames = M // (Hh * Ww)
        x = _rnd((frames, Hh, Ww, K), 21).half()
        w = pack_conv(_rnd((N, K, 3, 3), 22).cpu() / math.sqrt(9 * K)).to(DEV).half()
        b = _rnd((N,), 23, 0.1)
        tail = None
        if kind == "conv_tail":
            tail = _rnd((M, 320), 24).half()
            w = torch.cat([w, (_rnd((N, 320), 25) / math.sqrt(320)).half()], dim=1).contiguous()

        def run(rows):
            cs = ops.colstats_buffer(rows, N, DEV)
            kw = {} if tail is None else dict(tail=[tail[:rows]])
            y = ops.conv2d(x[:rows // (Hh * Ww)], w, b, kh=3, kw=3, colstats=cs, **kw)
            return y.reshape(rows, N), cs
    y2, cs2 = run(M)
    y1, cs1 = run(m)
    torch.cuda.synchronize()
    print(f"{kind} N={N} K={K}: route at {m} rows {routes[0]}, at {M} rows {routes[1]}")
    assert routes[0] != routes[1], "the pair must straddle a decision of the tile rule"
    _strip_moments_ok(cs1, y1)
    assert torch.equal(y1, y2[:m]), f"{int((y1 != y2[:m]).sum())} output elements depend on the call size"
    assert torch.equal(cs1, cs2[:m // 64]), f"{int((cs1 != cs2[:m // 64]).sum())} column moments depend on the call size"


@pytest.mark.parametrize("M,N,K", [(64 * 1500, 320, 640), (28800, 1280, 640), (4096, 320, 320), (9216 * 2, 640, 640)])
def test_column_moments_are_the_same_bits_in_every_tile_configuration(M, N, K):
    """The tile configuration that computes a 64-row strip depends on the total M (threshold and tail split above): its column moments
    must not.  Forced GEMM_CFG -1 ... 3 against each other with torch.equal, and against fp64 moments of the stored output."""
    from viewcrafter_amd import ops
    x = _rnd((M, K), 31).half()
    w = (_rnd((N, K), 32) / math.sqrt(K)).half()
    b = _rnd((N,), 33, 0.1, 2.0)
    res = _rnd((M, N), 34, 0.5).half()
    got = {}
    try:
        for cfg in (-1, 0, 1, 2, 3):
            ops.tune_set("GEMM_CFG", cfg)
            cs = ops.colstats_buffer(M, N, DEV)
            got[cfg] = (ops.linear(x, w, b, residual=res, colstats=cs), cs)
            torch.cuda.synchronize()
    finally:
        ops.tune_set("GEMM_CFG", -1)
    _strip_moments_ok(got[-1][1], got[-1][0])
    for cfg in (0, 1, 2, 3):
        assert torch.equal(got[cfg][0], got[-1][0]), cfg
        assert torch.equal(got[cfg][1], got[-1][1]), f"GEMM_CFG {cfg}: {int((got[cfg][1] != got[-1][1]).sum())} column moments differ"


@pytest.mark.parametrize("m,variant", [(6144, "plain"), (6144, "colstats"), (4096 + 64, "bias+res"), (8192, "rowstats"), (9216, "rowstats+res")])
def test_weight_stationary_320_rows_do_not_depend_on_the_call_size(m, variant):
    """N = K = 320 linear layers: from M = 8192 on the weight-stationary kernel, below it the tiled engine.  A call over 2 m rows against
    a call over its first m rows - across the threshold (m < 8192: output and column moments) and above it (row statistics)."""
    from viewcrafter_amd import ops
    N = K = 320
    M = 2 * m
    x = _rnd((M, K), 41).half()
    w = (_rnd((N, K), 42) / math.sqrt(K)).half()
    b = _rnd((N,), 43, 0.3) if variant != "plain" else None
    res = _rnd((M, N), 44, 0.7).half() if "res" in variant else None

    def run(rows):
        kw = dict(residual=None if res is None else res[:rows])
        cs = st = None
        if variant == "colstats":
            cs = kw["colstats"] = ops.colstats_buffer(rows, N, DEV)
        if variant.startswith("rowstats"):
            assert ops.rowstats_ok(rows, N, K, ldr=N if res is not None else 0)
            st = kw["rowstats"] = ops.rowstats_buffer(rows, DEV)
        return ops.linear(x[:rows], w, b, **kw), cs, st
    y2, cs2, st2 = run(M)
    y1, cs1, st1 = run(m)
    torch.cuda.synchronize()
    ref = x[:m].float() @ w.float().t() + (b if b is not None else 0) + (res[:m].float() if res is not None else 0)
    assert rel_l2(y1, ref) <= 2e-3
    assert torch.equal(y1, y2[:m]), f"{int((y1 != y2[:m]).sum())} output elements depend on the call size"
    if cs1 is not None:
        _strip_moments_ok(cs1, y1)
        assert torch.equal(cs1, cs2[:m // 64])
    if st1 is not None:
        ln = ops.row_stats(y1, 1e-5)
        assert float((st1[:, 0] - ln[:, 0]).abs().max()) <= 2e-6 * (float(y1.float().abs().max()) + 1.0)
        assert torch.equal(st1, st2[:m]), f"{int((st1 != st2[:m]).sum())} row statistics depend on the call size"


@pytest.mark.parametrize("unit_rows,rowstats", [(9216, True), (9216, False), (25 * 2560, True), (4096, False), (2560 * 3, False)])
def test_gemm_units_one_unit_is_the_same_route_as_two(unit_rows, rowstats):
    """vcx_gemm_units_f16 with one unit (a single video: the folded GroupNorm of proj_in at B = 1) against two (B = 2): the first unit's
    output and row statistics are the same bits.  Row statistics exist where rowstats_ok says so for ONE video - then for any batch."""
    from viewcrafter_amd import ops
    C = N = 320
    x = _rnd((2 * unit_rows, C), 51).half()
    wn = (_rnd((2, N, C), 52) / math.sqrt(C)).half()
    bn = _rnd((2, N), 53) + torch.tensor([[0.0], [3.0]], device=DEV)
    assert ops.rowstats_ok(unit_rows, N, C, unit_rows=unit_rows) == ops.rowstats_ok(2 * unit_rows, N, C, unit_rows=unit_rows, video_rows=unit_rows)
    if rowstats:
        assert ops.rowstats_ok(unit_rows, N, C, unit_rows=unit_rows)
    outs = {}
    for units in (1, 2):
        rows = units * unit_rows
        st = ops.rowstats_buffer(rows, DEV) if rowstats else None
        outs[units] = (ops.gemm_units(x[:rows], wn[:units].contiguous(), bn[:units].contiguous(), unit_rows=unit_rows, rowstats=st), st)
    torch.cuda.synchronize()
    y1, st1 = outs[1]
    assert rel_l2(y1, x[:unit_rows].float() @ wn[0].float().t() + bn[0]) <= 2e-3
    assert torch.equal(y1, outs[2][0][:unit_rows]), "unit 0 depends on the number of units"
    if rowstats:
        ln = ops.row_stats(y1, 1e-5)
        assert float((st1[:, 0] - ln[:, 0]).abs().max()) <= 2e-6 * (float(y1.float().abs().max()) + 1.0)
        assert float(((st1[:, 1] - ln[:, 1]).abs() / ln[:, 1]).max()) <= 6e-5
        assert torch.equal(st1, outs[2][1][:unit_rows]), "unit 0's row statistics depend on the number of units"


# ------------------------------------------------------------------------------------------------------------------ B: module level
def _unet512():
    from tests.test_fullconfig_gpu import _model
    model, params = _model("inference_pvd_512.yaml")
    return model, model.model.diffusion_model


def _txt_kv(st, B, seed, r=1):
    """Context K / V of r * B videos (text tokens only, zero-padded to 80 rows per video) for a SpatialTransformer."""
    ctx = torch.zeros(r * B * 80, 1024, device=DEV, dtype=torch.float16)
    ctx.view(r * B, 80, 1024)[:, :77] = _rnd((r * B, 77, 1024), seed).half()
    return st.project_context(dict(txt=ctx, img=None, n_img=0, per_frame=False)), ctx


# (T, h, w) on both sides of the thresholds: at 40 x 64 (2560 pixels) 3 frames are 7680 rows (< 8192) alone and 15360 in a pair; 6 frames
# are 9.8 MB alone and 19.7 MB in a pair (16 MiB spatial fold); 16 frames are config 1's latent (fold and epilogue statistics on)
GRID = [(3, 40, 64), (6, 40, 64), (16, 40, 64)]


@pytest.mark.parametrize("T,h,w", GRID)
def test_level0_blocks_batch_of_two_equals_two_batches_of_one(T, h, w):
    _, unet = _unet512()
    rb, st, tt = list(unet.input_blocks[1])
    C = 320
    P = h * w
    x = _rnd((2 * T, h, w, C), 61 + T).half()
    emb = _rnd((2, rb.emb_channels), 62).half()
    kv2, ctx2 = _txt_kv(st, 2, 63)
    with torch.no_grad():
        r2, _ = rb(x, emb, batch_size=2)
        r1 = torch.cat([rb(x[i * T:(i + 1) * T].contiguous(), emb[i:i + 1].contiguous(), batch_size=1)[0] for i in range(2)])
        s2, _ = st(x, context_kv=kv2, frames_per_video=T)
        s1 = torch.cat([st(x[i * T:(i + 1) * T].contiguous(), frames_per_video=T,
                           context_kv=st.project_context(dict(txt=ctx2[i * 80:(i + 1) * 80].contiguous(), img=None, n_img=0, per_frame=False)))[0]
                        for i in range(2)])
        t2, _ = tt(x.view(2, T, P, C))
        t1 = torch.cat([tt(x[i * T:(i + 1) * T].reshape(1, T, P, C))[0] for i in range(2)])
    torch.cuda.synchronize()
    assert torch.equal(r1, r2), f"ResBlock: {int((r1 != r2).sum())} elements differ"
    assert torch.equal(s1, s2), f"SpatialTransformer: {int((s1 != s2).sum())} elements differ"
    assert torch.equal(t1.view_as(t2), t2), f"TemporalTransformer: {int((t1.view_as(t2) != t2).sum())} elements differ"


@pytest.mark.parametrize("T,h,w,r", [(3, 40, 64, 2), (6, 40, 64, 2), (6, 40, 64, 3), (16, 40, 64, 2)])
def test_spatial_transformer_shared_prefix_equals_the_replicated_input(T, h, w, r):
    _, unet = _unet512()
    st = unet.input_blocks[1][1]
    x = _rnd((T, h, w, 320), 71 + T).half()
    kv, _ = _txt_kv(st, 1, 72, r=r)
    with torch.no_grad():
        shared, _ = st(x, context_kv=kv, frames_per_video=T, cfg_repeat=r)
        full, _ = st(torch.cat([x] * r), context_kv=kv, frames_per_video=T)
    torch.cuda.synchronize()
    assert torch.equal(shared, full), f"{int((shared != full).sum())} elements differ"
    assert not torch.equal(full[:T], full[T:2 * T])


@pytest.mark.parametrize("T,h,w", [(3, 40, 64), (16, 40, 64)])
def test_temporal_transformers_vs_fp32_oracle_and_batch(T, h, w):
    """C = 320 (input block 1) and C = 640 (input block 4: the LayerNorm -> GEGLU fold is on from 640): against the fp32 oracle (on the
    residual branch, the part the block computes) and B = 2 against two B = 1 calls."""
    from oracle import lvdm_oracle as O
    _, unet = _unet512()
    for blk_i, C, hh, ww in ((1, 320, h, w), (4, 640, h // 2, w // 2)):
        tt = unet.input_blocks[blk_i][2]
        P = hh * ww
        with torch.no_grad():
            x = _rnd((2, T, P, C), 83 + T).half()
            y2, _ = tt(x)
            y1 = torch.cat([tt(x[i:i + 1].contiguous())[0] for i in range(2)])
            prefix = f"input_blocks.{blk_i}.2"
            sd = {k: v.float() for k, v in unet.state_dict().items() if k.startswith(prefix + ".")}
            xr = x.float().view(2, T, hh, ww, C).permute(0, 4, 1, 2, 3).contiguous()
            ref = O.temporal_transformer(sd, prefix, xr, tt.n_heads).permute(0, 2, 3, 4, 1).reshape(2, T, P, C)
        e = rel_l2(y2.float() - x.float(), ref - x.float())
        print(f"TemporalTransformer C={C} T={T} {hh}x{ww}: rel-L2 of the residual branch vs fp32 oracle = {e:.3e}")
        assert e <= 6e-3
        assert torch.equal(y1, y2), f"C={C}: {int((y1 != y2).sum())} elements differ between B = 2 and two B = 1"


# ------------------------------------------------------------------------------------------------------------------ C: model level
def _three_way(unet, T, h, w, seed):
    from tests.test_fullconfig_gpu import _inputs
    x, ctx = _inputs(T, h, w, seed=seed, B=2)
    x1 = x[:1].contiguous()
    ts, fs = torch.tensor([599, 599], device=DEV), torch.tensor([10, 10], device=DEV)
    with torch.no_grad():
        x2 = torch.cat([x1, x1])
        plain = unet._forward(x2, ts, context=ctx, fs=fs)
        ones = torch.cat([unet._forward(x1, ts[:1], context=ctx[i:i + 1].contiguous(), fs=fs[:1]) for i in range(2)])
        shared = unet._forward(x1, ts[:1], context=ctx, fs=fs[:1], cfg_repeat=2)
    torch.cuda.synchronize()
    assert torch.isfinite(plain).all() and not torch.equal(plain[0], plain[1])
    assert torch.equal(ones, plain), f"B = 2 differs from two B = 1 forwards in {int((ones != plain).sum())} elements"
    assert torch.equal(shared, plain), f"the shared CFG prefix differs from the plain batch in {int((shared != plain).sum())} elements"


@pytest.mark.parametrize("T", [3, 6, 16])
def test_unet512_batch_and_shared_prefix_are_bit_identical(T):
    _, unet = _unet512()
    _three_way(unet, T, 40, 64, seed=500 + T)


def test_unet1024_batch_and_shared_prefix_are_bit_identical_at_25x72x128():
    from tests.test_fullconfig_gpu import _model
    model, _ = _model("inference_pvd_1024.yaml")
    _three_way(model.model.diffusion_model, 25, 72, 128, seed=525)
    torch.cuda.empty_cache()


def test_sampler_guidance_routes_agree_at_a_threshold_latent():
    """DDIMSampler._apply_batched with the shared prefix and as a plain batch (ddim.py): the same denoiser outputs, at T = 3, 40 x 64."""
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    model, _ = _unet512()
    T, h, w = 3, 40, 64
    s = DDIMSampler(model)
    cat = _rnd((1, 4, T, h, w), 91)
    c = {"c_crossattn": [_rnd((1, 77 + 256, 1024), 92)], "c_concat": [cat]}
    uc = {"c_crossattn": [_rnd((1, 77 + 256, 1024), 93)], "c_concat": [cat]}
    x, t, fs = _rnd((1, 4, T, h, w), 94), torch.tensor([500], device=DEV), torch.tensor([10], device=DEV)
    outs = []
    with torch.no_grad():
        for share in (True, False):
            s.share_cfg_prefix, s._cfg_cache = share, None
            assert s._shares_prefix((c, uc)) == share
            outs.append([o.clone() for o in s._apply_batched(x, t, (c, uc), {"fs": fs})])
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(*outs)), "the two guidance routes of the sampler differ"
