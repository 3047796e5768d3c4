"""The spatial self-attention over 2x2-pooled keys and values (VCX_SATTN_KV_POOL) on the MI355X: vcx_layernorm_pool2x2_f16 against the
composition it is defined as, byte for byte; its refusals; one tensor past 4 GiB; the flash kernels with four times as many queries as
keys; SpatialTransformer and the tiny UNet against the fp32 reference tests/kv_pool_ref.py; and the bit-identities the route must keep
(shared CFG prefix, batch rows, graph replay, a shallow forward of the feature cache, VCX_SATTN_MXFP8 beside it)."""
import pytest
import torch

from oracle.weights import synth_input
from tests import kv_pool_ref as REF
from tests.test_kernels_gpu import LN2, _log2_q, attn_ref, check, rnd
from tests.test_sattn_kv_pool_cpu import C as ST_C, _on, transformer_inputs
from tests.tiny_config import TINY_UNET
from tests.util import load_synth, rel_l2
from viewcrafter_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
UNET_TOL = 5e-3          # tests/test_model_gpu.py: the un-pooled module on the kernels against the fp32 oracle; the same arithmetic chain
EINVAL = -1
GUARD = 64               # canary halfs on either side of y (128 bytes: y stays 16-byte aligned)
CANARY = 0x7A5C          # an fp16 bit pattern no LayerNorm of these inputs produces in a whole guard


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
def _ln_inputs(n, H, W, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n * H * W, Cc), generator=g) * 1.7 + 0.2
    rows = torch.arange(n * H * W)
    hard = rows % 3 == 1          # rows of large mean and small spread: in every window of two or more columns
    x[hard] = 180.0 + 0.06 * torch.randn((int(hard.sum()), Cc), generator=g)
    gamma, beta = 1.0 + 0.3 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g)
    return x.half().to(DEV), gamma.to(DEV), beta.to(DEV)


def _launch(x, gamma, beta, n, H, W, mode, eps=1e-5, y_off=GUARD):
    """vcx_layernorm_pool2x2_f16 into the middle of a canary-filled buffer -> (rc, the buffer as int16, rows, C)"""
    from viewcrafter_amd import ops
    Cc = x.shape[1]
    rows = n * (H // 2) * (W // 2)
    buf = torch.full((2 * GUARD + rows * Cc,), CANARY, dtype=torch.int16, device=DEV)
    rc = _lib.lib().vcx_layernorm_pool2x2_f16(x.data_ptr(), buf.data_ptr() + 2 * y_off, gamma.data_ptr(), beta.data_ptr(), n, H, W, Cc, eps, mode, ops._stream())
    torch.cuda.synchronize()
    return rc, buf, rows, Cc


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,H,W", [(1, 2, 2), (3, 4, 6), (2, 8, 12), (1, 16, 16)])
@pytest.mark.parametrize("Cc", [64, 320, 640, 1280])          # one width per lane geometry of the LayerNorm kernels the model uses
def test_kernel_is_the_composition_byte_for_byte(Cc, n, H, W, mode):
    from viewcrafter_amd import ops
    x, gamma, beta = _ln_inputs(n, H, W, Cc, 1000 + Cc + H)
    a = ops.layer_norm(x, gamma, beta, 1e-5)
    want = ops.avgpool2x2(a.view(n, H, W, Cc)).reshape(-1, Cc) if mode == ops.POOL_MEAN else a.view(n, H, W, Cc)[:, ::2, ::2].reshape(-1, Cc).contiguous()
    rc, buf, rows, _ = _launch(x, gamma, beta, n, H, W, mode)
    assert rc == 0, _lib.lib().vcx_last_error()
    y = buf[GUARD:GUARD + rows * Cc].view(torch.float16).view(rows, Cc)
    assert torch.isfinite(y).all() and float(y.float().abs().max()) > 0.5
    bad = int((y.view(torch.int16) != want.view(torch.int16)).sum())
    assert bad == 0, f"{bad} of {y.numel()} values differ from the composition (max abs {float((y.float() - want.float()).abs().max()):.3e})"
    assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + rows * Cc:] == CANARY).all()), "canary bytes around y were written"
    assert torch.equal(ops.layer_norm_pool2x2(x, gamma, beta, 1e-5, n, H, W, mode), y), "the ops entry is the same launch"
    if mode == ops.POOL_NEAREST:
        # the three other rows of every window hold NaN: a kernel that read and used them would show it
        xp = torch.full_like(x, float("nan")).view(n, H, W, Cc)
        xp[:, ::2, ::2] = x.view(n, H, W, Cc)[:, ::2, ::2]
        assert torch.equal(ops.layer_norm_pool2x2(xp.view(-1, Cc), gamma, beta, 1e-5, n, H, W, mode), y)


def test_refusals_return_einval_and_write_nothing():
    from viewcrafter_amd import ops
    L = _lib.lib()
    x, gamma, beta = _ln_inputs(2, 6, 6, 64, 7)          # 72 rows: enough for every geometry the launcher is told below
    x72 = torch.zeros((72, 72), dtype=torch.float16, device=DEV)
    x8200 = torch.zeros((4, 8200), dtype=torch.float16, device=DEV)
    wide = torch.ones(8200 + 8, device=DEV)
    ok = dict(x=x.data_ptr(), y_off=GUARD, g=gamma.data_ptr(), b=beta.data_ptr(), n=2, H=4, W=6, Cc=64, mode=0)
    cases = [("odd H", dict(H=5)), ("odd W", dict(W=5)), ("C % 8", dict(x=x72.data_ptr(), g=wide.data_ptr(), b=wide.data_ptr(), Cc=68)),
             ("C > 8192", dict(x=x8200.data_ptr(), g=wide.data_ptr(), b=wide.data_ptr(), n=1, H=2, W=2, Cc=8200)), ("mode 2", dict(mode=2)),
             ("mode -1", dict(mode=-1)), ("n H W = 2^31", dict(n=1 << 17, H=128, W=128)), ("y not aligned", dict(y_off=GUARD + 4)),
             ("x not aligned", dict(x=x.data_ptr() + 8)), ("gamma not aligned", dict(g=wide.data_ptr() + 8)), ("beta not aligned", dict(b=wide.data_ptr() + 8)),
             ("null x", dict(x=None)), ("null gamma", dict(g=None))]
    for name, kw in cases:
        a = dict(ok, **kw)
        buf = torch.full((2 * GUARD + 16384,), CANARY, dtype=torch.int16, device=DEV)
        rc = L.vcx_layernorm_pool2x2_f16(a["x"], buf.data_ptr() + 2 * a["y_off"], a["g"], a["b"], a["n"], a["H"], a["W"], a["Cc"], 1e-5, a["mode"], ops._stream())
        torch.cuda.synchronize()
        assert rc == EINVAL and b"vcx_layernorm_pool2x2_f16" in L.vcx_last_error(), (name, rc, L.vcx_last_error())
        assert bool((buf == CANARY).all()), f"{name}: refused, yet something was written"
    # ... and the accepted call between them writes exactly its rows
    rc, buf, rows, Cc = _launch(x[:48], gamma, beta, 2, 4, 6, 0)
    assert rc == 0 and rows == 12 and not bool((buf[GUARD:GUARD + rows * Cc] == CANARY).all())


def test_x_past_4_gib_first_and_last_window_rows():
    """33 frames of 1024 x 1024 tokens of 64 channels: x is 4.13 GiB and its last frame starts at byte 2^32 exactly.  The first and the last
    row of windows are compared with the composition run on those two pairs of source rows alone (tests/test_large_extent_gpu.py's way)."""
    from viewcrafter_amd import ops
    n, H, W, Cc = 33, 1024, 1024, 64
    free, total = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip(f"needs 8 GiB of device memory, {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB free")
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.empty((n * H * W, Cc), dtype=torch.float16, device=DEV)
    flat = x.view(-1)
    for i in range(0, flat.numel(), 1 << 28):
        flat[i:i + (1 << 28)].normal_(0.3, 1.5, generator=g)
    assert x.numel() * 2 > 1 << 32 and (n - 1) * H * W * Cc * 2 == 1 << 32
    gamma, beta = _ln_inputs(1, 2, 2, Cc, 3)[1:]
    for mode in (ops.POOL_MEAN, ops.POOL_NEAREST):
        y = ops.layer_norm_pool2x2(x, gamma, beta, 1e-5, n, H, W, mode).view(n, H // 2, W // 2, Cc)
        for name, rows, got in (("first", x[:2 * W], y[0, 0]), ("last", x[-2 * W:], y[-1, -1])):
            a = ops.layer_norm(rows.contiguous(), gamma, beta, 1e-5).view(1, 2, W, Cc)
            want = ops.avgpool2x2(a)[0, 0] if mode == ops.POOL_MEAN else a[0, 0, ::2]
            assert torch.equal(got, want), f"mode {mode}, {name} window row: {int((got != want).sum())} values differ"
        del y
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 2. four queries per key
@pytest.mark.parametrize("impl,nq,nk", [(1, 256, 64), (2, 256, 64), (0, 96, 24)])          # the phased and the pipelined kernel; a ragged key tile
def test_flash_attn_with_four_times_as_many_queries_as_keys(impl, nq, nk):
    from viewcrafter_amd import ops
    G, heads = 3, 2
    Cc = heads * 64
    q = _log2_q(rnd(G * nq, Cc, seed=270)).to(DEV)
    k = rnd(G * nk, Cc, seed=271).to(DEV).half()
    v = rnd(G * nk, Cc, seed=272).to(DEV).half()
    out = torch.full((G * nq, Cc), float("nan"), device=DEV, dtype=torch.float16)
    prev = ops.tune_set("FLASH_IMPL", impl)
    try:
        ops.flash_attn(q, k, v.t().contiguous(), out, n_groups=G, heads=heads, nq=nq, nk=nk, kv_rows=nk, kv_div=1, ldq=Cc, ldk=Cc, ldvt=G * nk, ldo=Cc,
                       scale=0.0, log2_logits=True)
        torch.cuda.synchronize()
    finally:
        ops.tune_set("FLASH_IMPL", prev)

    def split(t, rows):
        return t.view(G, rows, heads, 64).permute(0, 2, 1, 3).reshape(G * heads, rows, 64)
    ref = attn_ref(split(q, nq), split(k, nk), split(v, nk), LN2).view(G, heads, nq, 64).permute(0, 2, 1, 3).reshape(G * nq, Cc)
    check(out, ref, tol=3e-3, name=f"flash nq {nq} nk {nk} impl {impl}")          # tests/test_kernels_gpu.py's tolerance for this kernel


# ------------------------------------------------------------------------------------------------------------------ 3. SpatialTransformer
CDIM = 128


@pytest.fixture(scope="module")
def transformer():
    from viewcrafter_amd.lvdm.modules import attention as A
    st = A.SpatialTransformer(ST_C, 1, 64, depth=1, context_dim=CDIM, use_checkpoint=False, use_linear=True, image_cross_attention=True).eval()
    sd = {"st." + k: v for k, v in load_synth(st).items()}
    return A, st.to(DEV), sd


def _dev_ctx(ctx, videos=slice(None)):
    txt = ctx["txt"].view(-1, 80, CDIM)[videos].reshape(-1, CDIM).contiguous().to(DEV)
    img = ctx["img"].view(-1, ctx["n_img"], CDIM)[videos].reshape(-1, CDIM).contiguous().to(DEV)
    return dict(txt=txt, img=img, n_img=ctx["n_img"], per_frame=False)


@pytest.mark.parametrize("mode", ["mean", "nearest"])
@pytest.mark.parametrize("H,W", [(16, 32), (8, 12)])
def test_transformer_against_the_pooled_reference(monkeypatch, transformer, H, W, mode):
    A, st, sd = transformer
    x16, ctx, xo, ctx_o = transformer_inputs(H, W)
    _on(monkeypatch, A, mode)
    ref = REF.spatial_transformer(sd, "st", xo, ctx_o, 1)
    x = x16.to(DEV)
    with torch.no_grad():
        off_kv = st.project_context(_dev_ctx(ctx))
        y, _ = st(x, context_kv=off_kv, frames_per_video=2)
        # B = 2 is two B = 1 forwards, bit for bit
        solo = [st(x[2 * i:2 * i + 2].contiguous(), context_kv=st.project_context(_dev_ctx(ctx, slice(i, i + 1))), frames_per_video=2)[0] for i in range(2)]
        # the shared CFG prefix is the replicated batch, bit for bit: one video's frames under two conditionings
        shared, _ = st(x[:2].contiguous(), context_kv=off_kv, frames_per_video=2, cfg_repeat=2)
        repl, _ = st(torch.cat([x[:2], x[:2]]).contiguous(), context_kv=off_kv, frames_per_video=2)
        monkeypatch.setattr(A, "SATTN_KV_POOL", None)
        plain, _ = st(x, context_kv=off_kv, frames_per_video=2)
    torch.cuda.synchronize()
    e = rel_l2(y.float().permute(0, 3, 1, 2), ref)
    print(f"\n[kv-pool] SpatialTransformer({ST_C}, {H}x{W}, {mode}) on the kernels: rel-L2 vs the pooled reference = {e:.3e}; pooled vs un-pooled kernels "
          f"{rel_l2(y, plain):.3e}")
    assert torch.isfinite(y).all() and rel_l2(y, plain) >= 10 * UNET_TOL, "the pooled route did not run"
    assert e <= UNET_TOL
    assert torch.equal(torch.cat(solo), y), "B = 2 differs from two B = 1 forwards"
    assert torch.equal(shared, repl) and not torch.equal(shared[:2], shared[2:]), "the shared CFG prefix differs from the replicated batch"


# ------------------------------------------------------------------------------------------------------------------ 4. tiny UNet
B, T, LH, LW = 1, 2, 16, 32          # latent 16 x 32: 512 / 128 / 32 / 8 tokens a frame; MIN_TOKENS = 128 pools the first two levels


@pytest.fixture(scope="module")
def unet():
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    sd = load_synth(m)
    yield m.to(DEV), sd
    m._graphs.clear()


def _unet_inputs(b=B):
    x = synth_input("kvpool_unet_x", (b, 8, T, LH, LW))
    ctx = synth_input("kvpool_unet_ctx", (b, 77 + 16 * T, TINY_UNET["context_dim"]))
    return x, torch.tensor([799, 350][:b]), ctx, torch.tensor([10, 4][:b])


@pytest.mark.parametrize("mode", ["mean", "nearest"])
def test_tiny_unet_against_the_pooled_oracle_and_graph_replay(monkeypatch, unet, mode):
    from viewcrafter_amd.lvdm.modules import attention as A
    m, sd = unet
    _on(monkeypatch, A, mode, min_tokens=128)
    assert [A.kv_pool_plan(LH >> l, LW >> l, 64) for l in range(4)] == [(8, 16), (4, 8), None, None]
    x, ts, ctx, fs = _unet_inputs()
    with torch.no_grad():
        ref = REF.unet_forward(sd, TINY_UNET, x, ts, ctx, fs)
        y = m(x.to(DEV), ts.to(DEV), context=ctx.to(DEV), fs=fs.to(DEV)).clone()
        m._graphs.clear()
        m.use_hip_graph = True
        try:
            captured = m(x.to(DEV), ts.to(DEV), context=ctx.to(DEV), fs=fs.to(DEV)).clone()
            replayed = m(x.to(DEV), ts.to(DEV), context=ctx.to(DEV), fs=fs.to(DEV)).clone()
        finally:
            m.use_hip_graph = False
            m._graphs.clear()
        monkeypatch.setattr(A, "SATTN_KV_POOL", None)
        plain = m(x.to(DEV), ts.to(DEV), context=ctx.to(DEV), fs=fs.to(DEV)).clone()
    torch.cuda.synchronize()
    e = rel_l2(y, ref)
    print(f"\n[kv-pool] tiny UNet {LH}x{LW}x{T} ({mode}, two levels pooled): rel-L2 vs the pooled oracle = {e:.3e}; pooled vs un-pooled kernels {rel_l2(y, plain):.3e}")
    assert torch.isfinite(y).all() and rel_l2(y, plain) >= 10 * UNET_TOL, "the pooled route did not run"
    assert e <= UNET_TOL
    assert torch.equal(captured, y) and torch.equal(replayed, y), "captured-graph replay differs from eager"


def test_shallow_forward_of_the_feature_cache_with_pooled_levels(monkeypatch, unet):
    """Composition only: a shallow forward at the filling inputs is the full forward's output, bit for bit, with the switch on."""
    from viewcrafter_amd import feature_cache as FC
    from viewcrafter_amd.lvdm.modules import attention as A
    m, _ = unet
    _on(monkeypatch, A, "mean", min_tokens=128)
    x, ts, ctx, fs = [a.to(DEV) for a in _unet_inputs()]
    fc = FC.FeatureCache(depth=1)
    try:
        with torch.no_grad():
            plain = m(x, ts, context=ctx, fs=fs).clone()
            full = m(x, ts, context=ctx, fs=fs, feature_cache=fc).clone()
            fc.set_mode("shallow")
            shallow = m(x, ts, context=ctx, fs=fs, feature_cache=fc).clone()
        torch.cuda.synchronize()
    finally:
        m.drop_feature_cache()
    assert torch.isfinite(full).all() and torch.equal(full, plain) and torch.equal(shallow, full)


def test_beside_sattn_mxfp8_rows_do_not_depend_on_the_batch(monkeypatch):
    """Composition only: both switches on - the two pooled levels run the pooled fp16 route, the two deeper ones the MX route - and row i
    of a B = 2 forward is the B = 1 forward of video i, bit for bit."""
    from viewcrafter_amd.lvdm.modules import attention as A
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    m = m.to(DEV)
    _on(monkeypatch, A, "mean", min_tokens=128)
    x, ts, ctx, fs = [a.to(DEV) for a in _unet_inputs(2)]
    with torch.no_grad():
        pool_only = m(x, ts, context=ctx, fs=fs).clone()
        monkeypatch.setattr(A, "SATTN_MXFP8", True)
        monkeypatch.setattr(A, "SATTN_MXFP8_SKIP_DIMS", frozenset())
        both = m(x, ts, context=ctx, fs=fs).clone()
        solo = [m(x[i:i + 1], ts[i:i + 1], context=ctx[i:i + 1].contiguous(), fs=fs[i:i + 1]).clone() for i in range(2)]
    torch.cuda.synchronize()
    assert torch.isfinite(both).all() and not torch.equal(both, pool_only), "the MX route of the deeper levels did not run"
    for i in range(2):
        assert torch.equal(both[i:i + 1], solo[i]), f"row {i} of the B = 2 forward differs from its B = 1 forward"
