"""ff.net[2] + proj_out of a transformer as ONE GEMM with a linear K tail, on the GPU (csrc/gemm_dma.hip TAIL in linear mode, ops.linear(tail=),
lvdm/modules/attention.py ff_proj_out).  Route and pack: tests/test_ff_out_fold_cpu.py.

The tail is the last K columns in the same K order, and the tile shape does not enter a row's arithmetic, so the tailed call must give the
bits of the plain linear layer on the concatenated operand - output and column moments - under the plan and under every forced tile
configuration that has the form (GEMM_CFG 0-5).  Column moments need whole 64-row strips (M % 64 == 0, vcx_gemm_f16's own rule), so their
variants run on the largest multiple of 64 rows below each M.

Measured on an MI355X (profiles/ff_out_fold.md section 4): module outputs at D = 320 against fp64 of the same fp16 weights 3.02e-4 - 3.20e-4
folded, 3.19e-4 - 3.38e-4 two-step (ratio 0.946 - 0.949), fold against two-step 2.2e-4 - 2.3e-4; tiny UNet against the reference golden
2.376e-3 folded, 2.401e-3 two-step, fold against two-step 2.377e-3.
"""
import pytest
import torch

from tests import exact_inputs as X
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGS = (-1, 0, 1, 2, 3, 4, 5)
SENTINEL = 77.0
# rows: a ragged last tile / one tile of the large configurations, several of the small / 65 tiles of 64 rows + 8
MS = (200, 1000, 64 * 65 + 8)
KS = {"k128_t64": (128, (64,)), "k1280_t320": (1280, (320,)), "k256_t64_64": (256, (64, 64))}
NS = (136, 320)
FOLD_RECORD = []            # (what, fold-vs-two-step rel-L2, fold vs reference, two-step vs reference) of this process


class _forced:
    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        from viewcrafter_amd import ops
        ops.tune_set("GEMM_CFG", self.cfg)

    def __exit__(self, *a):
        from viewcrafter_amd import ops
        ops.tune_set("GEMM_CFG", -1)


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def _problem(M, kmain, tails, N, seed):
    """g [M, kmain], tail sources as column slices of wider buffers (tail_lda = k + 8), w [N, K], bias, residual"""
    K = kmain + sum(tails)
    g = _rnd((M, kmain), seed).half()
    srcs = [_rnd((M, k + 8), seed + 1 + j).half()[:, :k] for j, k in enumerate(tails)]
    w = _rnd((N, K), seed + 5, K ** -0.5).half()
    return g, srcs, w, _rnd((N,), seed + 6, 0.1), _rnd((M, N), seed + 7).half()


def _variants(M):
    """(rows, residual, colstats): all four on whole strips, the two without moments on the ragged M too"""
    m64 = M // 64 * 64
    return [(M, False, False), (M, True, False)] + [(m64, r, True) for r in (False, True)] + ([(m64, True, False)] if m64 != M else [])


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kname", list(KS))
@pytest.mark.parametrize("M", MS)
def test_tailed_call_is_bit_identical_to_the_concatenated_operand(M, kname, N):
    from viewcrafter_amd import ops
    kmain, tails = KS[kname]
    g, srcs, w, b, res = _problem(M, kmain, tails, N, 1000 + M + N)
    cat = torch.cat([g] + srcs, dim=1).contiguous()
    ldc, cld, ccol = N + 24, N + 16, 8
    for rows, with_res, with_cs in _variants(M):
        kw = dict(residual=res[:rows]) if with_res else {}
        assert ops.linear_tail_ok(rows, N, kmain, list(tails), residual=with_res, colstats=with_cs, ldc=ldc)
        # the reference: the plain linear layer on [g | t...], dense output, dense moments - under the plan, once
        cs_ref = ops.colstats_buffer(rows, N, DEV) if with_cs else None
        ref = ops.linear(cat[:rows], w, b, **kw, **(dict(colstats=cs_ref) if with_cs else {}))
        for cfg in CFGS:
            buf = torch.full((rows + 64, ldc), SENTINEL, dtype=torch.float16, device=DEV)
            mom = torch.full((rows // 64 + 2, cld, 2), SENTINEL, dtype=torch.float32, device=DEV) if with_cs else None
            ckw = dict(colstats=mom[:rows // 64], colstats_ld=cld, colstats_col=ccol) if with_cs else {}
            with _forced(cfg):
                y = ops.linear(g[:rows], w, b, tail=[s[:rows] for s in srcs], out=buf[:rows, :N], ldc=ldc, **kw, **ckw)
            what = f"M={rows} {kname} N={N} residual={with_res} colstats={with_cs} GEMM_CFG {cfg}"
            assert torch.equal(y, ref), f"{what}: {int((y != ref).sum())} output elements differ from the concatenated call"
            assert bool((buf[:rows, N:] == SENTINEL).all()) and bool((buf[rows:] == SENTINEL).all()), f"{what}: wrote outside its output"
            if with_cs:
                assert torch.equal(mom[:rows // 64, ccol:ccol + N], cs_ref), f"{what}: column moments differ"
                assert bool((mom[:, :ccol] == SENTINEL).all()) and bool((mom[:, ccol + N:] == SENTINEL).all()) and bool((mom[rows // 64:] == SENTINEL).all())
    # and the values are the layer's: against fp32 of the concatenated operand
    full = cat.float() @ w.float().t() + b
    assert rel_l2(ops.linear(g, w, b, tail=srcs), full) <= 2e-3


def test_plan_with_a_large_tile_segment_and_a_small_tile_tail():
    """Enough rows for whole rounds of 256-row tiles (N = 320: from 384 row tiles on) plus a remainder: the plan's two launches, both tailed."""
    from viewcrafter_amd import ops
    M, N, kmain, tails = 256 * 400 + 200, 320, 128, (64,)
    g, srcs, w, b, res = _problem(M, kmain, tails, N, 77)
    ref = ops.linear(torch.cat([g] + srcs, dim=1).contiguous(), w, b, residual=res)
    y = ops.linear(g, w, b, tail=srcs, residual=res)
    assert torch.equal(y, ref), f"{int((y != ref).sum())} elements differ"
    for cfg in (3, 5):
        with _forced(cfg):
            assert torch.equal(ops.linear(g, w, b, tail=srcs, residual=res), ref), f"GEMM_CFG {cfg}"


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_integers(cfg):
    """Small integers: every product and fp32 partial sum is exact (tests/exact_inputs.py), so the result IS the int64 reference - one wrong
    row, K-step, source or tile is an exact mismatch.  Two row tiles of the largest configuration + a ragged 37 rows, two tail sources."""
    from viewcrafter_amd import ops
    M, N, kmain, tails, ax = 2 * 256 + 37, 136, 128, (128, 64), 3
    K = kmain + sum(tails)
    assert K * ax + 2 * X.ADD <= X.F16_EXACT
    x = X.int_tensor((M, kmain), -ax, ax, 4001)
    srcs = [X.int_tensor((M, k), -ax, ax, 4002 + j) for j, k in enumerate(tails)]
    w = X.int_tensor((N, K), -1, 1, 4010)
    b = X.int_tensor((N,), -X.ADD, X.ADD, 4011).float()
    res = X.int_tensor((M, N), -X.ADD, X.ADD, 4012)
    ref = (torch.cat([x] + srcs, 1).double() @ w.double().t() + b.double() + res.double()).to(torch.int64)
    with _forced(cfg):
        y = ops.linear(x.to(DEV), w.to(DEV), b.to(DEV), tail=[s.to(DEV) for s in srcs], residual=res.to(DEV))
    torch.cuda.synchronize()
    X.assert_exact(y, ref, f"linear K tail GEMM_CFG {cfg}")


def test_refused_call_is_an_error_not_a_fallback():
    from viewcrafter_amd import ops
    from viewcrafter_amd._lib import VcxError
    g, t = torch.zeros((128, 128), dtype=torch.float16, device=DEV), torch.zeros((128, 64), dtype=torch.float16, device=DEV)
    w = torch.zeros((64, 192), dtype=torch.float16, device=DEV)
    with pytest.raises(VcxError, match="tail"):
        ops.linear(g, w, None, tail=[t[:, :32]])                                   # not a whole K-step
    with pytest.raises(VcxError, match="linear K tail"):
        ops.linear(g, w, None, tail=[t], out_f32=True)
    with pytest.raises(VcxError, match="tail"):
        ops.linear(g[:, :72], w[:, :136].contiguous(), None, tail=[t])             # main K % 64 != 0


# ---------------------------------------------------------------- module level
def _round_params_to_fp16(m):
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    return m


def _sd64(m, prefix):
    return {f"{prefix}.{k}": v.double() for k, v in m.state_dict().items()}


def _on_off(run, tr, monkeypatch):
    """run() with the fold on, then off; asserts that the fold was taken / not taken"""
    from viewcrafter_amd.lvdm.modules import attention as A
    monkeypatch.setattr(A, "FF_OUT_FOLD", True)
    tr._drop_packed()
    y_on = run()
    assert "wcat" in tr.packed(), "the fold was not taken"
    monkeypatch.setattr(A, "FF_OUT_FOLD", False)
    tr._drop_packed()
    y_off = run()
    assert "wcat" not in tr.packed(), "VCX_FF_OUT_FOLD = 0 still folds"
    torch.cuda.synchronize()
    return y_on, y_off


def _judge(what, y_on, y_off, ref64):
    e_on, e_off, d = rel_l2(y_on, ref64), rel_l2(y_off, ref64), rel_l2(y_on, y_off.double())
    print(f"\n[ff out fold] {what}: rel-L2 vs fp64 of the fp16 weights: fold {e_on:.3e} two-step {e_off:.3e} (ratio {e_on / e_off:.3f}); fold against two-step {d:.3e}")
    FOLD_RECORD.append((what, d, e_on, e_off))
    assert e_on <= 1.10 * e_off, f"{what}: the folded form is further from the fp64 result ({e_on:.3e}) than the two-step form ({e_off:.3e}) by more than 10 %"
    assert 0 < d, f"{what}: fold on and off gave the same bits - the switch did nothing"


@pytest.mark.parametrize("n,H,W", [(3, 8, 16), (6, 6, 10)])          # 128 tokens per frame; 60 (not a multiple of 8: the padded-token path)
def test_spatial_transformer_fold_on_and_off_against_fp64(n, H, W, monkeypatch):
    from oracle import lvdm_oracle as O
    from viewcrafter_amd.lvdm.modules.attention import SpatialTransformer
    C, heads, cdim, n_img = 320, 5, 128, 16
    torch.manual_seed(5 + n)
    st = SpatialTransformer(C, heads, 64, depth=1, context_dim=cdim, use_checkpoint=False, use_linear=True, image_cross_attention=True).eval()
    with torch.no_grad():
        st.proj_out.weight.normal_(0.0, C ** -0.5)
        st.proj_out.bias.normal_(0.0, 0.1)
    st = _round_params_to_fp16(st).to(DEV)
    x = _rnd((n, H, W, C), 31).half()
    txt, img = _rnd((1, 77, cdim), 32).half(), _rnd((1, n_img, cdim), 33).half()
    txt80 = torch.zeros((80, cdim), dtype=torch.float16, device=DEV)
    txt80[:77] = txt[0]
    with torch.no_grad():
        kv = st.project_context(dict(txt=txt80, img=img[0].contiguous(), n_img=n_img, per_frame=False))
        y_on, y_off = _on_off(lambda: st(x, context_kv=kv, frames_per_video=n)[0], st, monkeypatch)
        ctx64 = torch.cat([txt, img], 1).double().expand(n, -1, -1)
        ref = O.spatial_transformer(_sd64(st, "st"), "st", x.double().permute(0, 3, 1, 2), ctx64, heads).permute(0, 2, 3, 1)
    _judge(f"SpatialTransformer D=320 {n}x{H}x{W}", y_on, y_off, ref)


def test_temporal_transformer_fold_on_and_off_against_fp64(monkeypatch):
    from oracle import lvdm_oracle as O
    from viewcrafter_amd.lvdm.modules.attention import TemporalTransformer
    C, heads, B, T, h, w = 320, 5, 2, 4, 6, 10           # 60 pixels per frame, 240 rows per video
    torch.manual_seed(9)
    tt = TemporalTransformer(C, heads, 64, depth=1, use_checkpoint=False, use_linear=True, only_self_att=True, temporal_length=16).eval()
    with torch.no_grad():
        tt.proj_out.weight.normal_(0.0, C ** -0.5)
        tt.proj_out.bias.normal_(0.0, 0.1)
    tt = _round_params_to_fp16(tt).to(DEV)
    x = _rnd((B, T, h * w, C), 41).half()
    with torch.no_grad():
        y_on, y_off = _on_off(lambda: tt(x)[0], tt, monkeypatch)
        xr = x.double().view(B, T, h, w, C).permute(0, 4, 1, 2, 3)
        ref = O.temporal_transformer(_sd64(tt, "tt"), "tt", xr, heads).permute(0, 2, 3, 4, 1).reshape(B, T, h * w, C)
        one = torch.cat([tt(x[i:i + 1].contiguous())[0] for i in range(B)])          # (the switch is off here: both forms must not depend on the batch)
    assert torch.equal(one, y_off)
    _judge(f"TemporalTransformer D=320 {B}x{T}x{h}x{w}", y_on, y_off, ref)


def test_unet_fold_on_and_off_against_the_reference_golden(monkeypatch):
    """The tiny UNet's B = 2 forward of tests/test_model_gpu.py::test_unet_forward_vs_reference_golden[shared] with the fold on and off:
    both within the project's bound (UNET_TOL) of the reference golden; fold on, B = 2 equals two B = 1 forwards bit for bit."""
    from tests.test_gemm_units_gpu import _forward, _shared_inputs
    from tests.test_model_gpu import UNET_TOL
    from tests.tiny_config import TINY_UNET
    from tests.util import load_synth
    from viewcrafter_amd.lvdm.modules import attention as A
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    m = m.to(DEV)
    x, ctx, ts, fs, gold = _shared_inputs()
    transformers = [t for t in m.modules() if isinstance(t, (A.SpatialTransformer, A.TemporalTransformer))]
    monkeypatch.setattr(A, "FF_OUT_FOLD", True)
    y_on = _forward(m, x, ctx, ts, fs)
    folded = sum("wcat" in t.packed() for t in transformers)
    assert folded, "no transformer took the fold"
    y01 = torch.cat([_forward(m, x, ctx, ts, fs, slice(0, 1)), _forward(m, x, ctx, ts, fs, slice(1, 2))])
    assert torch.equal(y_on, y01), "fold on: the B = 2 forward differs from two B = 1 forwards"
    monkeypatch.setattr(A, "FF_OUT_FOLD", False)
    for t in transformers:
        t._drop_packed()
    y_off = _forward(m, x, ctx, ts, fs)
    assert not any("wcat" in t.packed() for t in transformers)
    e_on, e_off, d = rel_l2(y_on, gold), rel_l2(y_off, gold), rel_l2(y_on, y_off)
    print(f"\n[ff out fold] tiny UNet, {folded} of {len(transformers)} transformers folded: rel-L2 vs reference golden fold {e_on:.3e} two-step {e_off:.3e}; fold against two-step {d:.3e}")
    FOLD_RECORD.append(("tiny UNet", d, e_on, e_off))
    assert e_on <= UNET_TOL and e_off <= UNET_TOL
