"""The MXFP8 temporal attention on the GPU (VCX_TATTN_MXFP8; include/vcx.h vcx_attn_temporal_d64_mxfp8): the quantising attention kernel
against the quantised fp16 kernel and against the format's definition byte for byte, row invariance, the TemporalTransformer's MX route
against the composition of its ops and against the fake-quant route, the skipped width, and the tiny UNet with the switch on and off and
from a captured graph."""
import pytest
import torch

from tests import exact_inputs as X
from tests import mx_emulation as MX
from tests import rounding_quality as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xAB
GUARD = 64          # sentinel rows behind both buffers


def _bytes_equal(got, want, name):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if not torch.equal(got, want):
        bad = got != want
        r, c = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{name}: {X._where(bad)}; got {int(got[r, c]):#04x} want {int(want[r, c]):#04x}")


def _qkv(B, T, P, heads, seed):
    """Random fp16 [B T P, 3 D]; the V columns of head h scaled by 2^(3 h - 4) x a per-(row, head) binade, so that the blocks of a row get
    different scale bytes."""
    D = 64 * heads
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((B * T * P, 3 * D), generator=g)
    e = torch.randint(-2, 3, (B * T * P, heads, 1), generator=g).float() + (3.0 * torch.arange(heads).view(1, heads, 1) - 4.0)
    qkv[:, 2 * D:] = (qkv[:, 2 * D:].view(-1, heads, 64) * torch.exp2(e)).view(-1, D)
    return qkv.half()


def _launch(qkv, B, T, P, heads, causal):
    """vcx_attn_temporal_d64_mxfp8 into poisoned buffers with GUARD sentinel rows behind them -> (q, scales), sentinels checked."""
    from viewcrafter_amd import _lib, ops
    D, rows = 64 * heads, B * T * P
    kp = MX.kp_of(D)
    q = torch.full((rows + GUARD, kp), POISON, dtype=torch.uint8, device=DEV)
    s = torch.full((rows + GUARD, kp // 32), POISON, dtype=torch.uint8, device=DEV)
    ops.check(_lib.lib().vcx_attn_temporal_d64_mxfp8(qkv.data_ptr(), q.data_ptr(), s.data_ptr(), B, T, P, heads, 3 * D, D, 2 * D, 0.125, 4 if causal else 0,
                                                     torch.cuda.current_stream().cuda_stream), "attn_temporal_d64_mxfp8")
    torch.cuda.synchronize()
    assert bool((q[rows:] == POISON).all()) and bool((s[rows:] == POISON).all()), "the kernel wrote behind its buffers"
    return q[:rows], s[:rows]


# ------------------------------------------------------------------------------------------------------------------ 6. kernel = quantised fp16 kernel
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,T,P,heads", [(2, 25, 3, 5), (1, 32, 37, 2), (2, 5, 8, 1), (1, 16, 1, 3)])
def test_kernel_writes_the_quantised_fp16_kernels_bytes(B, T, P, heads, causal):
    from viewcrafter_amd import ops
    D, rows = 64 * heads, B * T * P
    qkv = _qkv(B, T, P, heads, 100 * T + heads).to(DEV)
    o = torch.full((rows, D), float("nan"), dtype=torch.float16, device=DEV)
    ops.temporal_attn(qkv, o, B=B, T=T, P=P, heads=heads, ld=3 * D, k_off=D, v_off=2 * D, ldo=D, scale=0.125, causal=causal)
    torch.cuda.synchronize()
    want_q, want_s = MX.quant(o.cpu())
    assert len(set(want_s[:, :2 * heads].flatten().tolist())) > 3, "the data should spread over several scale bytes"
    q, s = _launch(qkv, B, T, P, heads, causal)
    name = f"tattn_mxfp8 {B}x{T}x{P}x{heads}{' causal' if causal else ''}"
    _bytes_equal(q, want_q, name + " elements (+ padding)")
    _bytes_equal(s, want_s, name + " scales (+ padding)")
    if heads % 2:
        assert bool((q[:, D:] == 0).all()) and bool((s[:, 2 * heads:] == 127).all()) and q.shape[1] == D + 64
    # a second call, through ops, gives the same bytes
    q2, s2 = ops.temporal_attn_mxfp8(qkv, B=B, T=T, P=P, heads=heads, ld=3 * D, k_off=D, v_off=2 * D, scale=0.125, causal=causal)
    torch.cuda.synchronize()
    assert torch.equal(q2, q) and torch.equal(s2, s)


# ------------------------------------------------------------------------------------------------------------------ 7. kernel against the definition
def test_one_frame_is_the_quantised_v():
    """T = 1: the one probability is 1, so the output is V - whatever the fp16 kernel does.  The format's edges planted into V: block
    maxima at powers of two, the 448 edge, fp16 subnormals, zero and -0 blocks, non-finite blocks.  One thing the attention does to V on the
    way: a value is the fp32 sum  0 + 1 x v,  and  (+0) + (-0) = +0  in round-to-nearest, so a -0 of V arrives as +0 (byte 0x00, not 0x80) -
    in the fp16 kernel as well.  The expected bytes are therefore quant(V + 0): every value and every other byte as quant(V)."""
    B, P, heads = 2, 9, 3
    D, rows = 64 * heads, B * P
    qkv = _qkv(B, 1, P, heads, 7).clone()
    v = qkv[:, 2 * D:].contiguous()
    where = MX.plant_boundaries(v.view(2 * rows, D // 2))          # a row of 96 = three whole blocks: block boundaries stay where they are
    assert len(where) == len(MX.boundary_blocks())
    qkv[:, 2 * D:] = v
    want_q, want_s = MX.quant(v)
    neg_zero = (v.view(torch.int16) == -32768)
    assert int(neg_zero.sum()) == 1 and int(want_q[:, :D][neg_zero]) == 0x80
    want_q[:, :D][neg_zero] = 0x00
    q, s = _launch(qkv.to(DEV), B, 1, P, heads, False)
    for name, (r, b) in where.items():                                      # the planted blocks first, by name
        row, blk = r // 2, (r % 2) * 3 + b
        _bytes_equal(s[row:row + 1, blk:blk + 1], want_s[row:row + 1, blk:blk + 1], f"scale of block '{name}'")
        _bytes_equal(q[row:row + 1, 32 * blk:32 * blk + 32], want_q[row:row + 1, 32 * blk:32 * blk + 32], f"elements of block '{name}'")
    _bytes_equal(q, want_q, "T = 1 elements (+ padding)")
    _bytes_equal(s, want_s, "T = 1 scales (+ padding)")


# ------------------------------------------------------------------------------------------------------------------ 8. row invariance
def test_a_row_does_not_depend_on_the_call():
    T, P, heads = 25, 5, 2
    D = 64 * heads
    qkv3 = _qkv(3, T, P, heads, 31).to(DEV)
    q3, s3 = _launch(qkv3, 3, T, P, heads, False)
    q1, s1 = _launch(qkv3[:T * P].contiguous(), 1, T, P, heads, False)
    _bytes_equal(q1, q3[:T * P], "first video alone, elements")
    _bytes_equal(s1, s3[:T * P], "first video alone, scales")


# ------------------------------------------------------------------------------------------------------------------ 9. TemporalTransformer
def _transformer(C, **kw):
    from viewcrafter_amd.lvdm.modules import attention as A
    torch.manual_seed(C)
    tr = A.TemporalTransformer(C, C // 64, 64, **kw).eval()
    with torch.no_grad():
        tr.proj_out.weight.copy_(torch.randn(tr.proj_out.weight.shape) * C ** -0.5)       # (zero-initialised: the branch would not show)
        tr.proj_out.bias.copy_(0.1 * torch.randn(C))
        for m in tr.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.2 * torch.randn(C))
                m.bias.copy_(0.1 * torch.randn(C))
        for blk in tr.transformer_blocks:
            for a in (blk.attn1, blk.attn2):
                a.to_out[0].bias.copy_(0.1 * torch.randn(C))
    return A, tr.to(DEV)


def _attention_by_hand(ops, attn, lnp, t, B, T, P, causal):
    D, heads = t.shape[1], t.shape[1] // 64
    am = attn.mx_packed()
    a = ops.layer_norm_mxfp8(t, *lnp)
    qkv = ops.linear_mxfp8(a, am["wqkv"], am["zero"], K=D)
    o = ops.temporal_attn_mxfp8(qkv, B=B, T=T, P=P, heads=heads, ld=3 * D, k_off=D, v_off=2 * D, scale=attn.scale, causal=causal)
    return ops.linear_mxfp8(o, am["wo"], am["bo"], K=D, residual=t)


@pytest.mark.parametrize("C,causal", [(64, False), (128, False), (320, False), (128, True)])
def test_transformer_on_the_mx_route_is_the_composition_of_its_ops(C, causal, monkeypatch):
    from viewcrafter_amd import ops
    A, tr = _transformer(C, **(dict(causal_attention=True, temporal_length=4) if causal else {}))
    B, T, P = 2, 4, 24
    x = (R.randn((B, T, P, C), 8000 + C) * 1.3).half().to(DEV)
    with torch.no_grad():
        y16, _ = tr(x)
        monkeypatch.setattr(A, "TATTN_MXFP8", True)
        monkeypatch.setattr(A, "TATTN_MXFP8_SKIP_DIMS", frozenset())
        ymx, _ = tr(x)
        # the chain, written out (at this size the per-video norm is a pass of its own)
        pk, blk = tr.packed(), tr.transformer_blocks[0]
        ln = blk.ln_params()
        tokens = B * T * P
        a = ops.group_norm(x.view(B, T * P, C), pk["gn_w"], pk["gn_b"], tr.norm.eps, False)
        t = ops.linear(a.view(tokens, C), pk["win"], pk["bin"])
        for attn, lnp in ((blk.attn1, ln[0]), (blk.attn2, ln[1])):
            t = _attention_by_hand(ops, attn, lnp, t, B, T, P, causal)
        y = A.ff_proj_out(tr, t, ln[2], x.reshape(tokens, C), {}, T * P).view(B, T, P, C)
    torch.cuda.synchronize()
    assert torch.equal(ymx, y), f"the transformer differs from the chain of its ops in {int((ymx != y).sum())} elements"
    assert torch.isfinite(ymx).all() and not torch.equal(ymx, y16), "the MX route did not run"
    print(f"\n[mxfp8] TemporalTransformer({C}{', causal' if causal else ''}): rel-L2(MX - fp16) of the branch = "
          f"{rel_l2(ymx.float() - x.float(), y16.float() - x.float()):.3e}")


# ------------------------------------------------------------------------------------------------------------------ 10. against fake-quant
def _dq16(pair, K):
    return MX.dequant(pair[0], pair[1], K).half().to(DEV)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_transformer_mx_route_against_fake_quant(D, monkeypatch):
    """One attention layer's branch (the residual stream subtracted) three ways, rows = 2 x 4 x 75.  Figures of the MI355X run are in
    profiles/mxfp8_tattn.md.
      fp16 route:  the module's own fp16 calls (ln_linear, temporal_attn, linear + residual);
      fake-quant:  pre-existing kernels only - dq(layer_norm_mxfp8(t)) through the fp16 linear with the dequantised Wqkv, the fp16
                   attention kernel, dq(quant_mxfp8(o)) through the fp16 linear with the dequantised Wo, bias and residual;
      MX route:    what the module computed - input and output of attn1's to_out, taken from the forward itself.
    d_quant = rel-L2(fake-quant - fp16) is fixed by code that existed before the MX route and is the yardstick; the MX route may differ from
    fake-quant only by fp32 summation order and by the rare fp16-ulp flip of o that moves one e4m3 step: d_kernel < 0.25 d_quant (estimate
    of those effects: at most 0.1; a wrong scale byte, a swapped block or a dropped head gives 1 or more)."""
    from viewcrafter_amd import ops
    A, tr = _transformer(D)
    B, T, P = 2, 4, 75
    x = (R.randn((B, T, P, D), 9000 + D) * 1.3).half().to(DEV)
    monkeypatch.setattr(A, "TATTN_MXFP8", True)
    monkeypatch.setattr(A, "TATTN_MXFP8_SKIP_DIMS", frozenset())
    seen = []
    real = ops.linear_mxfp8

    def spy(a, w, bias, **kw):
        out = real(a, w, bias, **kw)
        if kw.get("residual") is not None:
            seen.append((kw["residual"], out))
        return out
    monkeypatch.setattr(ops, "linear_mxfp8", spy)
    with torch.no_grad():
        tr(x)
        assert len(seen) == 2, "two attentions with a residual each"
        t, ymx = seen[0]
        blk = tr.transformer_blocks[0]
        attn, lnp = blk.attn1, blk.ln_params()[0]
        ap, am = attn.packed(), attn.mx_packed()
        heads, tokens = D // 64, B * T * P
        geo = dict(B=B, T=T, P=P, heads=heads, ld=3 * D, k_off=D, v_off=2 * D, ldo=D, scale=attn.scale)
        # fp16 route
        qkv = A.ln_linear(t, ap["qkv"], lnp)
        o = ops.temporal_attn(qkv, torch.empty((tokens, D), dtype=torch.float16, device=DEV), **geo)
        y16 = ops.linear(o, ap["wo"], ap["bo"], residual=t)
        # fake quant
        qkv = ops.linear(_dq16(ops.layer_norm_mxfp8(t, *lnp), D), _dq16(am["wqkv"], D))
        o = ops.temporal_attn(qkv, torch.empty((tokens, D), dtype=torch.float16, device=DEV), **geo)
        yfq = ops.linear(_dq16(ops.quant_mxfp8(o), D), _dq16(am["wo"], D), ap["bo"], residual=t)
    torch.cuda.synchronize()
    assert torch.isfinite(ymx).all()
    tf = t.float()
    d_kernel, d_quant = rel_l2(ymx.float() - tf, yfq.float() - tf), rel_l2(yfq.float() - tf, y16.float() - tf)
    print(f"\n[mxfp8] temporal attention D {D}: rel-L2(MX - fake-quant) {d_kernel:.3e}, rel-L2(fake-quant - fp16) {d_quant:.3e}, ratio {d_kernel / max(d_quant, 1e-30):.4f}")
    assert d_quant > 0
    assert d_kernel < 0.25 * d_quant, f"D {D}: the MX route deviates from fake-quant by {d_kernel / d_quant:.3f} of the quantisation effect itself (limit 0.25)"


# ------------------------------------------------------------------------------------------------------------------ 11. skipped width
def test_transformer_keeps_fp16_at_a_skipped_width(monkeypatch):
    A, tr = _transformer(320)
    assert 320 in A.TATTN_MXFP8_SKIP_DIMS, "320 is skipped by default"
    x = (R.randn((2, 4, 24, 320), 8500) * 1.3).half().to(DEV)
    packs = lambda: [a for blk in tr.transformer_blocks for a in (blk.attn1, blk.attn2) if a._pk is not None and "mx" in a._pk]
    with torch.no_grad():
        y16, _ = tr(x)
        monkeypatch.setattr(A, "TATTN_MXFP8", True)
        kept, _ = tr(x)
        assert packs() == [], "an MX pack was built at a skipped width"
        monkeypatch.setattr(A, "TATTN_MXFP8_SKIP_DIMS", frozenset())
        ymx, _ = tr(x)
    torch.cuda.synchronize()
    assert torch.equal(kept, y16) and len(packs()) == 2
    assert torch.isfinite(ymx).all() and not torch.equal(ymx, y16)


# ------------------------------------------------------------------------------------------------------------------ 12. / 13. tiny UNet
def _tiny_unet():
    from tests.tiny_config import TINY_UNET
    from tests.util import load_synth
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    return m.to(DEV), TINY_UNET


def _switch_on(monkeypatch, all_four):
    from viewcrafter_amd.lvdm.modules import attention as A
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    monkeypatch.setattr(A, "TATTN_MXFP8", True)
    monkeypatch.setattr(A, "TATTN_MXFP8_SKIP_DIMS", frozenset())
    if all_four:
        for mod, name in ((A, "FF"), (U, "TCONV"), (U, "RESCONV")):
            monkeypatch.setattr(mod, name + "_MXFP8", True)
            monkeypatch.setattr(mod, name + "_MXFP8_SKIP_DIMS", frozenset())


@pytest.mark.parametrize("all_four", [False, True])
def test_tiny_unet_with_the_switch_on_and_off(all_four):
    from oracle.weights import synth_input
    from viewcrafter_amd.lvdm.modules import attention as A
    m, cfg = _tiny_unet()
    t, h, w, L = 4, 16, 32, 77 + 64
    x = synth_input("mx_x", (2, 8, t, h, w)).to(DEV)
    x[1] = x[0]
    ctx = synth_input("mx_ctx", (2, L, cfg["context_dim"])).to(DEV)
    ts, fs = torch.tensor([799, 799], device=DEV), torch.tensor([10, 10], device=DEV)
    with torch.no_grad():
        before = m._forward(x, ts, context=ctx, fs=fs)             # the module flags have never been touched
        with pytest.MonkeyPatch.context() as mp:
            _switch_on(mp, all_four)
            on = m._forward(x, ts, context=ctx, fs=fs)
            ones = torch.cat([m._forward(x[i:i + 1].contiguous(), ts[:1], context=ctx[i:i + 1].contiguous(), fs=fs[:1]) for i in range(2)])
            shared = m._forward(x[:1].contiguous(), ts[:1], context=ctx, fs=fs[:1], cfg_repeat=2)
        off = m._forward(x, ts, context=ctx, fs=fs)
    torch.cuda.synchronize()
    n_tr = sum(isinstance(b, A.TemporalTransformer) for b in m.modules())
    n_mx = sum("mx" in (a._pk or {}) for b in m.modules() if isinstance(b, A.TemporalTransformer) for blk in b.transformer_blocks for a in (blk.attn1, blk.attn2))
    assert n_tr > 0 and n_mx == 2 * n_tr, f"every width on MX: {n_mx} packs for {n_tr} temporal transformers"
    assert torch.isfinite(on).all()
    assert not torch.equal(on, before), "the switch changed nothing: the MX route did not run"
    assert torch.equal(ones, on), f"B = 2 differs from two B = 1 forwards in {int((ones != on).sum())} elements"
    assert torch.equal(shared, on), f"the shared CFG prefix differs from the replicated batch in {int((shared != on).sum())} elements"
    assert torch.equal(off, before), f"switch off: {int((off != before).sum())} elements differ from the run before it was ever on"
    print(f"\n[mxfp8] tiny UNet, temporal attention{' + the other three switches' if all_four else ''}: rel-L2(on - off) = {rel_l2(on, off):.3e}")


def test_tiny_unet_with_the_switch_on_replays_from_a_captured_graph(monkeypatch):
    """The MX route is capturable: the packs (pack_mxfp8 runs on the host) are built by the warm-up forward ahead of the capture, the
    predicates touch no device, nothing on the path synchronises.  The replay is bit-equal to the eager forward, also with new inputs."""
    from oracle.weights import synth_input
    m, cfg = _tiny_unet()
    _switch_on(monkeypatch, False)
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
