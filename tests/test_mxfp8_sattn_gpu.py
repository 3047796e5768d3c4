"""The MXFP8 spatial attention on the GPU (VCX_SATTN_MXFP8; include/vcx.h vcx_attn_flash_d64_mxfp8 / vcx_attn_flash_dual_d64_mxfp8): the
quantising store tail of the three spatial attention kernels against the quantised fp16 kernels and against the format's definition byte
for byte, row invariance, the transposed MX projection, the SpatialTransformer's MX route against the composition of its ops and against
the fake-quant route, the skipped width, and the tiny UNet with the switch on and off and from a captured graph."""
import math

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
LOG2 = 2            # include/vcx.h VCX_ATTN_LOG2_LOGITS


def _bytes_equal(got, want, name):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if not torch.equal(got, want):
        bad = got != want
        r, c = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{name}: {X._where(bad)}; got {int(got[r, c]):#04x} want {int(want[r, c]):#04x}")


def _poisoned(rows, heads):
    kp = MX.kp_of(64 * heads)
    return (torch.full((rows + GUARD, kp), POISON, dtype=torch.uint8, device=DEV),
            torch.full((rows + GUARD, kp // 32), POISON, dtype=torch.uint8, device=DEV))


def _checked(q, s, rows):
    torch.cuda.synchronize()
    assert bool((q[rows:] == POISON).all()) and bool((s[rows:] == POISON).all()), "the kernel wrote behind its buffers"
    return q[:rows], s[:rows]


def _kv(sets, rows, heads, g):
    """K [sets * rows, D] and V^T [D, sets * rows] fp16.  The values of (key row, head) are scaled by a binade of their own, 2^(-6 .. 6) (as
    _qkv of the temporal test does per (row, head)); with unit-variance q and k the base-2 logits have a standard deviation of 8, so a
    query's output is dominated by few keys and the blocks of the output get many different scale bytes."""
    D = 64 * heads
    k = torch.randn((sets * rows, D), generator=g)
    v = torch.randn((sets * rows, heads, 64), generator=g)
    v = v * torch.exp2(torch.randint(-6, 7, (sets * rows, heads, 1), generator=g).float())
    return k.half().to(DEV), v.view(-1, D).t().contiguous().half().to(DEV)


def _single_problem(G, heads, nq, nk, kv_rows, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((G * nq, 64 * heads), generator=g).half().to(DEV)
    k, vt = _kv(G, kv_rows, heads, g)
    return q, k, vt


def _single_geo(G, heads, nq, nk, kv_rows):
    D = 64 * heads
    return dict(n_groups=G, heads=heads, nq=nq, nk=nk, kv_rows=kv_rows, kv_div=1, ldq=D, ldk=D, ldvt=G * kv_rows)


def _launch_single(q, k, vt, geo):
    from viewcrafter_amd import _lib, ops
    rows = geo["n_groups"] * geo["nq"]
    oq, os_ = _poisoned(rows, geo["heads"])
    ops.check(_lib.lib().vcx_attn_flash_d64_mxfp8(q.data_ptr(), k.data_ptr(), vt.data_ptr(), oq.data_ptr(), os_.data_ptr(), geo["n_groups"], geo["heads"],
                                                  geo["nq"], geo["nk"], geo["kv_rows"], geo["kv_div"], geo["ldq"], geo["ldk"], geo["ldvt"], 1.0, LOG2,
                                                  torch.cuda.current_stream().cuda_stream), "attn_flash_d64_mxfp8")
    return _checked(oq, os_, rows)


def _fp16_single(q, k, vt, geo):
    from viewcrafter_amd import ops
    D = 64 * geo["heads"]
    o = torch.full((geo["n_groups"] * geo["nq"], D), float("nan"), dtype=torch.float16, device=DEV)
    ops.flash_attn(q, k, vt, o, ldo=D, scale=1.0, log2_logits=True, **geo)
    torch.cuda.synchronize()
    return o


def _compare(got, o16, heads, name):
    q, s = got
    D = 64 * heads
    want_q, want_s = MX.quant(o16.cpu())
    assert len(set(want_s[:, :2 * heads].flatten().tolist())) > 3, "the data should spread over several scale bytes"
    _bytes_equal(q, want_q, name + " elements (+ padding)")
    _bytes_equal(s, want_s, name + " scales (+ padding)")
    if heads % 2:
        assert bool((q[:, D:] == 0).all()) and bool((s[:, 2 * heads:] == 127).all()) and q.shape[1] == D + 64


class _knobs:
    """ops.tune_set for the length of a with block; the old values come back in any case."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from viewcrafter_amd import ops
        self.old = {k: ops.tune_get(k) for k in self.kw}
        for k, v in self.kw.items():
            ops.tune_set(k, v)

    def __exit__(self, *exc):
        from viewcrafter_amd import ops
        for k, v in self.old.items():
            ops.tune_set(k, v)


# ------------------------------------------------------------------------------------------------------------------ 1. kernel = quantised fp16 kernel
# (epilogue, G, heads, nq, nk, kv_rows, knobs): the smallest shapes that reach every store tail behind vcx_attn_flash_d64_mxfp8
SINGLE = [("flash_d64 QB1 ragged key tile, odd heads", 2, 3, 72, 72, 72, {}),
          ("flash_d64 QB1 padded tokens", 1, 1, 64, 60, 64, {}),
          ("flash_d64 QB2", 1, 2, 232, 232, 232, {}),
          ("flash2 natural dispatch, partial query block", 1, 3, 2112, 2112, 2112, {}),
          ("flash2 forced", 2, 1, 192, 192, 192, {"FLASH_IMPL": 2}),
          ("flash2 forced, padded tokens", 1, 1, 200, 192, 200, {"FLASH_IMPL": 2})]


@pytest.mark.parametrize("name,G,heads,nq,nk,kv_rows,knobs", SINGLE, ids=[c[0].replace(" ", "_").replace(",", "") for c in SINGLE])
def test_single_entry_writes_the_quantised_fp16_kernels_bytes(name, G, heads, nq, nk, kv_rows, knobs):
    from viewcrafter_amd import ops
    q, k, vt = _single_problem(G, heads, nq, nk, kv_rows, 1000 + nq + heads)
    geo = _single_geo(G, heads, nq, nk, kv_rows)
    with _knobs(**knobs):
        o16 = _fp16_single(q, k, vt, geo)
        got = _launch_single(q, k, vt, geo)
        q2, s2 = ops.flash_attn_mxfp8(q, k, vt, **geo)          # a second call, through ops, gives the same bytes
        torch.cuda.synchronize()
    _compare(got, o16, heads, name)
    assert torch.equal(q2, got[0]) and torch.equal(s2, got[1])


def _dual_problem(G, heads, nq, nk2, kv_div2, seed):
    """8 frames of two videos (kv_div1 = 4): 77 text keys in 80 rows per video, and nk2 image keys per video (kv_div2 = 4) or frame (1)."""
    D = 64 * heads
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((G * nq, D), generator=g).half().to(DEV)
    k1, vt1 = _kv(G // 4, 80, heads, g)
    k2, vt2 = _kv(G // kv_div2, nk2, heads, g)
    geo = dict(n_groups=G, heads=heads, nq=nq, nk1=77, kv_rows1=80, kv_div1=4, ldk1=D, ldvt1=(G // 4) * 80, nk2=nk2, kv_rows2=nk2, kv_div2=kv_div2,
               ldk2=D, ldvt2=(G // kv_div2) * nk2, ldq=D)
    return (q, k1, vt1, k2, vt2), geo


def _launch_dual(t, geo):
    from viewcrafter_amd import _lib, ops
    rows = geo["n_groups"] * geo["nq"]
    oq, os_ = _poisoned(rows, geo["heads"])
    g = geo
    ops.check(_lib.lib().vcx_attn_flash_dual_d64_mxfp8(*[x.data_ptr() for x in t], oq.data_ptr(), os_.data_ptr(), g["n_groups"], g["heads"], g["nq"], g["nk1"],
                                                       g["kv_rows1"], g["kv_div1"], g["ldk1"], g["ldvt1"], g["nk2"], g["kv_rows2"], g["kv_div2"], g["ldk2"],
                                                       g["ldvt2"], g["ldq"], 1.0, LOG2, torch.cuda.current_stream().cuda_stream), "attn_flash_dual_d64_mxfp8")
    return _checked(oq, os_, rows)


def _fp16_dual(t, geo):
    from viewcrafter_amd import ops
    D = 64 * geo["heads"]
    o = torch.full((geo["n_groups"] * geo["nq"], D), float("nan"), dtype=torch.float16, device=DEV)
    ops.flash_attn_dual(*t, o, ldo=D, scale=1.0, log2_logits=True, **geo)
    torch.cuda.synchronize()
    return o


# (kernel, heads, nq, nk2, kv_div2)
DUAL = [("resident2 one iteration", 3, 40, 64, 4), ("resident2 two iterations", 3, 136, 64, 4), ("DUAL flash QB1", 2, 40, 16, 1), ("DUAL flash QB2", 2, 232, 16, 1)]


@pytest.mark.parametrize("name,heads,nq,nk2,kv_div2", DUAL, ids=[c[0].replace(" ", "_") for c in DUAL])
def test_dual_entry_writes_the_quantised_fp16_kernels_bytes(name, heads, nq, nk2, kv_div2):
    from viewcrafter_amd import ops
    t, geo = _dual_problem(8, heads, nq, nk2, kv_div2, 2000 + nq + heads)
    assert ops.flash_attn_dual_mxfp8_ok(**geo)
    o16 = _fp16_dual(t, geo)
    got = _launch_dual(t, geo)
    q2, s2 = ops.flash_attn_dual_mxfp8(*t, **geo)
    torch.cuda.synchronize()
    _compare(got, o16, heads, name)
    assert torch.equal(q2, got[0]) and torch.equal(s2, got[1])


def test_dual_entry_refuses_the_first_form_resident_kernel():
    """Knob XATTN_RESIDENT = 2 (A/B runs) selects the first-form kernel, which has no MX store tail: predicate and launcher refuse, nothing runs."""
    from viewcrafter_amd import _lib, ops
    t, geo = _dual_problem(8, 3, 40, 64, 4, 5)
    with _knobs(XATTN_RESIDENT=2):
        assert not ops.flash_attn_dual_mxfp8_ok(**geo) and b"first-form" in _lib.lib().vcx_last_error()
        with pytest.raises(ops.VcxError):
            ops.flash_attn_dual_mxfp8(*t, **geo)
    assert ops.flash_attn_dual_mxfp8_ok(**geo)


# ------------------------------------------------------------------------------------------------------------------ 2. kernel against the definition
def test_one_key_is_the_quantised_v():
    """nk = 1: the one probability is 1, so every output row of a group is that group's V row - whatever the fp16 kernel does.  The format's
    edges planted into V: block maxima at powers of two, the 448 edge, fp16 subnormals, zero and -0 blocks, non-finite blocks.  As in the
    temporal test a value is the fp32 sum  0 + 1 x v,  and  (+0) + (-0) = +0,  so a -0 of V arrives as +0 (byte 0x00, not 0x80) - in the fp16
    kernel as well: on the finite blocks the expected bytes are quant(V + 0).  (The two heads that hold the inf and the nan block are held
    to the fp16 kernel only.)"""
    G, heads, nq = 12, 3, 8
    D = 64 * heads
    g = torch.Generator().manual_seed(7)
    v = (torch.randn((G, heads, 64), generator=g) * torch.exp2(torch.randint(-6, 7, (G, heads, 1), generator=g).float())).view(G, D).half()
    where = MX.plant_boundaries(v.view(2 * G, D // 2))          # a row of 96 = three whole blocks: block boundaries stay where they are
    assert len(where) == len(MX.boundary_blocks())
    q = torch.randn((G * nq, D), generator=g).half().to(DEV)
    k = torch.randn((G * 8, D), generator=g).half().to(DEV)
    vt = torch.zeros((D, G * 8), dtype=torch.float16)
    vt[:, ::8] = v.t()
    geo = dict(n_groups=G, heads=heads, nq=nq, nk=1, kv_rows=8, kv_div=1, ldq=D, ldk=D, ldvt=G * 8)
    o16 = _fp16_single(q, k, vt.to(DEV), geo)
    got_q, got_s = _launch_single(q, k, vt.to(DEV), geo)
    want_q, want_s = MX.quant(o16.cpu())
    _bytes_equal(got_q, want_q, "nk = 1 elements (+ padding) against the fp16 kernel")
    _bytes_equal(got_s, want_s, "nk = 1 scales (+ padding) against the fp16 kernel")
    # the definition: quant(V + 0), every query row of a group alike, on the heads whose V is finite
    vq, vs = MX.quant(v)
    neg_zero = (v.view(torch.int16) == -32768)
    assert int(neg_zero.sum()) == 1 and int(vq[:, :D][neg_zero]) == 0x80
    vq[:, :D][neg_zero] = 0x00
    finite_head = torch.isfinite(v.float()).view(G, heads, 64).all(-1)
    assert int((~finite_head).sum()) == 2, "the inf and the nan block"
    checked = 0
    for name, (r, b) in where.items():
        grp, blk = r // 2, (r % 2) * 3 + b
        if not finite_head[grp, blk // 2]:
            continue
        for row in (grp * nq, grp * nq + nq - 1):
            _bytes_equal(got_s[row:row + 1, blk:blk + 1], vs[grp:grp + 1, blk:blk + 1], f"scale of block '{name}'")
            _bytes_equal(got_q[row:row + 1, 32 * blk:32 * blk + 32], vq[grp:grp + 1, 32 * blk:32 * blk + 32], f"elements of block '{name}'")
        checked += 1
    assert checked == len(where) - 2
    for grp in range(G):
        for h in range(heads):
            if finite_head[grp, h]:
                rows = slice(grp * nq, grp * nq + nq)
                _bytes_equal(got_q[rows, 64 * h:64 * h + 64], vq[grp:grp + 1, 64 * h:64 * h + 64].expand(nq, -1), f"group {grp} head {h} elements against quant(V)")
                _bytes_equal(got_s[rows, 2 * h:2 * h + 2], vs[grp:grp + 1, 2 * h:2 * h + 2].expand(nq, -1), f"group {grp} head {h} scales against quant(V)")


# ------------------------------------------------------------------------------------------------------------------ 3. row invariance
def test_a_group_does_not_depend_on_the_call():
    G, heads, nq = 3, 2, 72
    q, k, vt = _single_problem(G, heads, nq, nq, nq, 31)
    q3, s3 = _launch_single(q, k, vt, _single_geo(G, heads, nq, nq, nq))
    q1, s1 = _launch_single(q[:nq].contiguous(), k[:nq].contiguous(), vt[:, :nq].contiguous(), _single_geo(1, heads, nq, nq, nq))
    _bytes_equal(q1, q3[:nq], "first group alone, elements")
    _bytes_equal(s1, s3[:nq], "first group alone, scales")
    # the dual entry: the first video (4 frames) alone
    t, geo = _dual_problem(8, 3, 136, 64, 4, 32)
    q8, s8 = _launch_dual(t, geo)
    t4 = (t[0][:4 * 136].contiguous(), t[1][:80].contiguous(), t[2][:, :80].contiguous(), t[3][:64].contiguous(), t[4][:, :64].contiguous())
    q4, s4 = _launch_dual(t4, dict(geo, n_groups=4, ldvt1=80, ldvt2=64))
    _bytes_equal(q4, q8[:4 * 136], "first video alone (dual), elements")
    _bytes_equal(s4, s8[:4 * 136], "first video alone (dual), scales")


# ------------------------------------------------------------------------------------------------------------------ 4. the transposed projection
@pytest.mark.parametrize("tokens,D", [(600, 64), (1096, 192)])
def test_linear_t_is_the_transposed_linear(tokens, D):
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_mxfp8
    x = ops.quant_mxfp8((R.randn((tokens, D), 40 + D) * 1.5).half().to(DEV))
    w = pack_mxfp8((R.randn((D, D), 41 + D) * D ** -0.5).half().to(DEV))
    assert ops.linear_t_mxfp8_ok(tokens, D, D)
    yt = ops.linear_t_mxfp8(x, w, K=D)
    y = ops.linear_mxfp8(x, w, torch.zeros(D, dtype=torch.float32, device=DEV), K=D)
    torch.cuda.synchronize()
    assert tuple(yt.shape) == (D, tokens) and torch.isfinite(y).all() and float(y.float().abs().max()) > 0
    assert torch.equal(yt, y.t()), f"{int((yt != y.t()).sum())} elements differ"


# ------------------------------------------------------------------------------------------------------------------ 5. SpatialTransformer
CDIM, N_IMG = 128, 16


def _transformer(C):
    from viewcrafter_amd.lvdm.modules import attention as A
    torch.manual_seed(C)
    st = A.SpatialTransformer(C, C // 64, 64, depth=1, context_dim=CDIM, use_checkpoint=False, use_linear=True, image_cross_attention=True).eval()
    with torch.no_grad():
        st.proj_out.weight.copy_(torch.randn(st.proj_out.weight.shape) * C ** -0.5)       # (zero-initialised: the branch would not show)
        st.proj_out.bias.copy_(0.1 * torch.randn(C))
        for m in st.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.2 * torch.randn(C))
                m.bias.copy_(0.1 * torch.randn(C))
        for blk in st.transformer_blocks:
            for a in (blk.attn1, blk.attn2):
                a.to_out[0].bias.copy_(0.1 * torch.randn(C))
    return A, st.to(DEV)


def _context(st, videos, seed):
    txt = torch.zeros((videos, 80, CDIM), dtype=torch.float16)
    txt[:, :77] = R.randn((videos, 77, CDIM), seed).half()
    img = R.randn((videos * N_IMG, CDIM), seed + 1).half()
    with torch.no_grad():
        return st.project_context(dict(txt=txt.view(videos * 80, CDIM).to(DEV), img=img.to(DEV), n_img=N_IMG, per_frame=False))


def _on(monkeypatch, A):
    monkeypatch.setattr(A, "SATTN_MXFP8", True)
    monkeypatch.setattr(A, "SATTN_MXFP8_SKIP_DIMS", frozenset())


def _chain(A, ops, st, kv, x, fpv):
    """SpatialTransformer.forward on the MX route, written out for depth 1 and at sizes where the norm is a pass of its own."""
    n, H, W, C = x.shape
    N_img, D, heads = H * W, C, C // 64
    N = (N_img + 7) // 8 * 8
    pk, blk, kv = st.packed(), st.transformer_blocks[0], kv[0]
    ln, m1, m2 = blk.ln_params(), blk.attn1.mx_packed(), blk.attn2.mx_packed()
    a = ops.group_norm(x.view(n, N_img, C), pk["gn_w"], pk["gn_b"], st.norm.eps, False)
    xin = x.reshape(n * N_img, C)
    if N != N_img:
        def pad(src):
            dst = torch.zeros((n * N, C), dtype=torch.float16, device=DEV)
            ops.copy2d(src, dst, n, N_img * C, N_img * C, N * C)
            return dst
        xin, a = pad(xin), pad(a.view(n * N_img, C))
    tokens = n * N
    t = ops.linear(a.view(tokens, C), pk["win"], pk["bin"])
    an = ops.layer_norm_mxfp8(t, *ln[0])
    qk = ops.linear_mxfp8(an, m1["wqk"], m1["zero"], K=D)
    vt = ops.linear_t_mxfp8(an, m1["wv"], K=D)
    o = ops.flash_attn_mxfp8(qk, qk[:, D:], vt, n_groups=n, heads=heads, nq=N, nk=N_img, kv_rows=N, kv_div=1, ldq=2 * D, ldk=2 * D, ldvt=tokens)
    t = ops.linear_mxfp8(o, m1["wo"], m1["bo"], K=D, residual=t)
    q2 = ops.linear_mxfp8(ops.layer_norm_mxfp8(t, *ln[1]), m2["wq"], m2["zero"], K=D)
    o2 = ops.flash_attn_dual_mxfp8(q2, kv.k_txt, kv.vt_txt, kv.k_img, kv.vt_img, n_groups=n, heads=heads, nq=N, nk1=kv.n_txt, kv_rows1=80, kv_div1=fpv,
                                   ldk1=D, ldvt1=kv.n_txt_rows, nk2=kv.n_img, kv_rows2=kv.n_img, kv_div2=fpv, ldk2=D, ldvt2=kv.vt_img.shape[1], ldq=D)
    t = ops.linear_mxfp8(o2, m2["wo"], m2["bo"], K=D, residual=t)
    out = A.ff_proj_out(st, t, ln[2], xin, {}, fpv * N)
    if N != N_img:
        unp = torch.empty((n * N_img, C), dtype=torch.float16, device=DEV)
        ops.copy2d(out, unp, n, N_img * C, N * C, N_img * C)
        out = unp
    return out.view(n, H, W, C)


@pytest.mark.parametrize("C,H,W", [(64, 6, 8), (128, 6, 8), (320, 6, 8), (128, 6, 10)])          # 6 x 10 = 60 tokens: the padded case
def test_transformer_on_the_mx_route_is_the_composition_of_its_ops(C, H, W, monkeypatch):
    from viewcrafter_amd import ops
    A, st = _transformer(C)
    fpv, n = 4, 8
    kv = _context(st, 2, 600 + C)
    x = (R.randn((n, H, W, C), 8000 + C + W) * 1.3).half().to(DEV)
    with torch.no_grad():
        y16, _ = st(x, context_kv=kv, frames_per_video=fpv)
        _on(monkeypatch, A)
        ymx, _ = st(x, context_kv=kv, frames_per_video=fpv)
        y = _chain(A, ops, st, kv, x, fpv)
    torch.cuda.synchronize()
    assert torch.equal(ymx, y), f"the transformer differs from the chain of its ops in {int((ymx != y).sum())} elements"
    assert torch.isfinite(ymx).all() and not torch.equal(ymx, y16), "the MX route did not run"
    print(f"\n[mxfp8] SpatialTransformer({C}, {H}x{W}): rel-L2(MX - fp16) of the branch = "
          f"{rel_l2(ymx.float() - x.float(), y16.float() - x.float()):.3e}")


def test_transformer_shared_cfg_prefix_equals_the_replicated_input(monkeypatch):
    A, st = _transformer(128)
    _on(monkeypatch, A)
    kv = _context(st, 2, 77)
    x = (R.randn((4, 6, 8, 128), 8300) * 1.3).half().to(DEV)
    with torch.no_grad():
        shared, _ = st(x, context_kv=kv, frames_per_video=4, cfg_repeat=2)
        repl, _ = st(torch.cat([x, x]).contiguous(), context_kv=kv, frames_per_video=4)
    torch.cuda.synchronize()
    assert tuple(shared.shape) == (8, 6, 8, 128) and torch.isfinite(shared).all()
    assert torch.equal(shared, repl), f"{int((shared != repl).sum())} elements differ"
    assert not torch.equal(shared[:4], shared[4:]), "the two conditionings should differ"


# ------------------------------------------------------------------------------------------------------------------ 6. against fake-quant
def _dq16(pair, K):
    return MX.dequant(pair[0], pair[1], K).half().to(DEV)


FAKE_QUANT_RECORD = []


@pytest.mark.parametrize("D", [64, 128, 256])
def test_transformer_mx_route_against_fake_quant(D, monkeypatch):
    """The branch of each of the two attentions (the residual stream subtracted) three ways, 8 frames of 6 x 8 tokens.  Figures of the
    MI355X run are in profiles/mxfp8_sattn.md.
      fp16 route:  the module's own fp16 calls (ln_linear, ln_linear_t, the flash kernels, linear + residual);
      fake-quant:  pre-existing kernels only - dq(layer_norm_mxfp8(t)) through the fp16 GEMMs with the dequantised MX weights, the fp16
                   attention kernel, dq(quant_mxfp8(o)) through the fp16 linear with the dequantised Wo, bias and residual;
      MX route:    what the module computed - input and output of each to_out, taken from the forward itself.
    d_quant = rel-L2(fake-quant - fp16) is fixed by code that existed before the MX route and is the yardstick; the MX route may differ from
    fake-quant only by fp32 summation order and by the rare fp16-ulp flip that moves one e4m3 step: d_kernel < 0.25 d_quant (the
    project's bound for every MX route; a wrong scale byte, a swapped block or a dropped head gives 1 or more)."""
    from viewcrafter_amd import ops
    A, st = _transformer(D)
    n, H, W, fpv = 8, 6, 8, 4
    N, heads, tokens = H * W, D // 64, n * H * W
    kv = _context(st, 2, 900 + D)
    x = (R.randn((n, H, W, D), 9000 + D) * 1.3).half().to(DEV)
    _on(monkeypatch, A)
    seen = []
    real = ops.linear_mxfp8

    def spy(a, w, bias, **kw):
        out = real(a, w, bias, **kw)
        if kw.get("residual") is not None:
            seen.append((kw["residual"], out))
        return out
    monkeypatch.setattr(ops, "linear_mxfp8", spy)
    with torch.no_grad():
        st(x, context_kv=kv, frames_per_video=fpv)
        assert len(seen) == 2, "two attentions with a residual each"
        blk, c = st.transformer_blocks[0], kv[0]
        ln = blk.ln_params()
        empty = lambda: torch.empty((tokens, D), dtype=torch.float16, device=DEV)
        geo1 = dict(n_groups=n, heads=heads, nq=N, nk=N, kv_rows=N, kv_div=1, ldq=2 * D, ldk=2 * D, ldvt=tokens, ldo=D, scale=1.0, log2_logits=True)
        geo2 = dict(n_groups=n, heads=heads, nq=N, nk1=c.n_txt, kv_rows1=80, kv_div1=fpv, ldk1=D, ldvt1=c.n_txt_rows, nk2=c.n_img, kv_rows2=c.n_img, kv_div2=fpv,
                    ldk2=D, ldvt2=c.vt_img.shape[1], ldq=D, ldo=D, scale=1.0, log2_logits=True)
        results = []
        # ---- self-attention
        (t, ymx), a1, m1 = seen[0], blk.attn1.packed(), blk.attn1.mx_packed()
        qk = A.ln_linear(t, a1["qk"], ln[0], alpha=math.sqrt(blk.attn1.scale * ops.LOG2E))
        o = ops.flash_attn(qk, qk[:, D:], A.ln_linear_t(t, a1["v"], ln[0]), empty(), **geo1)
        y16 = ops.linear(o, a1["wo"], a1["bo"], residual=t)
        an = _dq16(ops.layer_norm_mxfp8(t, *ln[0]), D)
        qk = ops.linear(an, _dq16(m1["wqk"], D))
        vt = ops.gemm(_dq16(m1["wv"], D), an, M=D, N=tokens, K=D, lda=D)
        o = ops.flash_attn(qk, qk[:, D:], vt, empty(), **geo1)
        yfq = ops.linear(_dq16(ops.quant_mxfp8(o), D), _dq16(m1["wo"], D), a1["bo"], residual=t)
        results.append(("self", t, ymx, yfq, y16))
        # ---- cross-attention
        (t, ymx), a2, m2 = seen[1], blk.attn2.packed(), blk.attn2.mx_packed()
        q2 = A.ln_linear(t, a2["q"], ln[1], alpha=blk.attn2.scale * ops.LOG2E)
        o = ops.flash_attn_dual(q2, c.k_txt, c.vt_txt, c.k_img, c.vt_img, empty(), **geo2)
        y16 = ops.linear(o, a2["wo"], a2["bo"], residual=t)
        q2 = ops.linear(_dq16(ops.layer_norm_mxfp8(t, *ln[1]), D), _dq16(m2["wq"], D))
        o = ops.flash_attn_dual(q2, c.k_txt, c.vt_txt, c.k_img, c.vt_img, empty(), **geo2)
        yfq = ops.linear(_dq16(ops.quant_mxfp8(o), D), _dq16(m2["wo"], D), a2["bo"], residual=t)
        results.append(("cross", t, ymx, yfq, y16))
    torch.cuda.synchronize()
    for which, t, ymx, yfq, y16 in results:
        assert torch.isfinite(ymx).all()
        tf = t.float()
        d_kernel, d_quant = rel_l2(ymx.float() - tf, yfq.float() - tf), rel_l2(yfq.float() - tf, y16.float() - tf)
        print(f"\n[mxfp8] spatial {which}-attention D {D}: rel-L2(MX - fake-quant) {d_kernel:.3e}, rel-L2(fake-quant - fp16) {d_quant:.3e}, "
              f"ratio {d_kernel / max(d_quant, 1e-30):.4f}")
        FAKE_QUANT_RECORD.append((which, D, d_kernel, d_quant))
    for which, D_, d_kernel, d_quant in FAKE_QUANT_RECORD[-2:]:
        assert d_quant > 0
        assert d_kernel < 0.25 * d_quant, f"{which} D {D_}: the MX route deviates from fake-quant by {d_kernel / d_quant:.3f} of the quantisation effect itself (limit 0.25)"


# ------------------------------------------------------------------------------------------------------------------ 7. skipped width
def test_transformer_keeps_fp16_at_a_skipped_width(monkeypatch):
    A, st = _transformer(320)
    assert 320 in A.SATTN_MXFP8_SKIP_DIMS, "320 is skipped by default"
    kv = _context(st, 2, 55)
    x = (R.randn((8, 6, 8, 320), 8500) * 1.3).half().to(DEV)
    packs = lambda: [a for blk in st.transformer_blocks for a in (blk.attn1, blk.attn2) if a._pk is not None and "mx" in a._pk]
    with torch.no_grad():
        y16, _ = st(x, context_kv=kv, frames_per_video=4)
        monkeypatch.setattr(A, "SATTN_MXFP8", True)
        kept, _ = st(x, context_kv=kv, frames_per_video=4)
        assert packs() == [], "an MX pack was built at a skipped width"
        monkeypatch.setattr(A, "SATTN_MXFP8_SKIP_DIMS", frozenset())
        ymx, _ = st(x, context_kv=kv, frames_per_video=4)
    torch.cuda.synchronize()
    assert torch.equal(kept, y16) and len(packs()) == 2
    assert torch.isfinite(ymx).all() and not torch.equal(ymx, y16)


# ------------------------------------------------------------------------------------------------------------------ 8. / 9. tiny UNet
def _tiny_unet():
    from tests.tiny_config import TINY_UNET
    from tests.util import load_synth
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    return m.to(DEV), TINY_UNET


def _switch_on(monkeypatch, all_five):
    from viewcrafter_amd.lvdm.modules import attention as A
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    _on(monkeypatch, A)
    if all_five:
        for mod, name in ((A, "FF"), (U, "TCONV"), (U, "RESCONV"), (A, "TATTN")):
            monkeypatch.setattr(mod, name + "_MXFP8", True)
            monkeypatch.setattr(mod, name + "_MXFP8_SKIP_DIMS", frozenset())


@pytest.mark.parametrize("all_five", [False, True])
def test_tiny_unet_with_the_switch_on_and_off(all_five):
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
            _switch_on(mp, all_five)
            on = m._forward(x, ts, context=ctx, fs=fs)
            ones = torch.cat([m._forward(x[i:i + 1].contiguous(), ts[:1], context=ctx[i:i + 1].contiguous(), fs=fs[:1]) for i in range(2)])
            shared = m._forward(x[:1].contiguous(), ts[:1], context=ctx, fs=fs[:1], cfg_repeat=2)
        off = m._forward(x, ts, context=ctx, fs=fs)
    torch.cuda.synchronize()
    attns = [a for b in m.modules() if isinstance(b, A.SpatialTransformer) for blk in b.transformer_blocks for a in (blk.attn1, blk.attn2)]
    n_mx = sum("mx" in (a._pk or {}) for a in attns)
    assert attns and n_mx == len(attns), f"every width on MX: {n_mx} packs for {len(attns)} spatial attentions"
    assert torch.isfinite(on).all()
    assert not torch.equal(on, before), "the switch changed nothing: the MX route did not run"
    assert torch.equal(ones, on), f"B = 2 differs from two B = 1 forwards in {int((ones != on).sum())} elements"
    assert torch.equal(shared, on), f"the shared CFG prefix differs from the replicated batch in {int((shared != on).sum())} elements"
    assert torch.equal(off, before), f"switch off: {int((off != before).sum())} elements differ from the run before it was ever on"
    print(f"\n[mxfp8] tiny UNet, spatial attention{' + the other four switches' if all_five else ''}: rel-L2(on - off) = {rel_l2(on, off):.3e}")


def test_tiny_unet_with_the_switch_on_replays_from_a_captured_graph(monkeypatch):
    """The MX route is capturable: the packs and the cached zero bias are built by the warm-up forward ahead of the capture, the
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
