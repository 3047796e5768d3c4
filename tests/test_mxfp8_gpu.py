"""The MXFP8 path on the GPU (include/vcx.h "MXFP8 operands"; opt-in feed-forward, VCX_FF_MXFP8): the quantisers against the torch
definition byte for byte, vcx_gemm_mxfp8 on operands with exactly known products, its GEGLU epilogues, row invariance, FeedForward.run
against the fake-quant route, and the tiny UNet with the switch on and off.  Conditions of the exact data: tests/test_mxfp8_cpu.py."""
import ctypes

import pytest
import torch

from tests import exact_inputs as X
from tests import mx_emulation as MX
from tests import rounding_quality as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xAB


def _random_f16(rows, K, seed, spread=6):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, K // 32, 32), generator=g)
    e = torch.randint(-spread, spread + 1, (rows, K // 32, 1), generator=g)
    return (x * torch.exp2(e.float())).view(rows, K).half()


def _bytes_equal(got, want, name):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if not torch.equal(got, want):
        bad = got != want
        r, c = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{name}: {X._where(bad)}; got {int(got[r, c]):#04x} want {int(want[r, c]):#04x}")


def _pair(q, s):
    return q.to(DEV), s.to(DEV)


# ------------------------------------------------------------------------------------------------------------------ quantisers
@pytest.mark.parametrize("rows,K,ldx", [(300, 320, 328), (65, 1280, 1280)])
def test_quantiser_writes_the_definitions_bytes_and_nothing_else(rows, K, ldx):
    from viewcrafter_amd import _lib, ops
    x = _random_f16(rows, K, 5 + K)
    where = MX.plant_boundaries(x)
    qe, se = MX.quant(x)
    buf = torch.full((rows, ldx), 777.0, dtype=torch.float16)
    buf[:, :K] = x
    xd = buf.to(DEV)[:, :K]
    kp = MX.kp_of(K)
    # one guard row in front and behind, everything poisoned: the kernel writes every byte of its rows (padding included) and no other
    q = torch.full((rows + 2, kp), POISON, dtype=torch.uint8, device=DEV)
    s = torch.full((rows + 2, kp // 32), POISON, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().vcx_quant_mxfp8_f16(xd.data_ptr(), ldx, q[1].data_ptr(), s[1].data_ptr(), rows, K, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for name, (r, b) in where.items():
        _, scale, elems = MX.boundary_blocks()[name]
        assert int(s[1 + r, b]) == scale, (name, int(s[1 + r, b]), scale)
        for i, byte in elems.items():
            assert int(q[1 + r, b * 32 + i]) == byte, (name, i, hex(int(q[1 + r, b * 32 + i])), hex(byte))
    _bytes_equal(q[1:-1], qe, "elements")
    _bytes_equal(s[1:-1], se, "scales")
    for g in (q[0], q[-1], s[0], s[-1]):
        assert bool((g == POISON).all()), "a guard row was written"
    q2, s2 = ops.quant_mxfp8(xd)
    _bytes_equal(q2, qe, "ops.quant_mxfp8 elements")
    _bytes_equal(s2, se, "ops.quant_mxfp8 scales")


def test_pack_mxfp8_agrees_with_the_kernel_quantiser():
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_mxfp8
    w = _random_f16(136, 320, 91)
    MX.plant_boundaries(w)
    q, s = pack_mxfp8(w.to(DEV))
    qk, sk = ops.quant_mxfp8(w.to(DEV))
    assert q.is_cuda and s.is_cuda
    _bytes_equal(q, qk, "elements")
    _bytes_equal(s, sk, "scales")


@pytest.mark.parametrize("rows,C", [(300, 320), (130, 640), (70, 1280), (40, 64)])      # every lanes-per-row geometry the widths 64 .. 1280 take
def test_layernorm_quantiser_is_the_quantised_layernorm(rows, C):
    from viewcrafter_amd import ops
    x = (R.randn((rows, C), 40 + C) * 1.7 + 0.3).half().to(DEV)
    x[3] *= 50.0                       # a loud row and a nearly constant one
    x[5] = 2.0
    x[5, 7] = 2.002
    gamma, beta = (1.0 + 0.3 * R.randn((C,), 41)).to(DEV), (0.2 * R.randn((C,), 42)).to(DEV)
    q, s = ops.layer_norm_mxfp8(x, gamma, beta, 1e-5)
    qr, sr = ops.quant_mxfp8(ops.layer_norm(x, gamma, beta, 1e-5))
    torch.cuda.synchronize()
    _bytes_equal(q, qr, "elements")
    _bytes_equal(s, sr, "scales")
    assert q.shape == (rows, MX.kp_of(C))


# ------------------------------------------------------------------------------------------------------------------ GEMM, exact data
def _addends(M, N, seed):
    """bias fp32 [N] and residual fp16 [M, N] on the 2^-2 grid, magnitudes <= 64"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-256, 257, (N,), generator=g).float() * MX.GRID,
            (torch.randint(-256, 257, (M, N), generator=g).float() * MX.GRID).half())


def _assert_fp16_bits(out, ref64, name):
    got, want = out.cpu(), ref64.half()
    assert got.dtype == torch.float16 and got.shape == want.shape
    if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        bad = got.view(torch.int16) != want.view(torch.int16)
        r, c = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{name}: {X._where(bad)}; got {float(got[r, c])} want {float(want[r, c])}")


@pytest.mark.parametrize("M,N,K,residual", [(300, 320, 1280, True), (257, 640, 320, False), (1, 64, 128, False), (600, 640, 2560, True)])
def test_gemm_is_exact_on_the_integer_grid(M, N, K, residual):
    """out == fp16(sum + bias [+ residual]) bit for bit: elements in [-7, 7], scale exponents in {-1, 0, 1} per (row, block) on both
    operands, an asymmetric W - a swapped lane map, a misplaced scale byte or a dropped K padding block is an exact mismatch."""
    from viewcrafter_amd import ops
    aq, asc, a = MX.exact_operand(M, K, 100 + M)
    wq, wsc, w = MX.exact_operand(N, K, 200 + N)
    assert not torch.equal(w[:min(N, K), :min(N, K)], w[:min(N, K), :min(N, K)].t())
    bias, res = _addends(M, N, 300 + K)
    ref = a @ w.t() + bias.double()
    if residual:
        ref = ref + res.double()
    assert float(ref.abs().max()) < (1 << 24) * MX.GRID and float(ref.abs().max()) < 65504
    out = ops.linear_mxfp8(_pair(aq, asc), _pair(wq, wsc), bias.to(DEV), K=K, residual=res.to(DEV) if residual else None)
    torch.cuda.synchronize()
    _assert_fp16_bits(out, ref, f"gemm_mxfp8 {M}x{N}x{K}")


# ------------------------------------------------------------------------------------------------------------------ GEGLU epilogues
def _pack_geglu_mx(q, s, bias):
    from viewcrafter_amd.packing import pack_geglu
    qp, bp = pack_geglu(q, bias)
    return (qp, pack_geglu(s, None)[0]), bp


@pytest.mark.parametrize("name,M,K,D,ea,ew", [("k320", 300, 320, 160, -4, -5), ("k64", 300, 64, 128, -4, -4)])
def test_geglu_fp16_out_rounds_once(name, M, K, D, ea, ew):
    """x * gelu_erf(gate) against fp64 of the SAME operands with exact accumulators (integer-grid data scaled to outputs of order one):
    the only errors are the gate's fp32 evaluation and one fp16 rounding - the bound of the fp16 engine's GEGLU test
    (tests/rounding_quality.py: E <= 1.05, mismatch <= 10 %)."""
    from viewcrafter_amd import ops
    aq, asc, a = MX.exact_operand(M, K, 400 + K, e_offset=ea)
    wq, wsc, w = MX.exact_operand(2 * D, K, 500 + K, e_offset=ew)
    bias = R.randn((2 * D,), 600 + K)
    wp, bp = _pack_geglu_mx(wq, wsc, bias)
    out = ops.linear_mxfp8(_pair(aq, asc), _pair(*wp), bp.to(DEV), K=K, geglu=True)
    torch.cuda.synchronize()
    assert out.shape == (M, D)
    ref = R.geglu_ref(a @ w.t() + bias.double())
    R.check_rounding("gemm_mxfp8_geglu", name, out, ref)


def _random_problem(M, N, K, seed):
    """MXFP8 operands of N(0, 1) activations and N(0, 1 / K) weights, bias N(0, 1): outputs of order one."""
    from viewcrafter_amd import ops
    a = ops.quant_mxfp8(R.randn((M, K), seed + 1).half().to(DEV))
    w = ops.quant_mxfp8(R.randn((N, K), seed + 2, K ** -0.5).half().to(DEV))
    return a, w, R.randn((N,), seed + 3).to(DEV)


@pytest.mark.parametrize("M,N,K", [(300, 2560, 320), (130, 5120, 640), (65, 320, 64)])
def test_geglu_mxfp8_out_is_the_quantised_fp16_out(M, N, K):
    """(65, 320, 64): 160 output columns - the last 96 of the 256-byte rows are the K padding the epilogue writes itself."""
    from viewcrafter_amd import ops
    a, w, bias = _random_problem(M, N, K, 700 + K)
    h = ops.linear_mxfp8(a, w, bias, K=K, geglu=True)
    q, s = ops.linear_mxfp8(a, w, bias, K=K, geglu=True, mx_out=True)
    qr, sr = ops.quant_mxfp8(h)
    torch.cuda.synchronize()
    assert torch.isfinite(h).all() and float(h.float().abs().max()) > 0.5
    _bytes_equal(q, qr, "elements")
    _bytes_equal(s, sr, "scales")
    qe, se = MX.quant(h.cpu())
    _bytes_equal(q, qe, "elements against the torch definition")
    _bytes_equal(s, se, "scales against the torch definition")


@pytest.mark.parametrize("epi", ["residual", "geglu", "geglu_mx"])
def test_rows_do_not_depend_on_the_call_size(epi):
    from viewcrafter_amd import ops
    N, K = (320, 1280) if epi == "residual" else (2560, 320)
    a, w, bias = _random_problem(320, N, K, 800)
    res = R.randn((320, N), 804).half().to(DEV)
    kw = dict(residual=res) if epi == "residual" else dict(geglu=True, mx_out=epi == "geglu_mx")
    kw64 = dict(kw, residual=res[:64].contiguous()) if epi == "residual" else kw
    big = ops.linear_mxfp8(a, w, bias, K=K, **kw)
    small = ops.linear_mxfp8((a[0][:64].contiguous(), a[1][:64].contiguous()), w, bias, K=K, **kw64)
    torch.cuda.synchronize()
    for b, s_ in zip(big if epi == "geglu_mx" else (big,), small if epi == "geglu_mx" else (small,)):
        assert torch.equal(b[:64], s_), f"{epi}: {int((b[:64] != s_).sum())} elements of rows 0..63 depend on M"


# ------------------------------------------------------------------------------------------------------------------ FeedForward.run
# rel-L2(MX - fake-quant) / rel-L2(fake-quant - fp16) of the feed-forward branch as measured on the MI355X (600 rows, the inputs below;
# profiles/mxfp8_ff.md): the MX kernels deviate from the fake-quant route by 1 - 2 % of what quantising changes at all.  The kernels are
# deterministic, so the figure is a property of the code; the test asserts twice the measured value (and so, far below 1).
FF_RATIO_MEASURED = {64: 0.0094, 128: 0.0207, 256: 0.0107}


def _dq16(pair, K):
    return MX.dequant(pair[0], pair[1], K).half().to(DEV)


@pytest.mark.parametrize("dim", [64, 128, 256])
def test_feed_forward_mx_route_against_fake_quant(dim, monkeypatch):
    """The fake-quant route is the fp16 kernels fed the dequantised operands (exact in fp16): it differs from the MX route by the fp32
    summation order and by an occasional fp16-ulp flip of the GEGLU output that moves one quantisation step."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.lvdm.modules import attention as A
    from viewcrafter_amd.packing import pack_geglu
    torch.manual_seed(dim)
    ff = A.FeedForward(dim, glu=True).eval()
    ln = torch.nn.LayerNorm(dim)
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.2 * torch.randn(dim))
        ln.bias.copy_(0.1 * torch.randn(dim))
    ff._pre_norm = [ln]
    ff, ln = ff.to(DEV), ln.to(DEV)
    rows = 600
    t = (R.randn((rows, dim), 900 + dim) * 1.3).half().to(DEV)
    lnp = (ln.weight.detach().float().contiguous(), ln.bias.detach().float().contiguous(), ln.eps)
    with torch.no_grad():
        monkeypatch.setattr(A, "FF_MXFP8", False)
        y16 = ff.run(t, lnp)
        monkeypatch.setattr(A, "FF_MXFP8", True)
        assert ff._mx_ok(t)
        ymx = ff.run(t, lnp)
        # fake quant
        pk = ff.packed()
        proj = ff.net[0].proj
        w1, b1 = pack_geglu(proj.weight.detach().half(), proj.bias.detach().float())
        a = _dq16(ops.layer_norm_mxfp8(t, *lnp), dim)
        g = ops.linear(a, _dq16(pk["mx"]["w1"], dim), b1, geglu=True)
        yfq = ops.linear(_dq16(ops.quant_mxfp8(g), 4 * dim), _dq16(pk["mx"]["w2"], 4 * dim), pk["b2"], residual=t)
    torch.cuda.synchronize()
    assert torch.isfinite(ymx).all() and not torch.equal(ymx, y16)
    # the residual stream t is common to all three: compare the feed-forward branches
    d_kernel, d_quant = rel_l2(ymx.float() - t.float(), yfq.float() - t.float()), rel_l2(yfq.float() - t.float(), y16.float() - t.float())
    ratio = d_kernel / d_quant
    print(f"\n[mxfp8] FeedForward dim {dim}: rel-L2(MX - fake-quant) {d_kernel:.3e}, rel-L2(fake-quant - fp16) {d_quant:.3e}, ratio {ratio:.4f}")
    assert d_quant > 0
    limit = min(2 * FF_RATIO_MEASURED[dim], 0.99)
    assert ratio < limit, f"dim {dim}: the MX kernels deviate from fake-quant by {ratio:.3f} of the quantisation effect itself (limit {limit:.3f})"


def test_feed_forward_keeps_fp16_at_a_skipped_width(monkeypatch):
    """Width 320 is in FF_MXFP8_SKIP_DIMS by default (its MX pair was measured no faster): switch on, the output is the fp16 route's, bit
    for bit, and no MX pack is built; with the set emptied the same module takes the MX route."""
    from viewcrafter_amd.lvdm.modules import attention as A
    torch.manual_seed(320)
    ff = A.FeedForward(320, glu=True).eval()
    ln = torch.nn.LayerNorm(320)
    ff._pre_norm = [ln]
    ff, ln = ff.to(DEV), ln.to(DEV)
    t = (R.randn((200, 320), 950) * 1.3).half().to(DEV)
    lnp = (ln.weight.detach().float().contiguous(), ln.bias.detach().float().contiguous(), ln.eps)
    assert 320 in A.FF_MXFP8_SKIP_DIMS
    with torch.no_grad():
        y16 = ff.run(t, lnp)
        monkeypatch.setattr(A, "FF_MXFP8", True)
        kept = ff.run(t, lnp)
        assert "mx" not in ff.packed()
        monkeypatch.setattr(A, "FF_MXFP8_SKIP_DIMS", frozenset())
        ymx = ff.run(t, lnp)
    torch.cuda.synchronize()
    assert torch.equal(kept, y16) and "mx" in ff.packed()
    assert torch.isfinite(ymx).all() and not torch.equal(ymx, y16)


# ------------------------------------------------------------------------------------------------------------------ tiny UNet
def test_tiny_unet_with_the_switch_on_and_off(monkeypatch):
    from oracle.weights import synth_input
    from tests.tiny_config import TINY_UNET
    from tests.util import load_synth
    from viewcrafter_amd.lvdm.modules import attention as A
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    m = m.to(DEV)
    t, h, w, L = 4, 16, 32, 77 + 64
    x = synth_input("mx_x", (2, 8, t, h, w)).to(DEV)
    x[1] = x[0]
    ctx = synth_input("mx_ctx", (2, L, TINY_UNET["context_dim"])).to(DEV)
    ts, fs = torch.tensor([799, 799], device=DEV), torch.tensor([10, 10], device=DEV)
    with torch.no_grad():
        before = m._forward(x, ts, context=ctx, fs=fs)             # the module flag has never been touched
        monkeypatch.setattr(A, "FF_MXFP8", True)
        on = m._forward(x, ts, context=ctx, fs=fs)
        ones = torch.cat([m._forward(x[i:i + 1].contiguous(), ts[:1], context=ctx[i:i + 1].contiguous(), fs=fs[:1]) for i in range(2)])
        shared = m._forward(x[:1].contiguous(), ts[:1], context=ctx, fs=fs[:1], cfg_repeat=2)
        monkeypatch.setattr(A, "FF_MXFP8", False)
        off = m._forward(x, ts, context=ctx, fs=fs)
    torch.cuda.synchronize()
    assert torch.isfinite(on).all()
    assert not torch.equal(on, before), "the switch changed nothing: the MX route did not run"
    assert torch.equal(ones, on), f"B = 2 differs from two B = 1 forwards in {int((ones != on).sum())} elements"
    assert torch.equal(shared, on), f"the shared CFG prefix differs from the replicated batch in {int((shared != on).sum())} elements"
    assert torch.equal(off, before), f"switch off: {int((off != before).sum())} elements differ from the run before it was ever on"
    print(f"\n[mxfp8] tiny UNet: rel-L2(on - off) = {rel_l2(on, off):.3e}")


def test_tiny_unet_with_the_switch_on_replays_from_a_captured_graph(monkeypatch):
    """The MX route is capturable: packs (pack_mxfp8 runs on the host) are built by the warm-up forward ahead of the capture, the shape
    predicate touches no device, nothing on the path synchronises.  The replay is bit-equal to the eager forward, also with new inputs."""
    from oracle.weights import synth_input
    from tests.tiny_config import TINY_UNET
    from tests.util import load_synth
    from viewcrafter_amd.lvdm.modules import attention as A
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    m = m.to(DEV)
    monkeypatch.setattr(A, "FF_MXFP8", True)
    T, h, w = 4, 16, 32
    ctx = synth_input("mxg_ctx", (2, 77 + 16 * T, TINY_UNET["context_dim"])).to(DEV)
    fs = torch.tensor([10, 10], device=DEV)
    try:
        for k, tval in enumerate((999, 479)):
            x = synth_input(f"mxg_x{k}", (2, TINY_UNET["in_channels"], T, h, w)).to(DEV)
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
