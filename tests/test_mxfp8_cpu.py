"""The MXFP8 format (include/vcx.h "MXFP8 operands") without a GPU: the torch definition at the format's edges, packing.pack_mxfp8
against it, the exactness conditions tests/test_mxfp8_gpu.py relies on, and vcx_gemm_mxfp8_ok (which touches no device)."""
import itertools

import pytest
import torch

from tests import mx_emulation as MX
from viewcrafter_amd import _lib
from viewcrafter_amd.packing import pack_mxfp8

G = _lib


def _random_f16(rows, K, seed, spread=6):
    """N(0, 1) values times a per-block power of two in [2^-spread, 2^spread]: blocks of every scale."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, K // 32, 32), generator=g)
    e = torch.randint(-spread, spread + 1, (rows, K // 32, 1), generator=g)
    return (x * torch.exp2(e.float())).view(rows, K).half()


def test_torch_cast_is_the_saturating_round_to_nearest_even_the_definition_assumes():
    f = lambda v: float(torch.tensor(v, dtype=torch.float32).clamp(-448, 448).to(torch.float8_e4m3fn).float())
    assert f(464.0) == 448.0 and f(465.0) == 448.0 and f(1e9) == 448.0 and f(-500.0) == -448.0
    assert f(1.5 * 2.0 ** -10) == 2.0 ** -9 and f(2.0 ** -10) == 0.0 and f(3 * 2.0 ** -10) == 2.0 ** -8
    assert f(17.0) == 16.0 and f(19.0) == 20.0 and f(18.0) == 18.0          # ties to even at 3 mantissa bits


@pytest.mark.parametrize("name", sorted(MX.boundary_blocks()))
def test_boundary_blocks(name):
    v, scale, elems = MX.boundary_blocks()[name]
    q, s = MX.quant(v.view(1, 32))
    assert q.shape == (1, 128) and s.shape == (1, 4)
    assert int(s[0, 0]) == scale, (name, int(s[0, 0]))
    for i, byte in elems.items():
        assert int(q[0, i]) == byte, (name, i, hex(int(q[0, i])), hex(byte))
    finite = bool(torch.isfinite(v).all())
    assert finite == (not bool(((q[0, :32] & 0x7F) == 0x7F).any())), "0x7F / 0xFF exactly where the block is not finite"
    if finite and scale:
        assert 95 <= scale <= 134
        # the largest element sits in the top binade of e4m3 after scaling: [256, 448]
        assert 256.0 <= float(q[0, :32].view(torch.float8_e4m3fn).float().abs().max()) <= 448.0
    assert torch.equal(q[0, 32:], torch.zeros(96, dtype=torch.uint8)) and s[0, 1:].tolist() == [127, 127, 127]


def test_padding_of_k_320():
    x = _random_f16(5, 320, 1)
    q, s = MX.quant(x)
    assert q.shape == (5, 384) and s.shape == (5, 12)
    assert not bool(q[:, 320:].any()) and bool((s[:, 10:] == 127).all())
    assert torch.equal(MX.quant(x[:, :128].contiguous())[0], q[:, :128])        # a block does not depend on its neighbours
    # in units of 2^(E - 8) the block's values lie below 512 and the e4m3 step is at most 32: half a step, 16, is the error of every value
    # up to 464; the values above clamp to 448 and are off by less than 64
    dq = MX.dequant(q, s, 320)
    xb = x.double().view(5, 10, 32)
    unit = torch.exp2(MX.block_exponent(xb.abs().amax(dim=2, keepdim=True).float()).double() - 8)
    err = (xb - dq.view(5, 10, 32)).abs() / unit
    assert bool((err <= torch.where(xb.abs() / unit <= 464, 16.0, 64.0)).all())


@pytest.mark.parametrize("rows,K", [(37, 320), (9, 1280), (24, 64)])
def test_pack_mxfp8_is_the_emulation(rows, K):
    x = _random_f16(rows, K, 7 + K)
    MX.plant_boundaries(x) if rows >= 2 * len(MX.boundary_blocks()) else None
    q, s = pack_mxfp8(x)
    qe, se = MX.quant(x)
    assert q.dtype == s.dtype == torch.uint8 and torch.equal(q, qe) and torch.equal(s, se)
    with pytest.raises(ValueError):
        pack_mxfp8(x[:, :48])


def test_every_fp16_magnitude_gets_the_exponent_of_its_leading_bit():
    """pack_mxfp8's integer route (exponent field, leading mantissa bit of subnormals) against frexp, over EVERY finite fp16 magnitude."""
    mags = torch.arange(1, 0x7C00, dtype=torch.int32).to(torch.int16).view(torch.float16)
    x = torch.zeros((mags.numel(), 32), dtype=torch.float16)
    x[:, 5] = -mags
    (q, s), (qe, se) = pack_mxfp8(x), MX.quant(x)
    assert torch.equal(s, se) and torch.equal(q, qe)
    assert int(s[:, 0].min()) == 95 and int(s[:, 0].max()) == 134
    top = q[:, 5].view(torch.float8_e4m3fn).float().abs()
    assert float(top.min()) == 256.0 and float(top.max()) == 448.0


# ------------------------------------------------------------------------------------------------------------------ exactness conditions
def test_exact_operand_elements_are_e4m3_integers_with_small_scale_exponents():
    q, s, val = MX.exact_operand(40, 1280, 3)
    elems = q[:, :1280].view(torch.float8_e4m3fn).float()
    assert bool((elems == elems.round()).all()) and float(elems.abs().max()) == MX.ELEM_MAX
    assert sorted(set((s[:, :40].to(torch.int32) - 127).flatten().tolist())) == list(MX.EXPONENTS)
    assert torch.equal(MX.dequant(q, s, 1280), val)
    for v in range(-MX.ELEM_MAX, MX.ELEM_MAX + 1):                # 3 significant bits: every integer up to 7 (and 8 .. 16 in steps) is e4m3
        assert float(torch.tensor(float(v)).to(torch.float8_e4m3fn).float()) == v


def test_every_product_is_a_multiple_of_a_quarter_below_196():
    vals = sorted({a * 2.0 ** e for a in range(-MX.ELEM_MAX, MX.ELEM_MAX + 1) for e in MX.EXPONENTS})
    prods = {a * b for a, b in itertools.product(vals, vals)}
    assert max(abs(p) for p in prods) == MX.PRODUCT_MAX == 196
    assert all(p / MX.GRID == round(p / MX.GRID) for p in prods)


@pytest.mark.parametrize("K", [1280, 2560])
def test_partial_sums_are_exact_in_fp32_in_any_order(K):
    """|any partial sum| <= K x 196 < 2^24 x 2^-2, all on the 2^-2 grid: representable in fp32, so no order of additions rounds."""
    assert K * MX.PRODUCT_MAX < (1 << 24) * MX.GRID
    _, _, a = MX.exact_operand(8, K, 11)
    _, _, w = MX.exact_operand(16, K, 12)
    ref = a @ w.t()
    # three orders in fp32: straight, reversed, pairwise by blocks of 128 (the matrix instruction's step)
    a32, w32 = a.float(), w.float()
    fwd = torch.zeros((8, 16))
    for k in range(K):
        fwd += a32[:, k:k + 1] * w32[:, k].unsqueeze(0)
    rev = torch.zeros((8, 16))
    for k in reversed(range(K)):
        rev += a32[:, k:k + 1] * w32[:, k].unsqueeze(0)
    blk = (a32.view(8, K // 128, 128).transpose(0, 1) @ w32.view(16, K // 128, 128).permute(1, 2, 0)).sum(0)
    for got in (fwd, rev, blk):
        assert torch.equal(got.double(), ref)
    # ... and the outputs with a bias and a residual on the same grid are exact in fp32 too (rounded once, to fp16)
    assert float(ref.abs().max()) + 2 * 64 < (1 << 24) * MX.GRID


# ------------------------------------------------------------------------------------------------------------------ the shape predicate
FF_SHAPES = [(460800, 2560, 320), (115200, 5120, 640), (28800, 10240, 1280), (460800, 320, 1280), (115200, 640, 2560), (28800, 1280, 5120)]
GEGLU_MX = G.GEMM_BIAS_N | G.GEMM_GEGLU | G.GEMM_MXFP8_OUT
RES = G.GEMM_BIAS_N | G.GEMM_RESIDUAL


@pytest.mark.parametrize("M,N,K", FF_SHAPES)
def test_predicate_accepts_the_feed_forward_shapes(M, N, K):
    L = _lib.lib()
    flags = GEGLU_MX if N > K else RES
    assert L.vcx_gemm_mxfp8_ok(M, N, K, flags) == 1
    assert L.vcx_gemm_mxfp8_ok(2 * M, N, K, flags) == 1                       # two videos in one forward
    if N > K:
        assert L.vcx_gemm_mxfp8_ok(M, N, K, G.GEMM_BIAS_N | G.GEMM_GEGLU) == 1


def test_predicate_refuses_what_the_kernel_cannot_take():
    L = _lib.lib()
    ok = lambda *a: L.vcx_gemm_mxfp8_ok(*a)
    assert ok(300, 320, 48, G.GEMM_BIAS_N) == 0 and b"K % 32" in L.vcx_last_error()
    assert ok(300, 324, 64, G.GEMM_BIAS_N) == 0                               # N % 8
    assert ok(300, 96, 64, GEGLU_MX) == 0 and ok(300, 96, 64, G.GEMM_BIAS_N | G.GEMM_GEGLU) == 0      # N / 2 % 32
    assert ok(300, 128, 64, GEGLU_MX) == 1 and ok(300, 64, 32, GEGLU_MX) == 1
    assert ok(0, 320, 64, G.GEMM_BIAS_N) == 0
    for flags in (0, G.GEMM_RESIDUAL, G.GEMM_BIAS_N | G.GEMM_MXFP8_OUT, RES | G.GEMM_GEGLU, G.GEMM_BIAS_N | G.GEMM_OUT_F32, G.GEMM_BIAS_N | G.GEMM_BIAS_M):
        assert ok(300, 128, 64, flags) == 0 and b"flags" in L.vcx_last_error(), flags
    # extents of 4 GiB or more: the activation bytes (2^22 rows x 1024), the fp16 output (2^21 rows x 1024 columns x 2 bytes)
    assert ok(1 << 22, 64, 1024, G.GEMM_BIAS_N) == 0 and b"4 GiB" in L.vcx_last_error()
    assert ok((1 << 22) - 4096, 64, 1024, G.GEMM_BIAS_N) == 1
    assert ok(1 << 21, 1024, 64, G.GEMM_BIAS_N) == 0 and b"4 GiB" in L.vcx_last_error()
    assert ok(1 << 20, 1024, 64, G.GEMM_BIAS_N) == 1


def test_launcher_validates_before_any_launch():
    """Fake pointers serve: every check sits in front of the first launch (as in tests/test_abi.py)."""
    L = _lib.lib()
    FAKE = 1 << 20
    args = lambda **kw: [kw.get(k, d) for k, d in (("a", FAKE), ("as_", FAKE), ("w", FAKE), ("ws", FAKE), ("out", FAKE), ("os_", None), ("bias", FAKE),
                                                   ("res", None), ("M", 300), ("N", 128), ("K", 64), ("ldc", 128), ("ldr", 0), ("flags", G.GEMM_BIAS_N), ("stream", None))]
    assert L.vcx_gemm_mxfp8(*args(bias=None)) == -1 and b"null" in L.vcx_last_error()
    assert L.vcx_gemm_mxfp8(*args(flags=GEGLU_MX, ldc=64)) == -1 and b"out_scales" in L.vcx_last_error()
    assert L.vcx_gemm_mxfp8(*args(flags=RES)) == -1 and b"residual" in L.vcx_last_error()
    assert L.vcx_gemm_mxfp8(*args(K=48)) == -1 and b"K % 32" in L.vcx_last_error()
    assert L.vcx_gemm_mxfp8(*args(ldc=64)) == -1                               # a row pitch below N
    assert L.vcx_gemm_mxfp8(*args(M=1 << 22, K=1024)) == -1 and b"4 GiB" in L.vcx_last_error()
    assert L.vcx_quant_mxfp8_f16(FAKE, 48, FAKE, FAKE, 4, 48, None) == -1 and b"K % 32" in L.vcx_last_error()
    assert L.vcx_layernorm_mxfp8_f16(FAKE, FAKE, FAKE, FAKE, FAKE, 4, 72, 1e-5, None) == -1 and b"C % 32" in L.vcx_last_error()
