"""The MXFP8 ResBlock convolutions (VCX_RESCONV_MXFP8, include/vcx.h vcx_conv3x3_mxfp8) without a GPU: packing.pack_conv3x3_mxfp8 against
the torch definition slab by slab and tap by tap, the library's shape predicate (which touches no device), the launchers' argument checks,
and the calls ResBlock.forward makes with the switch off, on, refused, mixed and at a skipped width - the `ops` functions replaced by
recording stand-ins."""
import pytest
import torch

from tests import mx_emulation as MX
from viewcrafter_amd import _lib
from viewcrafter_amd.packing import pack_conv3x3_mxfp8

G = _lib


def _weight(cout, cin, seed, spread=4):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((cout, cin, 3, 3), generator=g) * torch.exp2(torch.randint(-spread, spread + 1, (cout, cin // 32, 1, 1), generator=g).float()).repeat_interleave(32, 1)
    return (w * (9 * cin) ** -0.5).half().float()          # fp16 values: a power-of-two multiple of them is exact in fp16 too


def _tap_of(q, s, slab, tap):
    """the 128 element bytes and 4 scale bytes of K-step 9 slab + tap"""
    kt = 9 * slab + tap
    return q[:, kt * 128:(kt + 1) * 128], s[:, kt * 4:(kt + 1) * 4]


# ------------------------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("cout,cin", [(72, 320), (40, 64), (16, 128), (8, 32)])
def test_pack_is_the_emulations_quantisation_of_each_slab_and_tap_on_its_own(cout, cin):
    w = _weight(cout, cin, 10 + cin)
    q, s = pack_conv3x3_mxfp8(w)
    kp = MX.kp_of(cin)
    slabs = kp // 128
    assert q.dtype == s.dtype == torch.uint8 and q.shape == (cout, slabs * 9 * 128) and s.shape == (cout, slabs * 9 * 4)
    assert q.is_contiguous() and s.is_contiguous()
    for tap in range(9):
        qe, se = MX.quant(w[:, :, tap // 3, tap % 3].half().contiguous())          # [cout, kp], [cout, kp / 32]: the tap padded on its own
        for slab in range(slabs):
            qt, st = _tap_of(q, s, slab, tap)
            assert torch.equal(qt, qe[:, slab * 128:(slab + 1) * 128]), f"slab {slab} tap {tap}: element bytes"
            assert torch.equal(st, se[:, slab * 4:(slab + 1) * 4]), f"slab {slab} tap {tap}: scale bytes"
        # the tap's own padding, in its last slab: element bytes 0x00, scale bytes 127
        qt, st = _tap_of(q, s, slabs - 1, tap)
        used = cin - (slabs - 1) * 128
        assert not bool(qt[:, used:].any()) and bool((st[:, used // 32:] == 127).all())
    # the represented values are the fp16 weights to e4m3 precision: half a step of 2^-3 relative to the block maximum's binade
    for tap in range(9):
        qs = torch.cat([_tap_of(q, s, slab, tap)[0] for slab in range(slabs)], dim=1)
        ss = torch.cat([_tap_of(q, s, slab, tap)[1] for slab in range(slabs)], dim=1)
        dq = MX.dequant(qs, ss, cin)
        ref = w[:, :, tap // 3, tap % 3].half().double()
        amax = ref.view(cout, cin // 32, 32).abs().amax(dim=2, keepdim=True)
        assert bool(((dq - ref).view(cout, cin // 32, 32).abs() <= amax * 2.0 ** -3).all())


@pytest.mark.parametrize("loud", [0, 4, 8])
def test_one_loud_tap_does_not_move_the_scales_of_its_neighbours(loud):
    """One tap 2^6 louder than the others: were a block (or its maximum) to span two taps, the scale bytes of a quiet tap would move."""
    cout, cin = 24, 320
    w = _weight(cout, cin, 77, spread=0)
    quiet = pack_conv3x3_mxfp8(w)
    w2 = w.clone()
    w2[:, :, loud // 3, loud % 3] *= 64.0
    q, s = pack_conv3x3_mxfp8(w2)
    slabs = MX.kp_of(cin) // 128
    for slab in range(slabs):
        used = min(128, cin - slab * 128) // 32
        for tap in range(9):
            (qt, st), (q0, s0) = _tap_of(q, s, slab, tap), _tap_of(*quiet, slab, tap)
            assert torch.equal(qt, q0)
            if tap == loud:
                assert torch.equal(st[:, :used], s0[:, :used] + 6)          # exactly six binades up, same elements
                assert torch.equal(st[:, used:], s0[:, used:])              # its padding stays 127
            else:
                assert torch.equal(st, s0), f"the scale bytes of tap {tap} moved with tap {loud}"


def test_pack_rejects_other_weights():
    with pytest.raises(ValueError):
        pack_conv3x3_mxfp8(torch.zeros(8, 48, 3, 3))
    with pytest.raises(ValueError):
        pack_conv3x3_mxfp8(torch.zeros(8, 64, 1, 1))
    with pytest.raises(ValueError):
        pack_conv3x3_mxfp8(torch.zeros(8, 64, 3, 1, 1))
    with pytest.raises(ValueError):
        pack_conv3x3_mxfp8(torch.zeros(8, 64 * 9))


# ------------------------------------------------------------------------------------------------------------------ the shape predicate
BIAS = G.GEMM_BIAS_N
ROW, RES, CS = BIAS | G.GEMM_ROWADD, BIAS | G.GEMM_RESIDUAL, BIAS | G.GEMM_COLSTATS


def _ok(n, H, W, cin, N, flags=BIAS, ldc=None, ldr=None, ldcs=None, col=0, div=1):
    return _lib.lib().vcx_conv3x3_mxfp8_ok(n, H, W, cin, N, N if ldc is None else ldc, N if ldr is None else ldr, N if ldcs is None else ldcs, col, div, flags)


@pytest.mark.parametrize("cin", [320, 640, 960, 1280, 1920, 2560])
@pytest.mark.parametrize("H,W,N", [(72, 128, 320), (36, 64, 640), (18, 32, 1280), (9, 16, 1280)])
def test_predicate_accepts_the_resblock_convolutions_of_576x1024x25(H, W, N, cin):
    for B in (1, 2):
        n = 25 * B
        cs = G.GEMM_COLSTATS if (H * W) % 64 == 0 else 0
        assert _ok(n, H, W, cin, N, ROW | cs, div=25 * H * W) == 1, _lib.lib().vcx_last_error()          # conv1: embedding, moments
        assert _ok(n, H, W, N, N, RES) == 1 and _ok(n, H, W, N, N, RES | cs, ldc=2 * N, ldcs=2 * N) == 1      # conv2: residual, concat target
        assert _ok(n, H, W, cin, N, ROW | RES | cs, div=25 * H * W) == 1


def test_predicate_refuses_what_the_kernel_cannot_take():
    L = _lib.lib()
    assert _ok(2, 5, 8, 48, 64) == 0 and b"Cin % 32" in L.vcx_last_error()
    assert _ok(2, 5, 8, 64, 12) == 0 and b"N % 8" in L.vcx_last_error()
    assert _ok(0, 5, 8, 64, 64) == 0 and _ok(2, 0, 8, 64, 64) == 0 and _ok(2, 5, 0, 64, 64) == 0
    for flags in (0, G.GEMM_RESIDUAL, G.GEMM_ROWADD, BIAS | G.GEMM_GEGLU, BIAS | G.GEMM_MXFP8_OUT, BIAS | G.GEMM_OUT_F32, BIAS | G.GEMM_BIAS_M, BIAS | (1 << 30)):
        assert _ok(2, 5, 8, 64, 64, flags) == 0 and b"flags" in L.vcx_last_error(), flags
    # the row-indexed addend
    assert _ok(2, 5, 8, 64, 64, ROW, div=0) == 0 and b"rowadd_div" in L.vcx_last_error()
    assert _ok(2, 5, 8, 64, 64, ROW, div=-3) == 0
    assert _ok(2, 5, 8, 64, 64, ROW, div=40) == 1 and _ok(2, 5, 8, 64, 64, ROW, div=7) == 1
    assert _ok(2, 5, 8, 64, 64, div=0) == 1                                     # ignored without the flag
    # pitches and alignment
    assert _ok(2, 5, 8, 64, 64, ldc=56) == 0 and b"ldc" in L.vcx_last_error()
    assert _ok(2, 5, 8, 64, 64, ldc=68) == 0 and _ok(2, 5, 8, 64, 64, ldc=88) == 1
    assert _ok(2, 5, 8, 64, 64, RES, ldr=60) == 0 and b"ldr" in L.vcx_last_error()
    assert _ok(2, 5, 8, 64, 64, ldr=60) == 1                                   # ignored without the flag
    # column moments: whole 64-row strips, room for the columns, 16-byte aligned pairs
    assert _ok(2, 5, 8, 64, 64, CS) == 0 and b"COLSTATS" in L.vcx_last_error()            # 80 rows
    assert _ok(2, 8, 8, 64, 64, CS) == 1 and _ok(2, 8, 8, 64, 64, CS, ldcs=160, col=96) == 1
    assert _ok(2, 8, 8, 64, 64, CS, ldcs=161) == 0 and b"COLSTATS" in L.vcx_last_error()  # odd ldcs
    assert _ok(2, 8, 8, 64, 64, CS, ldcs=160, col=100) == 0 and _ok(2, 8, 8, 64, 64, CS, ldcs=160, col=3) == 0
    # 32-bit extents: (M + 127 + W + 1) Kp for the activation - a tile reaches 127 rows past M and the farthest tap W + 1 rows further
    W, kp = 1024, 1280
    Hmax = (0xFFFF0000 // kp - 128 - W - 1) // W + 1
    while (Hmax * W + 127 + W + 1) * kp >= 0xFFFF0000:
        Hmax -= 1                                                              # the largest H with (H W + 127 + W + 1) Kp < lim
    assert _ok(1, Hmax, W, kp, 64) == 1 and _ok(1, Hmax + 1, W, kp, 64) == 0 and b"4 GiB" in L.vcx_last_error()
    assert (Hmax + 1) * W * kp < 0xFFFF0000, "refused for the reach of the tile grid and the tap, not for M Kp"
    assert _ok(1, 1 << 11, 1 << 10, 64, 1024) == 0 and b"4 GiB" in L.vcx_last_error()      # the fp16 output
    assert _ok(1, 8, 8, 1 << 20, 1024) == 0 and b"4 GiB" in L.vcx_last_error()             # the weight: (N + 127) 9 Kp
    assert _ok(1 << 20, 1 << 10, 4, 64, 64) == 0 and b"2^31" in L.vcx_last_error()         # n H W past 2^31
    assert _ok(2, 5, 8, 64, 64, ROW, div=1 << 31) == 0 and b"2^31" in L.vcx_last_error()


def test_launchers_validate_before_any_launch():
    L = _lib.lib()
    FAKE = 1 << 20
    args = lambda **kw: [kw.get(k, d) for k, d in (("a", FAKE), ("as_", FAKE), ("w", FAKE), ("ws", FAKE), ("out", FAKE), ("bias", FAKE), ("rowadd", None), ("res", None),
                                                   ("cs", None), ("n", 2), ("H", 8), ("W", 8), ("cin", 64), ("N", 64), ("ldc", 64), ("ldr", 0), ("ldcs", 0),
                                                   ("rld", 0), ("div", 0), ("flags", BIAS), ("stream", None))]
    assert L.vcx_conv3x3_mxfp8(*args(bias=None)) == -1 and b"null" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(a=None)) == -1 and b"null" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(flags=ROW, rld=64, div=64)) == -1 and b"rowadd" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(flags=RES, ldr=64)) == -1 and b"residual" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(flags=CS, ldcs=64)) == -1 and b"colstats" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(cin=48)) == -1 and b"Cin % 32" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(ldc=56)) == -1
    assert L.vcx_conv3x3_mxfp8(*args(flags=ROW, rowadd=FAKE, rld=64, div=0)) == -1 and b"rowadd_div" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(flags=ROW, rowadd=FAKE, rld=60, div=64)) == -1 and b"rowadd_ld" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(flags=ROW, rowadd=FAKE + 4, rld=64, div=64)) == -1 and b"aligned" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(a=FAKE + 8)) == -1 and b"aligned" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(as_=FAKE + 2)) == -1 and b"aligned" in L.vcx_last_error()
    assert L.vcx_conv3x3_mxfp8(*args(flags=CS, cs=FAKE + 8, ldcs=64)) == -1 and b"aligned" in L.vcx_last_error()
    gn2 = lambda **kw: [kw.get(k, d) for k, d in (("x1", FAKE), ("c1", 32), ("x2", FAKE), ("q", FAKE), ("s", FAKE), ("stats", FAKE), ("g", FAKE), ("b", FAKE), ("n", 1),
                                                  ("pix", 64), ("C", 64), ("groups", 32), ("eps", 1e-5), ("silu", 1), ("stream", None))]
    assert L.vcx_groupnorm_apply2_mxfp8_f16(*gn2(x2=None)) == -1 and b"x2" in L.vcx_last_error()
    assert L.vcx_groupnorm_apply2_mxfp8_f16(*gn2(c1=12)) == -1 and b"c1 % 8" in L.vcx_last_error()
    assert L.vcx_groupnorm_apply2_mxfp8_f16(*gn2(c1=64)) == -1
    assert L.vcx_groupnorm_apply2_mxfp8_f16(*gn2(c1=40, C=72, groups=8)) == -1 and b"C % 32" in L.vcx_last_error()
    assert L.vcx_groupnorm_apply2_mxfp8_f16(*gn2(s=None)) == -1 and b"null" in L.vcx_last_error()
    assert L.vcx_groupnorm_apply2_mxfp8_f16(*gn2(x2=FAKE + 8)) == -1


# ------------------------------------------------------------------------------------------------------------------ host graph
class _Recorder:
    """Stand-ins for the ops a ResBlock calls: they record (name, what matters of the arguments) and return tensors of the right shape.
    `accept(kw)` is the stand-in predicate's answer for a query with the keywords kw."""

    NAMES = ("group_norm", "group_norm_mxfp8", "conv2d", "conv3x3_mxfp8", "conv3x3_mxfp8_ok", "colstats_ok", "colstats_buffer", "group_norm_stats_from_colstats",
             "conv_tail_ok", "concat_channels", "linear", "avgpool2x2", "upsample2x", "tune_get")

    def __init__(self, monkeypatch, accept=lambda kw: True, tail_ok=True):
        from viewcrafter_amd import ops
        self.calls, self.accept, self.tail_ok = [], accept, tail_ok
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, getattr(self, name))

    def names(self, skip=("ok",)):
        return [c[0] for c in self.calls if c[0] not in skip]

    def of(self, name):
        return [c for c in self.calls if c[0] == name]

    def tune_get(self, name):
        return 1

    def colstats_ok(self, M, pixels, cin, cout, in_rows=None):
        return pixels % 64 == 0 and M % 64 == 0

    def conv_tail_ok(self, M, cin, cout, taps, tail_ks, in_rows=None):
        return self.tail_ok

    def colstats_buffer(self, M, cout, device):
        return torch.zeros((M // 64, cout, 2))

    def group_norm_stats_from_colstats(self, colstats, n_outer, pixels, C, groups=32):
        self.calls.append(("stats_from_colstats", id(colstats), C))
        return torch.zeros((n_outer, groups, 2))

    def linear(self, x, w, bias=None, **kw):
        self.calls.append(("linear",))
        return torch.zeros((x.shape[0], w.shape[0]))

    def concat_channels(self, a, b):
        self.calls.append(("concat_channels",))
        return torch.zeros((a.shape[0], a.shape[1] + b.shape[1]), dtype=torch.float16)

    def avgpool2x2(self, x):
        self.calls.append(("avgpool2x2",))
        return torch.zeros((x.shape[0], x.shape[1] // 2, x.shape[2] // 2, x.shape[3]), dtype=torch.float16)

    def upsample2x(self, x):
        self.calls.append(("upsample2x",))
        return torch.zeros((x.shape[0], x.shape[1] * 2, x.shape[2] * 2, x.shape[3]), dtype=torch.float16)

    def group_norm(self, x, gamma, beta, eps, silu, groups=32, out=None, stats=None, x2=None):
        self.calls.append(("group_norm", tuple(x.shape), silu, stats is not None, x2 is not None))
        C = x.shape[2] + (0 if x2 is None else x2.shape[2])
        return torch.zeros((x.shape[0], x.shape[1], C), dtype=torch.float16)

    def group_norm_mxfp8(self, x, gamma, beta, eps, silu, groups=32, stats=None, x2=None):
        self.calls.append(("group_norm_mxfp8", tuple(x.shape), silu, stats is not None, x2 is not None))
        C = x.shape[2] + (0 if x2 is None else x2.shape[2])
        rows, kp = x.shape[0] * x.shape[1], MX.kp_of(C)
        return torch.zeros((rows, kp), dtype=torch.uint8), torch.zeros((rows, kp // 32), dtype=torch.uint8)

    def conv2d(self, x, w, bias, *, kh, kw, ups=0, **kwargs):
        n, H, W, _ = x.shape
        H, W = H << ups, W << ups
        self.calls.append(("conv2d", kh, sorted(k for k in kwargs if kwargs[k] is not None), len(kwargs.get("tail") or ())))
        out = kwargs.get("out")
        return (torch.zeros((n * H * W, w.shape[0]), dtype=torch.float16) if out is None else out).view(n, H, W, -1)

    def conv3x3_mxfp8_ok(self, n, H, W, cin, cout, **kw):
        self.calls.append(("ok", n, cin, cout, dict(kw)))
        return self.accept(kw)

    def conv3x3_mxfp8(self, a, w, bias, *, n, H, W, cin, **kw):
        kp = MX.kp_of(cin)
        assert a[0].shape == (n * H * W, kp) and w[0].shape == (bias.numel(), 9 * kp) and w[1].shape == (bias.numel(), 9 * kp // 32)
        self.calls.append(("conv3x3_mxfp8", sorted(k for k in kw if kw[k] is not None), kw))
        out = kw.get("out")
        return (torch.zeros((n * H * W, bias.numel()), dtype=torch.float16) if out is None else out).view(n, H, W, -1)


N_FRAMES, HH, WW, EMB = 4, 8, 8, 32            # two videos of two frames, 64 pixels per frame (whole moment strips)


def _block(cin=64, cout=None, **kw):
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    torch.manual_seed(cin)
    return U, U.ResBlock(cin, EMB, 0.0, out_channels=cout, **kw).eval()


def _switch(monkeypatch, U, keep_fold=True, skip=()):
    monkeypatch.setattr(U, "RESCONV_MXFP8", True)
    monkeypatch.setattr(U, "RESCONV_MXFP8_SKIP_DIMS", frozenset(skip))
    monkeypatch.setattr(U, "RESCONV_MXFP8_KEEP_FOLD", keep_fold)


def _run(blk, c=64, **kw):
    x = torch.zeros((N_FRAMES, HH, WW, c), dtype=torch.float16)
    emb = torch.zeros((2, EMB), dtype=torch.float16)
    with torch.no_grad():
        return blk(x, emb, batch_size=2, **kw)


FP16_IDENTITY = ["group_norm", "linear", "conv2d", "stats_from_colstats", "group_norm", "conv2d"]
MX_IDENTITY = ["group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm_mxfp8", "conv3x3_mxfp8"]


def test_switch_off_makes_the_calls_it_makes_today_and_no_mx_op(monkeypatch):
    U, blk = _block()
    assert U.RESCONV_MXFP8 is False, "the switch is off by default"
    rec = _Recorder(monkeypatch)
    h, cs = _run(blk, want_colstats=True)
    assert rec.names(skip=()) == FP16_IDENTITY
    convs = rec.of("conv2d")
    assert convs[0][2] == ["colstats", "rowadd", "rowadd_div"] and convs[1][2] == ["colstats", "residual"]
    assert [c[3] for c in rec.of("group_norm")] == [False, True]
    assert h.shape == (N_FRAMES, HH, WW, 64) and cs is not None and blk._mx == {}
    # ... and a block with a skip convolution: folded into the second convolution as a K tail
    U, blk = _block(64, 128)
    rec = _Recorder(monkeypatch)
    _run(blk)
    assert rec.names(skip=()) == FP16_IDENTITY and rec.of("conv2d")[1][2:] == (["tail"], 1) and blk._mx == {}


@pytest.mark.parametrize("want", [False, True])
def test_switch_on_identity_block_runs_two_quantising_norms_and_two_mx_convolutions(monkeypatch, want):
    U, blk = _block()
    _switch(monkeypatch, U)
    rec = _Recorder(monkeypatch)
    h, cs = _run(blk, want_colstats=want)
    asked = rec.of("ok")
    assert [c[1] for c in asked] == [2, 4, 2, 4], "each convolution is asked about for one video's frames and for the call's"
    assert all(c[4]["rowadd"] and c[4]["rowadd_div"] == 2 * 64 and c[4]["colstats"] for c in asked[:2])
    assert all(c[4]["residual"] and c[4]["colstats"] == want for c in asked[2:])
    assert rec.names() == MX_IDENTITY
    assert rec.names(skip=()).index("group_norm_mxfp8") > max(i for i, n in enumerate(rec.names(skip=())) if n == "ok"), "the route is decided before anything runs"
    c1, c2 = rec.of("conv3x3_mxfp8")
    assert c1[1] == ["colstats", "rowadd", "rowadd_div"] and c1[2]["rowadd_div"] == 2 * 64
    assert c2[1] == (["colstats", "residual"] if want else ["residual"]) and tuple(c2[2]["residual"].shape) == (N_FRAMES * 64, 64)
    norms = rec.of("group_norm_mxfp8")
    assert all(c[1] == (N_FRAMES, 64, 64) and c[2] is True for c in norms) and [c[3] for c in norms] == [False, True]
    assert h.shape == (N_FRAMES, HH, WW, 64) and (cs is not None) == want
    assert sorted(blk._mx) == ["w1", "w2"] and all(q.dtype == torch.uint8 and q.shape == (64, 9 * 128) and s.shape == (64, 36) for q, s in blk._mx.values())
    first = dict(blk._mx)
    _run(blk)
    assert all(blk._mx[k] is first[k] for k in first), "the packs are built once"
    blk.load_state_dict(blk.state_dict())
    assert blk._mx == {}, "loading a state dict drops the MX packs with the fp16 pack"


@pytest.mark.parametrize("keep_fold", [True, False])
def test_switch_on_skip_conv_block_under_both_policies(monkeypatch, keep_fold):
    U, blk = _block(64, 128)
    _switch(monkeypatch, U, keep_fold=keep_fold)
    rec = _Recorder(monkeypatch)
    h, _ = _run(blk)
    if keep_fold:      # (b): only the first convolution is MX, the second keeps the folded K tail
        assert rec.names() == ["group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm", "conv2d"]
        assert rec.of("conv2d")[0][1:] == (3, ["tail"], 1) and sorted(blk._mx) == ["w1"]
        assert len(rec.of("ok")) == 2, "the second convolution is not asked about"
    else:              # (a): both MX, the fp16 1x1 skip convolution's result is the residual
        assert rec.names() == ["group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm_mxfp8", "conv2d", "conv3x3_mxfp8"]
        assert rec.of("conv2d")[0][1:] == (1, [], 0) and rec.of("conv3x3_mxfp8")[1][1] == ["residual"] and sorted(blk._mx) == ["w1", "w2"]
        assert rec.of("ok")[2][4]["ldr"] == 128
    assert h.shape == (N_FRAMES, HH, WW, 128)


@pytest.mark.parametrize("keep_fold", [True, False])
def test_split_concat_is_read_in_place_by_the_quantising_norm(monkeypatch, keep_fold):
    U, blk = _block(128, 64)
    _switch(monkeypatch, U, keep_fold=keep_fold)
    rec = _Recorder(monkeypatch)
    x2 = torch.zeros((N_FRAMES, HH, WW, 64), dtype=torch.float16)
    colstats = torch.zeros((N_FRAMES * 64 // 64, 128, 2))
    h, _ = _run(blk, x2=x2, colstats=colstats)
    assert "concat_channels" not in rec.names()
    assert rec.names() == ["stats_from_colstats", "group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm", "conv2d"]
    assert rec.of("group_norm_mxfp8")[0][1:] == ((N_FRAMES, 64, 64), True, True, True), "the left half, with statistics and x2"
    assert rec.of("ok")[0][2] == 128 and rec.of("conv3x3_mxfp8")[0][2]["rowadd"] is not None
    assert rec.of("conv2d")[0][1:] == (3, ["tail"], 2), "the skip convolution reads both halves as the K tail of the fp16 second convolution"
    assert h.shape == (N_FRAMES, HH, WW, 64)


def test_split_concat_without_moments_is_materialised(monkeypatch):
    U, blk = _block(128, 64)
    _switch(monkeypatch, U)
    rec = _Recorder(monkeypatch)
    x2 = torch.zeros((N_FRAMES, HH, WW, 64), dtype=torch.float16)
    _run(blk, x2=x2)
    assert rec.names()[:2] == ["concat_channels", "group_norm_mxfp8"]
    assert rec.of("group_norm_mxfp8")[0][1:] == ((N_FRAMES, 64, 128), True, False, False)
    assert rec.of("conv2d")[-1][1:] == (3, ["tail"], 1)


@pytest.mark.parametrize("why", ["up", "down", "scale_shift", "skipped", "refused", "cin"])
def test_blocks_that_stay_on_fp16_make_the_calls_they_make_with_the_switch_off(monkeypatch, why):
    kw = dict(up=dict(up=True), down=dict(down=True), scale_shift=dict(use_scale_shift_norm=True)).get(why, {})
    cin = 48 if why == "cin" else 64           # (GroupNorm(32) wants cin % 32 == 0 for its groups; 48 % 32 != 0 would need 16 groups:
    if why == "cin":                           #  the rule is checked on the decision function directly)
        U, blk = _block(64)
        _switch(monkeypatch, U)
        rec = _Recorder(monkeypatch)
        x = torch.zeros((N_FRAMES, HH, WW, 48), dtype=torch.float16)
        plan = blk._plan(x, torch.zeros((2, EMB), dtype=torch.float16), 2, False, None, None, None)
        assert (plan.conv1, plan.conv2) == ("fp16", "fp16") and rec.calls == []
        return
    U, blk = _block(cin, **kw)
    rec = _Recorder(monkeypatch, accept=lambda q: False)
    off = _run(blk, want_colstats=True)
    off_calls = rec.names(skip=())
    _switch(monkeypatch, U, skip=[64] if why == "skipped" else [])
    rec = _Recorder(monkeypatch, accept=lambda q: False)
    on = _run(blk, want_colstats=True)
    assert rec.names() == off_calls and not any("mxfp8" in n for n in rec.names())
    assert ("ok" in rec.names(skip=())) == (why == "refused")
    assert blk._mx == {}, "no MX pack is built"
    assert on[0].shape == off[0].shape and (on[1] is None) == (off[1] is None)


@pytest.mark.parametrize("which", ["conv1", "conv2"])
def test_one_refused_convolution_gives_the_mixed_route(monkeypatch, which):
    U, blk = _block()
    _switch(monkeypatch, U)
    rec = _Recorder(monkeypatch, accept=(lambda q: bool(q.get("rowadd"))) if which == "conv1" else (lambda q: bool(q.get("residual"))))
    h, cs = _run(blk, want_colstats=True)
    if which == "conv1":
        assert rec.names() == ["group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm", "conv2d"]
        assert rec.of("conv2d")[0][2] == ["colstats", "residual"] and sorted(blk._mx) == ["w1"]
    else:
        assert rec.names() == ["group_norm", "linear", "conv2d", "stats_from_colstats", "group_norm_mxfp8", "conv3x3_mxfp8"]
        assert rec.of("conv2d")[0][2] == ["colstats", "rowadd", "rowadd_div"] and sorted(blk._mx) == ["w2"]
    assert h.shape == (N_FRAMES, HH, WW, 64) and cs is not None


def test_concat_target_and_moments_keywords_arrive_at_the_second_convolution(monkeypatch):
    from viewcrafter_amd.lvdm.modules.flow import CatTarget
    U, blk = _block()
    _switch(monkeypatch, U)
    rec = _Recorder(monkeypatch)
    M = N_FRAMES * 64
    target = CatTarget(M, 64, 32, "cpu", with_moments=True)
    h, cs = _run(blk, target=target)
    last = rec.of("ok")[-1][4]
    assert last["ldc"] == 96 and last["colstats_ld"] == 96 and last["colstats"] is True, "the predicate sees the concat buffer's pitches"
    conv = rec.of("conv3x3_mxfp8")[-1]
    assert conv[1] == ["colstats", "colstats_col", "colstats_ld", "ldc", "out", "residual"] and conv[2]["colstats_col"] == 0 and conv[2]["out"] is target.data
    assert cs is target.moments and h.shape == (N_FRAMES, HH, WW, 96)
    rec = _Recorder(monkeypatch)
    h, cs = _run(blk, want_colstats=True)
    conv = rec.of("conv3x3_mxfp8")[-1]
    assert conv[1] == ["colstats", "residual"] and cs is conv[2]["colstats"]


def test_the_real_predicate_decides_per_convolution():
    from viewcrafter_amd import ops
    assert ops.conv3x3_mxfp8_ok(4, 8, 8, 64, 64, rowadd=True, rowadd_div=128, colstats=True) is True
    assert ops.conv3x3_mxfp8_ok(4, 5, 8, 64, 64, rowadd=True, rowadd_div=80, colstats=True) is False and b"COLSTATS" in _lib.lib().vcx_last_error()
    assert ops.conv3x3_mxfp8_ok(4, 8, 8, 64, 64, residual=True, ldc=96, colstats=True, colstats_ld=96) is True
    assert ops.conv3x3_mxfp8_ok(4, 8, 8, 64, 64, rowadd=True, rowadd_div=0) is False
    assert ops.conv3x3_mxfp8_ok(1, 1 << 13, 1 << 13, 64, 64) is False and b"4 GiB" in _lib.lib().vcx_last_error()
