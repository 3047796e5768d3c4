"""The ResBlock skip convolution as a K tail of the MXFP8 3x3 convolution (VCX_RESCONV_MXFP8_TAIL; include/vcx.h vcx_conv3x3_tail_mxfp8,
vcx_groupnorm_apply(2)_mxfp8_raw_f16) without a GPU: packing.pack_conv3x3_tail_mxfp8 against its two parts, the library's shape predicate
(which touches no device), the launchers' argument checks, the bindings, and the calls ResBlock.forward makes with the new switch off
(the parent's, call for call) and on - the `ops` functions replaced by recording stand-ins."""
import re

import pytest
import torch

from tests import mx_emulation as MX
from tests.test_mxfp8_resconv_cpu import EMB, HH, N_FRAMES, WW, _block, _Recorder, _run, _switch
from viewcrafter_amd import _lib

G = _lib
BIAS = G.GEMM_BIAS_N
CS = BIAS | G.GEMM_COLSTATS
LIM = 0xFFFF0000


# ------------------------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("cout,cin,ct", [(72, 320, 960), (24, 32, 160), (16, 128, 96), (8, 64, 32)])
def test_pack_is_the_3x3_pack_followed_by_the_quantised_1x1_weight(cout, cin, ct):
    from viewcrafter_amd.packing import pack_conv3x3_mxfp8, pack_conv3x3_tail_mxfp8
    g = torch.Generator().manual_seed(cout + cin + ct)
    w3 = (torch.randn((cout, cin, 3, 3), generator=g) * (9 * cin) ** -0.5).half().float()
    w1 = torch.randn((cout, ct, 1, 1), generator=g) * torch.exp2(torch.randint(-4, 5, (cout, ct // 32, 1, 1), generator=g).float()).repeat_interleave(32, 1)
    w1 = (w1 * ct ** -0.5).half().float()
    q, s = pack_conv3x3_tail_mxfp8(w3, w1)
    kp, kpt = MX.kp_of(cin), MX.kp_of(ct)
    assert q.dtype == s.dtype == torch.uint8 and q.shape == (cout, 9 * kp + kpt) and s.shape == (cout, (9 * kp + kpt) // 32)
    assert q.is_contiguous() and s.is_contiguous()
    qm, sm = pack_conv3x3_mxfp8(w3)
    assert torch.equal(q[:, :9 * kp], qm) and torch.equal(s[:, :9 * kp // 32], sm), "the main columns are pack_conv3x3_mxfp8's"
    qt, st = MX.quant(w1.view(cout, ct).half().contiguous())
    assert torch.equal(q[:, 9 * kp:], qt) and torch.equal(s[:, 9 * kp // 32:], st), "the tail columns are the emulation's quantisation of the 1x1 weight"
    # each part padded on its own: the tail's padding is its own last bytes, the main part's padding sits inside its last slab
    assert not bool(q[:, 9 * kp + ct:].any()) and bool((s[:, (9 * kp + ct) // 32:] == 127).all())
    # a loud tail does not move a scale byte of the main part, and the other way round
    q2, s2 = pack_conv3x3_tail_mxfp8(w3, w1 * 64.0)
    assert torch.equal(s2[:, :9 * kp // 32], sm) and torch.equal(q2, q) and torch.equal(s2[:, 9 * kp // 32:(9 * kp + ct) // 32], st[:, :ct // 32] + 6)


def test_pack_rejects_other_weights():
    from viewcrafter_amd.packing import pack_conv3x3_tail_mxfp8
    ok3, ok1 = torch.zeros(8, 64, 3, 3), torch.zeros(8, 96, 1, 1)
    pack_conv3x3_tail_mxfp8(ok3, ok1)
    for w3, w1 in ((ok3, torch.zeros(8, 48, 1, 1)), (ok3, torch.zeros(8, 96, 3, 3)), (ok3, torch.zeros(8, 96)), (ok3, torch.zeros(16, 96, 1, 1)),
                   (torch.zeros(8, 48, 3, 3), ok1), (torch.zeros(8, 64, 1, 1), ok1), (torch.zeros(8, 64 * 9), ok1)):
        with pytest.raises(ValueError):
            pack_conv3x3_tail_mxfp8(w3, w1)


# ------------------------------------------------------------------------------------------------------------------ the shape predicate
def _ok(n, H, W, cin, ct, N, flags=BIAS, ldc=None, ldcs=None, col=0):
    return _lib.lib().vcx_conv3x3_tail_mxfp8_ok(n, H, W, cin, ct, N, N if ldc is None else ldc, N if ldcs is None else ldcs, col, flags)


# (H, W, c1, c2, cout) of the fourteen ResBlocks with a skip convolution at 576x1024x25: the two channel-changing blocks of the down path
# (c2 = 0), the twelve split-concat blocks of the up path
SKIP_BLOCKS = [(36, 64, 320, 0, 640), (18, 32, 640, 0, 1280),
               (9, 16, 1280, 1280, 1280), (9, 16, 1280, 1280, 1280), (9, 16, 1280, 1280, 1280),
               (18, 32, 1280, 1280, 1280), (18, 32, 1280, 1280, 1280), (18, 32, 1280, 640, 1280),
               (36, 64, 1280, 640, 640), (36, 64, 640, 640, 640), (36, 64, 640, 320, 640),
               (72, 128, 640, 320, 320), (72, 128, 320, 320, 320), (72, 128, 320, 320, 320)]


@pytest.mark.parametrize("H,W,c1,c2,cout", SKIP_BLOCKS)
def test_predicate_accepts_the_skip_conv_blocks_of_576x1024x25(H, W, c1, c2, cout):
    assert len(SKIP_BLOCKS) == 14
    from viewcrafter_amd import ops
    for n in (25, 50):          # one video's frames, the CFG batch
        cs = G.GEMM_COLSTATS if (H * W) % 64 == 0 else 0
        assert _ok(n, H, W, cout, c1 + c2, cout) == 1, _lib.lib().vcx_last_error()
        assert _ok(n, H, W, cout, c1 + c2, cout, BIAS | cs, ldc=2 * cout, ldcs=2 * cout) == 1, _lib.lib().vcx_last_error()      # concat target, moments
        assert ops.conv3x3_tail_mxfp8_ok(n, H, W, cout, c1 + c2, cout, ldc=2 * cout, colstats=bool(cs), colstats_ld=2 * cout) is True


def test_predicate_refuses_what_the_kernel_cannot_take():
    from viewcrafter_amd import ops
    L = _lib.lib()
    assert _ok(2, 8, 8, 64, 96, 64) == 1
    assert _ok(2, 8, 8, 64, 48, 64) == 0 and b"Ct" in L.vcx_last_error()
    assert _ok(2, 8, 8, 64, 0, 64) == 0 and _ok(2, 8, 8, 48, 96, 64) == 0 and b"Cin % 32" in L.vcx_last_error()
    assert _ok(2, 8, 8, 64, 96, 12) == 0 and b"N % 8" in L.vcx_last_error()
    # a residual, a row addend, a missing bias, anything else: refused on the tailed form
    for flags in (0, G.GEMM_COLSTATS, BIAS | G.GEMM_RESIDUAL, BIAS | G.GEMM_ROWADD, CS | G.GEMM_RESIDUAL, BIAS | G.GEMM_GEGLU, BIAS | G.GEMM_MXFP8_OUT, BIAS | (1 << 30)):
        assert _ok(2, 8, 8, 64, 96, 64, flags) == 0 and b"flags" in L.vcx_last_error(), flags
    assert ops.conv3x3_tail_mxfp8_ok(2, 8, 8, 64, 96, 64) is True
    assert ops.conv3x3_tail_mxfp8_ok(2, 8, 8, 64, 96, 64, residual=True) is False and ops.conv3x3_tail_mxfp8_ok(2, 8, 8, 64, 96, 64, rowadd=True) is False
    assert ops.conv3x3_tail_mxfp8_ok(2, 8, 8, 64, 96, 64, bias=False) is False and b"flags" in L.vcx_last_error()
    # pitches and the moments' alignment
    assert _ok(2, 8, 8, 64, 96, 64, ldc=56) == 0 and b"ldc" in L.vcx_last_error()
    assert _ok(2, 8, 8, 64, 96, 64, ldc=68) == 0 and _ok(2, 8, 8, 64, 96, 64, ldc=88) == 1
    assert _ok(2, 5, 8, 64, 96, 64, CS) == 0 and b"COLSTATS" in L.vcx_last_error()            # 80 rows: no whole strips
    assert _ok(2, 8, 8, 64, 96, 64, CS) == 1 and _ok(2, 8, 8, 64, 96, 64, CS, ldcs=160, col=96) == 1
    assert _ok(2, 8, 8, 64, 96, 64, CS, ldcs=161) == 0 and b"COLSTATS" in L.vcx_last_error()
    assert _ok(2, 8, 8, 64, 96, 64, CS, ldcs=160, col=3) == 0 and _ok(2, 8, 8, 64, 96, 64, CS, ldcs=160, col=100) == 0
    assert _ok(2, 8, 8, 64, 96, 64, ldcs=161, col=3) == 1                                     # ignored without the flag
    assert _ok(1 << 20, 1 << 10, 4, 64, 96, 64) == 0 and b"2^31" in L.vcx_last_error()
    assert _ok(2, 8, 8, 64, 1 << 31, 64) == 0


def _largest(pred, lo, hi):
    """the largest v in [lo, hi) with pred(v), pred being true up to some point and false from there on"""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


def test_each_32_bit_extent_is_refused_one_step_past_its_limit():
    """(M + 127 + W + 1) Kp(Cin) for the gathered source, (M + 127) Kp(Ct) for the tail, (N + 127) (9 Kp(Cin) + Kp(Ct)) for the weight: each on
    its own, the other two far below the limit.  The limit is the launchers' 0xFFFF0000 (32-bit buffer offsets)."""
    L = _lib.lib()
    W = 1024
    # the gathered source: Kp(Cin) = 1280, a 32-channel tail, eight output columns
    H = _largest(lambda h: _ok(1, h, W, 1280, 32, 8) == 1, 1, 1 << 13)
    assert (H * W + 127 + W + 1) * 1280 < LIM <= ((H + 1) * W + 127 + W + 1) * 1280
    assert _ok(1, H + 1, W, 1280, 32, 8) == 0 and b"4 GiB" in L.vcx_last_error()
    assert ((H + 1) * W + 127) * 128 < LIM and (8 + 127) * (9 * 1280 + 128) < LIM
    # the tail: Kp(Ct) = 1280 behind a 32-channel convolution - the step past the limit is also past 2^32 once the 127 rows are counted
    H = _largest(lambda h: _ok(1, h, W, 32, 1280, 8) == 1, 1, 1 << 13)
    assert (H * W + 127) * 1280 < LIM <= ((H + 1) * W + 127) * 1280
    assert _ok(1, H + 1, W, 32, 1280, 8) == 0 and b"4 GiB" in L.vcx_last_error() and b"tail" in L.vcx_last_error()
    assert ((H + 1) * W + 127 + W + 1) * 128 < LIM
    # the weight: rows of 9 x 128 + 2^20 bytes
    kpt = 1 << 20
    N = _largest(lambda k: _ok(1, 8, 8, 32, kpt, 8 * k) == 1, 1, 1 << 12) * 8
    assert (N + 127) * (9 * 128 + kpt) < LIM <= (N + 8 + 127) * (9 * 128 + kpt)
    assert _ok(1, 8, 8, 32, kpt, N + 8) == 0 and b"4 GiB" in L.vcx_last_error()
    assert (64 + 127) * kpt < LIM
    # ... and each of the three at the first shape whose extent is 2^32 or more
    assert _ok(1, (1 << 32) // (1280 * W) + 1, W, 1280, 32, 8) == 0 and _ok(1, (1 << 32) // (1280 * W) + 1, W, 32, 1280, 8) == 0
    assert _ok(1, 8, 8, 32, kpt, 4096) == 0


def test_launchers_validate_before_any_launch():
    L = _lib.lib()
    FAKE = 1 << 20
    names = (("a", FAKE), ("as_", FAKE), ("t", FAKE), ("ts", FAKE), ("w", FAKE), ("ws", FAKE), ("out", FAKE), ("bias", FAKE), ("cs", None), ("n", 2), ("H", 8), ("W", 8),
             ("cin", 64), ("ct", 96), ("N", 64), ("ldc", 64), ("ldcs", 0), ("flags", BIAS), ("stream", None))
    args = lambda **kw: [kw.get(k, d) for k, d in names]
    call = lambda **kw: L.vcx_conv3x3_tail_mxfp8(*args(**kw))
    assert call(bias=None) == -1 and b"null" in L.vcx_last_error()
    assert call(t=None) == -1 and b"null" in L.vcx_last_error()
    assert call(ts=None) == -1 and call(a=None) == -1 and call(ws=None) == -1
    assert call(flags=CS, ldcs=64) == -1 and b"colstats" in L.vcx_last_error()
    assert call(ct=48) == -1 and b"Ct" in L.vcx_last_error()
    assert call(cin=48) == -1 and b"Cin % 32" in L.vcx_last_error()
    assert call(flags=BIAS | G.GEMM_RESIDUAL) == -1 and b"flags" in L.vcx_last_error()
    assert call(flags=BIAS | G.GEMM_ROWADD) == -1 and b"flags" in L.vcx_last_error()
    assert call(flags=0) == -1 and b"flags" in L.vcx_last_error()
    assert call(ldc=56) == -1
    assert call(flags=CS, cs=FAKE, ldcs=161) == -1 and b"COLSTATS" in L.vcx_last_error()
    assert call(flags=CS, cs=FAKE + 8, ldcs=64) == -1 and b"aligned" in L.vcx_last_error()          # an odd first moments column
    assert call(t=FAKE + 8) == -1 and b"aligned" in L.vcx_last_error()
    assert call(ts=FAKE + 2) == -1 and b"aligned" in L.vcx_last_error()
    W = 1024
    assert call(n=1, H=(1 << 32) // (1280 * W) + 1, W=W, cin=1280, ct=32, N=8, ldc=8) == -1 and b"4 GiB" in L.vcx_last_error()
    assert call(n=1, H=(1 << 32) // (1280 * W) + 1, W=W, cin=32, ct=1280, N=8, ldc=8) == -1 and b"4 GiB" in L.vcx_last_error()
    assert call(n=1, H=8, W=8, cin=32, ct=1 << 20, N=4096, ldc=4096) == -1 and b"4 GiB" in L.vcx_last_error()
    gn = (("x", FAKE), ("q", FAKE), ("s", FAKE), ("rq", FAKE), ("rs", FAKE), ("stats", FAKE), ("g", FAKE), ("b", FAKE), ("n", 1), ("pix", 64), ("C", 64), ("groups", 32),
          ("eps", 1e-5), ("silu", 1), ("stream", None))
    raw = lambda **kw: L.vcx_groupnorm_apply_mxfp8_raw_f16(*[kw.get(k, d) for k, d in gn])
    assert raw(rq=None) == -1 and b"null" in L.vcx_last_error()
    assert raw(rs=None) == -1 and raw(q=None) == -1 and raw(x=None) == -1
    assert raw(C=48, groups=8) == -1 and b"C % 32" in L.vcx_last_error()
    assert raw(rq=FAKE + 8) == -1 and b"aligned" in L.vcx_last_error()
    assert raw(rs=FAKE + 2) == -1 and b"aligned" in L.vcx_last_error()
    gn2 = (("x1", FAKE), ("c1", 32), ("x2", FAKE), ("q", FAKE), ("s", FAKE), ("rq", FAKE), ("rs", FAKE), ("stats", FAKE), ("g", FAKE), ("b", FAKE), ("n", 1), ("pix", 64),
           ("C", 64), ("groups", 32), ("eps", 1e-5), ("silu", 1), ("stream", None))
    raw2 = lambda **kw: L.vcx_groupnorm_apply2_mxfp8_raw_f16(*[kw.get(k, d) for k, d in gn2])
    assert raw2(x2=None) == -1 and b"x2" in L.vcx_last_error()
    assert raw2(c1=12) == -1 and b"c1 % 8" in L.vcx_last_error()
    assert raw2(c1=64) == -1 and raw2(rq=None) == -1 and raw2(rs=None) == -1
    assert raw2(c1=40, C=72, groups=8) == -1 and b"C % 32" in L.vcx_last_error()


# ------------------------------------------------------------------------------------------------------------------ bindings
NEW = ["vcx_groupnorm_apply_mxfp8_raw_f16", "vcx_groupnorm_apply2_mxfp8_raw_f16", "vcx_conv3x3_tail_mxfp8", "vcx_conv3x3_tail_mxfp8_ok"]


def test_header_library_and_bindings_agree_and_the_abi_number_stays():
    import os
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vcx.h")).read()
    declared = set(re.findall(r"\b(vcx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and getattr(L, name) is not None
        assert len(getattr(L, name).argtypes) == {"vcx_groupnorm_apply_mxfp8_raw_f16": 15, "vcx_groupnorm_apply2_mxfp8_raw_f16": 17, "vcx_conv3x3_tail_mxfp8": 19,
                                                  "vcx_conv3x3_tail_mxfp8_ok": 10}[name]
    assert declared == set(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 62
    assert L.vcx_abi_version() == 18 and "#define VCX_ABI_VERSION 18" in header


# ------------------------------------------------------------------------------------------------------------------ host graph
class _TailRecorder(_Recorder):
    """tests/test_mxfp8_resconv_cpu._Recorder plus the three new launchers.  `tail_accept(kw)`: the tailed predicate's answer."""

    NAMES = _Recorder.NAMES + ("group_norm_mxfp8_raw", "conv3x3_tail_mxfp8", "conv3x3_tail_mxfp8_ok")

    def __init__(self, monkeypatch, accept=lambda kw: True, tail_ok=True, tail_accept=lambda kw: True):
        self.tail_accept = tail_accept
        super().__init__(monkeypatch, accept=accept, tail_ok=tail_ok)

    def names(self, skip=("ok", "tail_ok")):
        return super().names(skip=skip)

    def group_norm_mxfp8_raw(self, x, gamma, beta, eps, silu, groups=32, stats=None, x2=None):
        self.calls.append(("group_norm_mxfp8_raw", tuple(x.shape), silu, stats is not None, x2 is not None))
        C = x.shape[2] + (0 if x2 is None else x2.shape[2])
        rows, kp = x.shape[0] * x.shape[1], MX.kp_of(C)
        pair = lambda: (torch.zeros((rows, kp), dtype=torch.uint8), torch.zeros((rows, kp // 32), dtype=torch.uint8))
        return pair(), pair()

    def conv3x3_tail_mxfp8_ok(self, n, H, W, cin, ct, cout, **kw):
        self.calls.append(("tail_ok", n, cin, ct, cout, dict(kw)))
        return self.tail_accept(kw)

    def conv3x3_tail_mxfp8(self, a, tail, w, bias, *, n, H, W, cin, ct, **kw):
        kp, kpt = MX.kp_of(cin), MX.kp_of(ct)
        assert a[0].shape == (n * H * W, kp) and tail[0].shape == (n * H * W, kpt) and tail[1].shape == (n * H * W, kpt // 32)
        assert w[0].shape == (bias.numel(), 9 * kp + kpt) and w[1].shape == (bias.numel(), (9 * kp + kpt) // 32)
        self.calls.append(("conv3x3_tail_mxfp8", sorted(k for k in kw if kw[k] is not None), kw, ct, tail))
        out = kw.get("out")
        return (torch.zeros((n * H * W, bias.numel()), dtype=torch.float16) if out is None else out).view(n, H, W, -1)


def _summary(rec):
    """the recorded calls without tensors: names, shapes, keyword names, predicate keywords"""
    out = []
    for c in rec.calls:
        if c[0] in ("conv3x3_mxfp8", "conv3x3_tail_mxfp8"):
            out.append((c[0], tuple(c[1])))
        elif c[0] == "stats_from_colstats":
            out.append((c[0], c[2]))
        elif c[0] == "ok":
            out.append((c[0], c[1], c[2], c[3], tuple(sorted((k, v) for k, v in c[4].items()))))
        else:
            out.append(tuple(tuple(v) if isinstance(v, list) else v for v in c))
    return out


# kind -> (channels of x, channels of x2, out_channels, moments of the input handed in)
KINDS = {"identity": (64, 0, 64, False), "skip_conv": (64, 0, 128, False), "split_concat": (64, 64, 64, True), "materialised_concat": (64, 64, 64, False)}
G16 = ("group_norm", (N_FRAMES, 64, 64), True)
# the parent's calls: (kind, RESCONV_MXFP8, KEEP_FOLD) -> names, as tests/test_mxfp8_resconv_cpu.py states them for the parent route
PARENT = {
    ("identity", False): ["group_norm", "linear", "conv2d", "stats_from_colstats", "group_norm", "conv2d"],
    ("skip_conv", False): ["group_norm", "linear", "conv2d", "stats_from_colstats", "group_norm", "conv2d"],
    ("split_concat", False): ["stats_from_colstats", "group_norm", "linear", "conv2d", "stats_from_colstats", "group_norm", "conv2d"],
    ("materialised_concat", False): ["concat_channels", "group_norm", "linear", "conv2d", "stats_from_colstats", "group_norm", "conv2d"],
    ("identity", True, True): ["group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm_mxfp8", "conv3x3_mxfp8"],
    ("identity", True, False): ["group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm_mxfp8", "conv3x3_mxfp8"],
    ("skip_conv", True, True): ["group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm", "conv2d"],
    ("skip_conv", True, False): ["group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm_mxfp8", "conv2d", "conv3x3_mxfp8"],
    ("split_concat", True, True): ["stats_from_colstats", "group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm", "conv2d"],
    ("split_concat", True, False): ["stats_from_colstats", "group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm", "conv2d"],
    ("materialised_concat", True, True): ["concat_channels", "group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm", "conv2d"],
    ("materialised_concat", True, False): ["concat_channels", "group_norm_mxfp8", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm_mxfp8", "conv2d",
                                           "conv3x3_mxfp8"],
}
# ... and the keywords of the block's last convolution: (launcher, kernel size or None, keyword names, tail sources)
PARENT_LAST = {
    ("identity", False): ("conv2d", 3, ["residual"], 0), ("skip_conv", False): ("conv2d", 3, ["tail"], 1), ("split_concat", False): ("conv2d", 3, ["tail"], 2),
    ("materialised_concat", False): ("conv2d", 3, ["tail"], 1),
    ("identity", True, True): ("conv3x3_mxfp8", ["residual"]), ("identity", True, False): ("conv3x3_mxfp8", ["residual"]),
    ("skip_conv", True, True): ("conv2d", 3, ["tail"], 1), ("skip_conv", True, False): ("conv3x3_mxfp8", ["residual"]),
    ("split_concat", True, True): ("conv2d", 3, ["tail"], 2), ("split_concat", True, False): ("conv2d", 3, ["tail"], 2),
    ("materialised_concat", True, True): ("conv2d", 3, ["tail"], 1), ("materialised_concat", True, False): ("conv3x3_mxfp8", ["residual"]),
}


def _run_kind(blk, kind, **kw):
    c1, c2, _, moments = KINDS[kind]
    if c2:
        kw["x2"] = torch.zeros((N_FRAMES, HH, WW, c2), dtype=torch.float16)
    if moments:
        kw["colstats"] = torch.zeros((N_FRAMES * HH * WW // 64, c1 + c2, 2))
    return _run(blk, c1, **kw)


def _set(monkeypatch, U, resconv, keep_fold, tail):
    monkeypatch.setattr(U, "RESCONV_MXFP8", resconv)
    monkeypatch.setattr(U, "RESCONV_MXFP8_SKIP_DIMS", frozenset())
    monkeypatch.setattr(U, "RESCONV_MXFP8_KEEP_FOLD", keep_fold)
    monkeypatch.setattr(U, "RESCONV_MXFP8_TAIL", tail)


def test_the_new_switch_is_off_by_default_and_read_once_at_import():
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    assert U.RESCONV_MXFP8_TAIL is False
    assert 'os.environ.get("VCX_RESCONV_MXFP8_TAIL", "0") == "1"' in open(U.__file__).read()


@pytest.mark.parametrize("keep_fold", [False, True])
@pytest.mark.parametrize("resconv", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_new_switch_off_makes_exactly_the_parents_calls(monkeypatch, kind, resconv, keep_fold):
    c1, c2, cout, _ = KINDS[kind]
    U, blk = _block(c1 + c2, cout)
    _set(monkeypatch, U, resconv, keep_fold, False)
    rec = _TailRecorder(monkeypatch)
    h, _ = _run_kind(blk, kind)
    key = (kind, True, keep_fold) if resconv else (kind, False)
    assert rec.names() == PARENT[key]
    last = rec.calls[-1]
    assert (last[:4] if last[0] == "conv2d" else last[:2]) == PARENT_LAST[key]
    assert not any(c[0] in ("group_norm_mxfp8_raw", "conv3x3_tail_mxfp8", "tail_ok") for c in rec.calls), "a new launcher was called with the new switch off"
    assert "w2s" not in blk._mx and (resconv or blk._mx == {})
    assert h.shape == (N_FRAMES, HH, WW, cout)
    # the new switch on under RESCONV_MXFP8 = 0 or KEEP_FOLD = 1, or at an identity block: the same calls, keyword for keyword
    if not resconv or keep_fold or kind == "identity":
        U2, blk2 = _block(c1 + c2, cout)
        _set(monkeypatch, U2, resconv, keep_fold, True)
        rec2 = _TailRecorder(monkeypatch)
        _run_kind(blk2, kind)
        assert _summary(rec2) == _summary(rec) and "w2s" not in blk2._mx
        assert not rec2.of("tail_ok"), "the new switch was consulted where it does not apply"


@pytest.mark.parametrize("want", [False, True])
def test_switch_on_skip_conv_block_runs_the_raw_norm_and_the_tailed_convolution(monkeypatch, want):
    U, blk = _block(64, 128)
    _set(monkeypatch, U, True, False, True)
    rec = _TailRecorder(monkeypatch)
    h, cs = _run(blk, want_colstats=want)
    assert rec.names() == ["group_norm_mxfp8_raw", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm_mxfp8", "conv3x3_tail_mxfp8"]
    assert "conv2d" not in rec.names() and "concat_channels" not in rec.names()
    asked = rec.of("tail_ok")
    assert [c[1:5] for c in asked] == [(2, 128, 64, 128), (4, 128, 64, 128)], "asked about one video's frames and about the call's: cin = cout, ct = the block's input"
    assert all(c[5]["colstats"] == want and c[5]["ldc"] is None for c in asked)
    every = rec.names(skip=())
    assert every.index("group_norm_mxfp8_raw") > max(i for i, n in enumerate(every) if n in ("ok", "tail_ok")), "the route is decided before anything runs"
    assert rec.of("group_norm_mxfp8_raw")[0][1:] == ((N_FRAMES, 64, 64), True, False, False)
    assert rec.of("conv3x3_mxfp8")[0][1] == ["colstats", "rowadd", "rowadd_div"]
    conv = rec.of("conv3x3_tail_mxfp8")[0]
    assert conv[1] == (["colstats"] if want else []) and conv[3] == 64 and "residual" not in conv[2]
    assert conv[4][0].shape == (N_FRAMES * 64, 128) and (cs is not None) == want and (not want or cs is conv[2]["colstats"])
    assert h.shape == (N_FRAMES, HH, WW, 128)
    assert sorted(blk._mx) == ["w1", "w2s"] and blk._mx["w2s"][0].shape == (128, 9 * 128 + 128) and blk._mx["w2s"][1].shape == (128, 40)
    first = dict(blk._mx)
    _run(blk)
    assert all(blk._mx[k] is first[k] for k in first), "the packs are built once"
    blk.load_state_dict(blk.state_dict())
    assert blk._mx == {}


def test_switch_on_split_concat_is_read_in_place_by_the_two_source_raw_norm(monkeypatch):
    U, blk = _block(128, 64)
    _set(monkeypatch, U, True, False, True)
    rec = _TailRecorder(monkeypatch)
    h, _ = _run_kind(blk, "split_concat")
    assert rec.names() == ["stats_from_colstats", "group_norm_mxfp8_raw", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm_mxfp8", "conv3x3_tail_mxfp8"]
    assert rec.of("group_norm_mxfp8_raw")[0][1:] == ((N_FRAMES, 64, 64), True, True, True), "the left half, with statistics and x2"
    assert [c[1:5] for c in rec.of("tail_ok")] == [(2, 64, 128, 64), (4, 64, 128, 64)]
    conv = rec.of("conv3x3_tail_mxfp8")[0]
    assert conv[3] == 128 and conv[4][0].shape == (N_FRAMES * 64, 128), "one tail source: the quantised concat"
    assert h.shape == (N_FRAMES, HH, WW, 64) and sorted(blk._mx) == ["w1", "w2s"]


def test_switch_on_split_concat_without_moments_is_materialised_once(monkeypatch):
    U, blk = _block(128, 64)
    _set(monkeypatch, U, True, False, True)
    rec = _TailRecorder(monkeypatch)
    _run_kind(blk, "materialised_concat")
    assert rec.names() == ["concat_channels", "group_norm_mxfp8_raw", "linear", "conv3x3_mxfp8", "stats_from_colstats", "group_norm_mxfp8", "conv3x3_tail_mxfp8"]
    assert rec.of("group_norm_mxfp8_raw")[0][1:] == ((N_FRAMES, 64, 128), True, False, False), "the single-source form on the materialised concat"


@pytest.mark.parametrize("why", ["conv1", "tailed", "keep_fold", "identity"])
@pytest.mark.parametrize("kind", ["skip_conv", "split_concat", "materialised_concat"])
def test_a_refusal_gives_the_parent_route(monkeypatch, kind, why):
    if why == "identity":
        kind = "identity"
    c1, c2, cout, _ = KINDS[kind]
    accept = (lambda q: not q.get("rowadd")) if why == "conv1" else (lambda q: True)
    tail_accept = (lambda q: False) if why == "tailed" else (lambda q: True)
    runs = []
    for tail in (False, True):
        U, blk = _block(c1 + c2, cout)
        _set(monkeypatch, U, True, why == "keep_fold", tail)
        rec = _TailRecorder(monkeypatch, accept=accept, tail_accept=tail_accept)
        _run_kind(blk, kind, want_colstats=True)
        runs.append((rec, blk))
    (off, blk_off), (on, blk_on) = runs
    assert _summary(on)[:] and [c for c in _summary(on) if c[0] != "tail_ok"] == _summary(off), "the calls of the parent route, keyword for keyword"
    assert not on.of("group_norm_mxfp8_raw") and not on.of("conv3x3_tail_mxfp8") and sorted(blk_on._mx) == sorted(blk_off._mx) and "w2s" not in blk_on._mx
    assert bool(on.of("tail_ok")) == (why == "tailed"), "the tailed predicate is asked only where conv1 is MX, KEEP_FOLD is off and there is a skip convolution"


@pytest.mark.parametrize("why", ["up", "down", "scale_shift", "skipped"])
def test_blocks_off_the_mx_route_are_left_alone(monkeypatch, why):
    kw = dict(up=dict(up=True), down=dict(down=True), scale_shift=dict(use_scale_shift_norm=True)).get(why, {})
    runs = []
    for tail in (False, True):
        U, blk = _block(64, 128, **kw)
        _set(monkeypatch, U, True, False, tail)
        monkeypatch.setattr(U, "RESCONV_MXFP8_SKIP_DIMS", frozenset([128] if why == "skipped" else []))
        rec = _TailRecorder(monkeypatch)
        _run(blk, want_colstats=True)
        runs.append(rec)
        assert blk._mx == {}
    assert _summary(runs[1]) == _summary(runs[0]) and not any("mxfp8" in n for n in runs[1].names(skip=()))


def test_target_and_temporal_plumbing_arrive_at_the_tailed_convolution(monkeypatch):
    from viewcrafter_amd.lvdm.modules.flow import CatTarget
    U, blk = _block(64, 128)
    _set(monkeypatch, U, True, False, True)
    rec = _TailRecorder(monkeypatch)
    M = N_FRAMES * 64
    target = CatTarget(M, 128, 32, "cpu", with_moments=True)
    h, cs = _run(blk, target=target)
    last = rec.of("tail_ok")[-1][5]
    assert last["ldc"] == 160 and last["colstats_ld"] == 160 and last["colstats"] is True, "the predicate sees the concat buffer's pitches"
    conv = rec.of("conv3x3_tail_mxfp8")[-1]
    assert conv[1] == ["colstats", "colstats_col", "colstats_ld", "ldc", "out"] and conv[2]["colstats_col"] == 0 and conv[2]["out"] is target.data
    assert cs is target.moments and h.shape == (N_FRAMES, HH, WW, 160)
    # the temporal block behind the second convolution: the tailed convolution produces its per-video moments
    U, blk = _block(64, 128, use_temporal_conv=True)
    _set(monkeypatch, U, True, False, True)
    rec = _TailRecorder(monkeypatch)
    calls = []
    monkeypatch.setattr(blk.temopral_conv, "forward", lambda h, **kw: (calls.append((tuple(h.shape), kw)), (h, None))[1])
    h, _ = _run(blk)
    conv = rec.of("conv3x3_tail_mxfp8")[-1]
    assert conv[1] == ["colstats"] and calls[0][0] == (2, 2, 64, 128) and calls[0][1]["colstats"] is conv[2]["colstats"]


def test_the_real_predicate_and_the_cpu_stand_in():
    """ops.conv3x3_tail_mxfp8_ok is the library's answer; the CPU stand-in of the launcher (tests/cpu_kernels_mx_tail.py) is the documented
    function: on exact operands it equals the fp64 sum of the two convolutions, and its tail reads row m itself."""
    from tests import cpu_kernels_mx_tail as CT
    from viewcrafter_amd import ops
    assert ops.conv3x3_tail_mxfp8_ok(4, 8, 8, 128, 64, 128, colstats=True) is True
    assert ops.conv3x3_tail_mxfp8_ok(4, 5, 8, 128, 64, 128, colstats=True) is False and b"COLSTATS" in _lib.lib().vcx_last_error()
    assert ops.conv3x3_tail_mxfp8_ok(4, 8, 8, 128, 72, 128) is False
    n, H, W, cin, ct, N = 2, 3, 4, 32, 64, 8
    M = n * H * W
    aq, asc, a = MX.exact_operand(M, cin, 1)
    tq, tsc, t = MX.exact_operand(M, ct, 2)
    wq, wsc, w = MX.exact_operand(9 * N, cin, 3)
    vq, vsc, v = MX.exact_operand(N, ct, 4)
    bias = torch.arange(N).float()
    out = CT.conv3x3_tail_mxfp8((aq, asc), (tq, tsc), CT.join_weight(CT.slab_major(wq, wsc, N), (vq, vsc)), bias, n=n, H=H, W=W, cin=cin, ct=ct).view(M, N)
    a4 = torch.nn.functional.conv2d(a.view(n, H, W, cin).permute(0, 3, 1, 2), w.view(N, 3, 3, cin).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(M, N)
    assert torch.equal(out.double(), (a4 + t @ v.t() + bias.double()).half().double())
