"""ff.net[2] + proj_out of a transformer as one GEMM with a linear K tail (packing.pack_ff_out_folded, ops.linear_tail_ok, vcx_gemm_route):
the pack's algebra and the route's answers, without a GPU.  The kernel side is tests/test_ff_out_fold_gpu.py."""
import ctypes

import pytest
import torch

from viewcrafter_amd import _lib as G
from viewcrafter_amd import ops
from viewcrafter_amd.packing import pack_ff_out_folded

# (rows of the benchmark's B = 2 forward, D) per UNet level: N = D, main K = 4 D, tail D
BENCH = [(460800, 320), (115200, 640), (28800, 1280)]


def _route(M, N, K, tails, unit_rows=0, flags=G.GEMM_BIAS_N, **kw):
    d = ops._gemm_desc(M, N, K + sum(k for k, _ in tails), kw.pop("lda", K), kw.pop("ldc", N), tail=tails, flags=flags, **kw)
    L = G.lib()
    return L.vcx_gemm_route(ctypes.byref(d), unit_rows), L.vcx_last_error()


@pytest.mark.parametrize("D,C", [(64, 64), (128, 72)])
def test_pack_is_the_fp64_algebra_of_the_fp16_weights_rounded_once(D, C):
    g = torch.Generator().manual_seed(D)
    w2 = torch.randn((D, 4 * D), generator=g) * (4 * D) ** -0.5
    b2 = torch.randn((D,), generator=g) * 0.1
    wout = torch.randn((C, D), generator=g) * D ** -0.5
    bout = torch.randn((C,), generator=g) * 0.1
    wcat, bcat = pack_ff_out_folded(w2, b2, wout, bout)
    assert wcat.dtype is torch.float16 and tuple(wcat.shape) == (C, 5 * D) and wcat.is_contiguous()
    assert bcat.dtype is torch.float32 and tuple(bcat.shape) == (C,)
    w2d, woutd = w2.half().double(), wout.half().double()
    assert torch.equal(wcat[:, :4 * D], (woutd @ w2d).half()), "the product columns are not ONE rounding of the fp64 product of the fp16 weights"
    assert torch.equal(wcat[:, 4 * D:], wout.half()), "the tail columns are not Wout itself"
    assert torch.equal(bcat, (woutd @ b2.double() + bout.double()).float())
    # the folded layer against the two layers it replaces, both in fp64 on the pack's own operands: they differ by the product's rounding only
    gl, t = torch.randn((50, 4 * D), generator=g).double(), torch.randn((50, D), generator=g).double()
    two = (gl @ w2d.t() + b2.double() + t) @ woutd.t() + bout.double()
    one = torch.cat([gl, t], 1) @ wcat.double().t() + bcat.double()
    assert float((one - two).norm() / two.norm()) < 2.0 ** -11


def test_pack_runs_on_meta_tensors():
    D, C = 320, 320
    with torch.device("meta"):
        wcat, bcat = pack_ff_out_folded(torch.empty((D, 4 * D)), torch.empty((D,)), torch.empty((C, D), dtype=torch.float16), torch.empty((C,)))
    assert wcat.is_meta and wcat.dtype is torch.float16 and tuple(wcat.shape) == (C, 5 * D)
    assert bcat.is_meta and bcat.dtype is torch.float32 and tuple(bcat.shape) == (C,)


@pytest.mark.parametrize("M,D", BENCH)
def test_the_benchmark_shapes_go_to_the_tiled_engine(M, D):
    """... with proj_out's epilogues: bias + residual, with and without column moments, into a concat buffer (ldc > N) - and never to a
    weight-stationary kernel, although N = 320 with K = 320 + M >= 8192 is that kernel's shape without the tail."""
    for cs in (0, G.GEMM_COLSTATS):
        for ldc in (D, 2 * D):
            rc, msg = _route(M, D, 4 * D, [(D, D)], flags=G.GEMM_BIAS_N | G.GEMM_RESIDUAL | cs, ldr=D, ldc=ldc)
            assert rc == G.ROUTE_TILED, (rc, msg)
            assert ops.linear_tail_ok(M, D, 4 * D, [D], ldc=ldc, residual=True, colstats=bool(cs))
    assert _route(8192, 320, 320, [(320, 320)])[0] == G.ROUTE_TILED and _route(8192, 320, 320, [])[0] == G.ROUTE_WS320
    assert _route(1000, 136, 256, [(64, 64), (64, 72)])[0] == G.ROUTE_TILED          # two sources, a row stride beyond the width


def test_what_the_kernel_cannot_do_is_refused():
    base = dict(M=1000, N=64, K=128)
    ok = lambda **kw: ops.linear_tail_ok(kw.pop("M", 1000), kw.pop("N", 64), kw.pop("K", 128), kw.pop("tail_ks", [64]), **kw)
    assert ok() and ok(tail_ks=[64, 128])
    assert not ok(tail_ks=[32]) and not ok(tail_ks=[]) and not ok(tail_ks=[64, 64, 64]) and not ok(tail_ks=[0])
    assert not ok(K=72) and not ok(K=96), "main K % 64 != 0"
    assert not ok(N=60), "N % 8 != 0: the register-staged kernel has no tail"
    rc, msg = _route(tails=[(64, 56)], **base)                                        # tail_lda < tail_k
    assert rc == -1 and b"K tail" in msg
    rc, msg = _route(tails=[(32, 32)], **base)
    assert rc == -1 and b"K tail" in msg
    rc, msg = _route(tails=[(64, 68)], **base)                                        # tail_lda % 8 != 0
    assert rc == -1 and b"K tail" in msg
    rc, msg = _route(1000, 64, 72, [(64, 64)], lda=72)
    assert rc == G.ROUTE_REFUSED and b"a K tail needs the DMA kernel" in msg
    for flag, extra in ((G.GEMM_GEGLU, {}), (G.GEMM_LNFOLD, {}), (G.GEMM_ROWSTATS, {}), (G.GEMM_OUT_F32, {})):
        rc, msg = _route(tails=[(64, 64)], flags=G.GEMM_BIAS_N | flag, **base, **extra)
        assert rc == G.ROUTE_REFUSED and b"linear K tail" in msg, (flag, rc, msg)
    rc, msg = _route(8 * 1024, 320, 320, [(64, 64)], flags=G.GEMM_BIAS_N | G.GEMM_ROWSTATS)      # the weight-stationary kernel's ROWSTATS shape
    assert rc == G.ROUTE_REFUSED and b"linear K tail" in msg
    rc, msg = _route(3 * 3600, 640, 128, [(64, 64)], unit_rows=3600)                  # per-unit weights (vcx_gemm_units_f16)
    assert rc == G.ROUTE_REFUSED and b"no K tail" in msg
    ops.tune_set("GEMM_DMA", 0)
    try:
        assert not ok()                                                               # the register-staged kernel
    finally:
        ops.tune_set("GEMM_DMA", 1)
    for cfg, want in ((0, True), (2, True), (4, True), (5, True), (6, False)):        # 6: the GEGLU configuration
        ops.tune_set("GEMM_CFG", cfg)
        try:
            assert ok() == want, cfg
        finally:
            ops.tune_set("GEMM_CFG", -1)


def test_the_launcher_refuses_with_the_same_text():
    """vcx_gemm_f16 (fake pointers: the refusal comes before any launch) and vcx_gemm_route run the same code."""
    from tests.test_abi import EINVAL, FAKE, _gemm_rc
    for kw in (dict(M=1000, N=64, K=72 + 64, lda=72, ldc=64, tail_k0=64, tail_lda0=64),
               dict(M=1000, N=64, K=192, lda=128, ldc=64, tail_k0=64, tail_lda0=64, flags=G.GEMM_LNFOLD, ln_stats=FAKE, ln_colsum=FAKE),
               dict(M=1000, N=64, K=192, lda=128, ldc=64, tail_k0=64, tail_lda0=64, flags=G.GEMM_ROWSTATS, rowstats=FAKE)):
        rc, msg = _gemm_rc(tail_a0=FAKE, **kw)
        assert rc == EINVAL and b"K tail" in msg, (rc, msg)
        d = G.GemmDesc(alpha=1.0, ldw=kw["K"])
        for k, v in kw.items():
            setattr(d, k, v)
        assert G.lib().vcx_gemm_route(ctypes.byref(d), 0) == G.ROUTE_REFUSED and G.lib().vcx_last_error() == msg


def test_extents_flip_where_the_dispatcher_starts_rejecting():
    """linear_tail_ok turns false at exactly the row count where vcx_gemm_f16 rejects the call: the main operand (K = 4 D columns), the
    tail source and the output (256 rows past the end) each against the 32-bit limit."""
    from tests.test_abi import EINVAL, FAKE, LIM, _gemm_rc
    from tests.test_host_logic import _first_false
    # level 0 widths: the main operand g [M, 1280] goes first
    m = _first_false(lambda r: ops.linear_tail_ok(r, 320, 1280, [320], residual=True), 460800, 1 << 24)
    assert 2 * ((m - 1) * 1280 + 1280) >= LIM > 2 * ((m - 2) * 1280 + 1280)
    rc, msg = _gemm_rc(M=m, N=320, K=1600, lda=1280, ldc=320, ldr=320, residual=FAKE, bias=FAKE, flags=G.GEMM_BIAS_N | G.GEMM_RESIDUAL, tail_a0=FAKE, tail_k0=320, tail_lda0=320)
    assert rc == EINVAL and b"K tail" in msg
    # the tail source through its row stride: M rows of 4096 elements
    kw = dict(N=64, K=128, lda=64, ldc=64, tail_a0=FAKE, tail_k0=64, tail_lda0=4096)
    d_ok = lambda r: _route(r, 64, 64, [(64, 4096)])[0] == G.ROUTE_TILED
    m = _first_false(d_ok, 1000, 1 << 22)
    assert 2 * ((m - 1) * 4096 + 64) >= LIM > 2 * ((m - 2) * 4096 + 64) and _gemm_rc(M=m, **kw)[0] == EINVAL
    # the output: a narrow problem into a wide buffer
    m = _first_false(lambda r: ops.linear_tail_ok(r, 64, 64, [64], ldc=4096), 1000, 1 << 22)
    assert 2 * (m + 256) * 4096 >= LIM > 2 * (m + 255) * 4096
    assert _gemm_rc(M=m, N=64, K=128, lda=64, ldc=4096, tail_a0=FAKE, tail_k0=64, tail_lda0=64)[0] == EINVAL


@pytest.mark.parametrize("T,h,w", [(3, 40, 64), (25, 72, 128)])
def test_the_answer_for_one_video_is_the_answer_for_a_batch(T, h, w):
    """Every level of the UNet, both transformer kinds' keywords: the predicate for one video's rows equals the one for 2 and 3 videos."""
    for level, D in enumerate((320, 640, 1280, 1280)):
        rows = T * (h >> level) * (w >> level)
        for cs in (False, True):
            if cs and rows % 64 != 0:
                continue
            one = ops.linear_tail_ok(rows, D, 4 * D, [D], residual=True, colstats=cs)
            assert one, (level, rows)
            for B in (2, 3):
                assert ops.linear_tail_ok(B * rows, D, 4 * D, [D], residual=True, colstats=cs) == one, (level, B)
