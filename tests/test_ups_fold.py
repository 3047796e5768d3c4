"""Upsample convolutions folded into four 2x2 weight sets (packing.pack_conv_ups_folded, ops.conv2d_ups_folded_ok): the arithmetic of the
fold against fp64 nearest-2x + 3x3, and the library's route answers.  No GPU."""
import pytest
import torch

from tests import ups_fold_ref as R
from tests.util import rel_l2

# n, cin, cout, H, W: ragged, a single pixel (every tap a border tap), H != W with W = 1, and a multi-slab square-ish one
SHAPES = [(2, 64, 72, 9, 11), (1, 64, 64, 1, 1), (1, 128, 64, 3, 1), (1, 320, 320, 18, 16), (1, 8, 24, 5, 7)]


def _problem(n, cin, cout, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, H, W, cin), generator=g).half()
    w = (torch.randn((cout, cin, 3, 3), generator=g) * (9 * cin) ** -0.5).half()
    return x, w


@pytest.mark.parametrize("n,cin,cout,H,W", SHAPES)
def test_fold_is_the_same_function(n, cin, cout, H, W):
    """Unrounded sums: the four-class form equals nearest-2x + 3x3 (fp64: the same products, regrouped; differences are fp64 rounding of the
    regrouping, < 1e-13 of the output's scale - `equal` at fp64's level).  Rounded once to fp16: the output moves by one more fp16 rounding
    of a constant; the rel-L2 is printed (2e-4 expected) and bounded by 2^-10, the worst one rounding of every weight can do in the norm."""
    from viewcrafter_amd.packing import pack_conv, pack_conv_ups_folded
    x, w = _problem(n, cin, cout, H, W)
    ref = R.nine_tap_ref(x, w)
    w4 = R.fold_classes(w)
    packed64 = pack_conv_ups_folded(w, dtype=None)
    assert packed64.dtype == torch.float64 and tuple(packed64.shape) == (4, cout, 4 * cin)
    assert torch.equal(R.unpack_folded(packed64, cin), w4), "pack_conv_ups_folded: not the tap sums of the four classes in pack_conv's order"
    for c in range(4):
        assert torch.equal(packed64[c], pack_conv(w4[c >> 1, c & 1])), f"class {c} is not packed like a 2x2 kernel"
    exact = R.folded_ref(x, w4)
    scale = float(ref.abs().max())
    assert float((exact - ref).abs().max()) <= 1e-13 * scale
    packed16 = pack_conv_ups_folded(w)
    assert packed16.dtype == torch.float16 and torch.equal(packed16, packed64.half()), "the sums must be rounded once, from fp64"
    moved = rel_l2(R.folded_ref(x, R.unpack_folded(packed16, cin)), ref)
    print(f"\n[ups fold] n {n} cin {cin} cout {cout} {H}x{W}: unrounded max |d| {float((exact - ref).abs().max()):.2e}, rounded sums rel-L2 {moved:.3e}")
    assert moved <= 2.0 ** -10


def test_integer_weights_fold_exactly():
    from viewcrafter_amd.packing import pack_conv_ups_folded
    from tests import exact_inputs as X
    w = X.int_tensor((72, 64, 3, 3), -1, 1, 5)
    x = X.int_tensor((2, 5, 3, 64), -3, 3, 6)
    wf = pack_conv_ups_folded(w)
    assert torch.equal(wf.double(), pack_conv_ups_folded(w, dtype=None))
    assert torch.equal(R.folded_ref(x, R.unpack_folded(wf, 64)), R.nine_tap_ref(x, w))


def test_route_answers():
    """The three Upsample layers of the default workload and the refusals: H W % 64, W % 16, cin % 64, N % 8, 32-bit extents, a forced
    64-row configuration, the knob.  Asked of the library without a device (vcx_gemm_route)."""
    from viewcrafter_amd import ops
    ok = ops.conv2d_ups_folded_ok
    assert ok(*R.BENCH_LAYERS["36x64"], colstats=True) and ok(*R.BENCH_LAYERS["36x64"], ldc=1280, colstats=True)
    assert ok(*R.BENCH_LAYERS["18x32"], colstats=True) and ok(*R.BENCH_LAYERS["18x32"])
    assert not ok(*R.BENCH_LAYERS["9x16"]) and not ok(*R.BENCH_LAYERS["9x16"], colstats=True)          # 144 pixels: no whole 64-row strips
    assert ok(3, 4, 16, 64, 72) and ok(5, 8, 16, 128, 64, colstats=True) and ok(1, 8, 16, 128, 128)
    assert not ok(1, 8, 8, 64, 64)              # W % 16
    assert not ok(1, 2, 16, 64, 64)             # H W % 64
    assert not ok(1, 8, 16, 32, 64)             # cin % 64
    assert not ok(1, 8, 16, 64, 68)             # N % 8
    assert not ok(1, 8, 16, 64, 64, ldc=70)     # ldc % 4 (the launcher's validation)
    assert not ok(64, 256, 256, 320, 320)       # output beyond 32-bit byte offsets
    assert ok(40, 128, 128, 3200, 8) and not ok(41, 128, 128, 3200, 8)      # ... the source too (41 x 128 x 128 x 3200 x 2 bytes >= 0xFFFF0000)
    try:
        for cfg, want in ((0, True), (1, True), (2, True), (3, True), (4, False), (5, False), (6, False)):
            ops.tune_set("GEMM_CFG", cfg)
            assert ok(3, 4, 16, 64, 72) == want, cfg
    finally:
        ops.tune_set("GEMM_CFG", -1)
    try:
        ops.tune_set("GEMM_DMA", 0)
        assert not ok(3, 4, 16, 64, 72)
    finally:
        ops.tune_set("GEMM_DMA", 1)
    saved = ops.UPS_FOLD
    try:
        ops.UPS_FOLD = False
        assert not ok(*R.BENCH_LAYERS["36x64"])
    finally:
        ops.UPS_FOLD = saved


def test_cpu_graph_keeps_the_nine_tap_call(monkeypatch):
    """On a CPU tensor Upsample.forward calls ops.conv2d(..., ups=1) with the nine-tap pack, whatever the predicate says: the CPU stand-ins
    of the existing tests do not know the folded op."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import Upsample
    calls = []
    monkeypatch.setattr(ops, "conv2d", lambda x, w, b, **kw: calls.append((tuple(w.shape), kw)) or torch.zeros(x.shape[0], 2 * x.shape[1], 2 * x.shape[2], w.shape[0]))
    monkeypatch.setattr(ops, "conv2d_ups_folded", lambda *a, **k: pytest.fail("the folded op was called on a CPU tensor"))
    up = Upsample(128, True).eval()
    y, cs = up(torch.zeros(1, 8, 16, 128, dtype=torch.float16))
    assert calls == [((128, 9 * 128), dict(kh=3, kw=3, ups=1))] and cs is None and tuple(y.shape) == (1, 16, 32, 128)
    pk = up.packed()
    assert tuple(pk["wf"].shape) == (4, 128, 4 * 128) and pk["wf"].dtype == torch.float16 and tuple(pk["w"].shape) == (128, 9 * 128)
