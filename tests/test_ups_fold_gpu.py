"""The folded upsample convolution on the GPU (ops.conv2d_ups_folded; csrc/gemm_dma.hip UPSF, include/vcx.h ups = 2) under the tile plan
and every forced configuration it exists for (GEMM_CFG 0-3).

Shapes: n 3, 4x16, 64 -> 72 - 192 rows per parity class, ragged against 128- and 256-row tiles, so every tile after the first of a class
would straddle a class boundary if tiles were not counted per class, and N = 72 is ragged; n 5, 8x16, 128 -> 64 - 640 rows per class (2.5
large tiles), two channel slabs.  Measured on an MI355X (profiles/r11_ups_fold.md): E against the kernel's own rounded weights 1.0000,
against the original nine taps 1.16 - 1.17.
"""
import pytest
import torch

from tests import exact_inputs as X
from tests import rounding_quality as RQ
from tests import ups_fold_ref as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGS = (-1, 0, 1, 2, 3)
SHAPES = {"3x4x16_c64_n72": (3, 4, 16, 64, 72), "5x8x16_c128_n64": (5, 8, 16, 128, 64)}
SENTINEL = 77.0


def _forced(cfg):
    class _Ctx:
        def __enter__(self):
            from viewcrafter_amd import ops
            ops.tune_set("GEMM_CFG", cfg)

        def __exit__(self, *a):
            from viewcrafter_amd import ops
            ops.tune_set("GEMM_CFG", -1)
    return _Ctx()


def _random(shape, seed=0):
    n, H, W, cin, cout = shape
    x = RQ.randn((n, H, W, cin), 9000 + seed).half()
    w = RQ.randn((cout, cin, 3, 3), 9001 + seed, (9 * cin) ** -0.5).half()
    b = RQ.randn((cout,), 9002 + seed)
    return x, w, b


@pytest.fixture(scope="module")
def random_refs():
    """Per shape: inputs on the GPU, the packed weights, and the two fp64 references (computed once, on the GPU, never modified)."""
    from viewcrafter_amd.packing import pack_conv, pack_conv_ups_folded
    out = {}
    for name, shape in SHAPES.items():
        x, w, b = _random(shape)
        wf = pack_conv_ups_folded(w)
        xd, bd = x.to(DEV), b.to(DEV)
        own = R.folded_ref(xd, R.unpack_folded(wf, shape[3]), bd)              # the function of the operands the kernel receives
        orig = R.nine_tap_ref(xd, w.to(DEV), bd)
        out[name] = dict(x=xd, b=bd, wf=wf.to(DEV), w9=pack_conv(w).to(DEV), own=own, orig=orig)
    return out


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_integers_equal_the_nine_tap_kernel(name, cfg):
    """Integer inputs and weights: every product and partial sum is exact, the folded weights (sums of at most four taps in {-1, 0, 1}) too,
    so the folded kernel, the nine-tap kernel and the integer reference agree bit for bit - one wrong row, class, tap or tile is a mismatch."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv, pack_conv_ups_folded
    n, H, W, cin, cout = SHAPES[name]
    c = X.conv_case(n, H, W, cin, cout, ups=1, ax=1, seed=3)
    p = X.conv_problem(c)
    assert X.conv_bounds(c)[1] <= X.F16_EXACT
    x, b = p["x"].to(DEV), p["bias"].to(DEV)
    assert ops.conv2d_ups_folded_ok(n, H, W, cin, cout)
    with _forced(cfg):
        y = ops.conv2d_ups_folded(x, pack_conv_ups_folded(p["w"]).to(DEV), b)
        y9 = ops.conv2d(x, pack_conv(p["w"]).to(DEV), b, kh=3, kw=3, ups=1)
    torch.cuda.synchronize()
    X.assert_exact(y, p["ref"], f"folded {name} GEMM_CFG {cfg}")
    assert torch.equal(y, y9), f"{name} GEMM_CFG {cfg}: folded and nine-tap kernels differ on exact inputs"


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_random_data_is_one_rounding_of_its_own_weights(name, cfg, random_refs):
    from viewcrafter_amd import ops
    r = random_refs[name]
    with _forced(cfg):
        y = ops.conv2d_ups_folded(r["x"], r["wf"], r["b"])
    torch.cuda.synchronize()
    st = RQ.rounding_stats(y, r["orig"])
    print(f"\n[ups fold] {name} GEMM_CFG {cfg}: E against the ORIGINAL nine-tap weights {st['E']:.4f} (recorded, not bounded), rel-L2 {rel_l2(y, r['orig']):.3e}")
    RQ.RECORD.append(("conv_ups_folded_vs_original", f"{name}_cfg{cfg}", st["E"], None, st["mismatch"]))
    RQ.check_rounding("conv_ups_folded", f"{name}_cfg{cfg}", y, r["own"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_bits_do_not_depend_on_batch_or_configuration(name, random_refs):
    """A row's K order is fixed: image 0 at n = 1 equals image 0 of the whole batch, and every forced configuration gives the plan's bits."""
    from viewcrafter_amd import ops
    r = random_refs[name]
    base = ops.conv2d_ups_folded(r["x"], r["wf"], r["b"])
    one = ops.conv2d_ups_folded(r["x"][:1].contiguous(), r["wf"], r["b"])
    assert torch.equal(one[0], base[0]), "image 0 differs between n = 1 and the whole batch"
    for cfg in CFGS[1:]:
        with _forced(cfg):
            assert torch.equal(ops.conv2d_ups_folded(r["x"], r["wf"], r["b"]), base), f"GEMM_CFG {cfg} differs from the plan's result"
            assert torch.equal(ops.conv2d_ups_folded(r["x"][:1].contiguous(), r["wf"], r["b"])[0], base[0]), f"GEMM_CFG {cfg}, n = 1"


@pytest.mark.parametrize("cfg", CFGS)
def test_column_moments_and_concat_target(cfg, random_refs):
    """Output into columns [8, 8 + N) of a wider buffer (ldc > N), moments into columns [16, 16 + N) of a wider moment buffer
    (colstats_ld > N, colstats_col > 0): the values are those of the plain call, sentinels in the neighbouring columns, in the rows behind
    the output and in the strips behind the moments survive, and group_norm_stats_from_colstats of the written moments agrees with fp64
    statistics of the kernel's own fp16 output (tolerances of tests/test_kernels_gpu.py::test_conv_colstats_feed_the_groupnorm_behind_it)."""
    from viewcrafter_amd import ops
    name = "5x8x16_c128_n64"
    n, H, W, cin, cout = SHAPES[name]
    r = random_refs[name]
    M, ldc, cld, col, ccol = n * 4 * H * W, cout + 24, cout + 32, 8, 16
    assert ops.conv2d_ups_folded_ok(n, H, W, cin, cout, ldc=ldc, colstats=True)
    buf = torch.full((M + 64, ldc), SENTINEL, dtype=torch.float16, device=DEV)
    mom = torch.full((M // 64 + 4, cld, 2), SENTINEL, dtype=torch.float32, device=DEV)
    with _forced(cfg):
        plain = ops.conv2d_ups_folded(r["x"], r["wf"], r["b"])
        ops.conv2d_ups_folded(r["x"], r["wf"], r["b"], out=buf[:M, col:col + cout], ldc=ldc, colstats=mom[:M // 64], colstats_ld=cld, colstats_col=ccol)
        dense = ops.colstats_buffer(M, cout, DEV)
        y2 = ops.conv2d_ups_folded(r["x"], r["wf"], r["b"], colstats=dense)
    torch.cuda.synchronize()
    assert torch.equal(buf[:M, col:col + cout], plain.view(M, cout)) and torch.equal(y2, plain), "the output changes with its target / the moments"
    assert bool((buf[:M, :col] == SENTINEL).all()) and bool((buf[:M, col + cout:] == SENTINEL).all()) and bool((buf[M:] == SENTINEL).all())
    assert bool((mom[:, :ccol] == SENTINEL).all()) and bool((mom[:, ccol + cout:] == SENTINEL).all()) and bool((mom[M // 64:] == SENTINEL).all())
    own = mom[:M // 64, ccol:ccol + cout].contiguous()
    assert torch.equal(own, dense), "the moments depend on where they are written"
    stats = ops.group_norm_stats_from_colstats(own, n, 4 * H * W, cout)
    yd = plain.double().reshape(n, 4 * H * W, 32, cout // 32)
    mean, var = yd.mean(dim=(1, 3)), yd.var(dim=(1, 3), unbiased=False)
    dm, dv = float((stats[..., 0].double() - mean).abs().max()), rel_l2(stats[..., 1], var)
    print(f"\n[ups fold] column moments GEMM_CFG {cfg}: max |mean error| {dm:.2e}, variance rel-L2 {dv:.2e}")
    assert dm <= 2e-6 * float(mean.abs().max() + 1)
    assert dv <= 2e-5


def test_refused_shape_is_an_error_not_a_fallback():
    from viewcrafter_amd import ops
    from viewcrafter_amd._lib import VcxError
    x = torch.zeros((1, 8, 8, 64), dtype=torch.float16, device=DEV)                       # W % 16 != 0
    with pytest.raises(VcxError, match="folded upsample"):
        ops.conv2d_ups_folded(x, torch.zeros((4, 64, 256), dtype=torch.float16, device=DEV), None)


# ---------------------------------------------------------------- model level
def test_unet_fold_on_and_off_against_the_reference_golden(monkeypatch):
    """The tiny UNet at the 16x32 latent of tests/test_model_gpu.py::test_unet_forward_vs_reference_golden[shared]: its last Upsample has an
    8x16 source of 128 channels, which the route takes (the two deeper ones, 2x4 and 4x8, are refused: W % 16).  Fold on and off both meet
    UNET_TOL against the reference golden; they differ from each other by less than either differs from the golden.
    Measured: profiles/r11_ups_fold.md section 4."""
    from tests.test_gemm_units_gpu import _forward, _shared_inputs
    from tests.test_model_gpu import UNET_TOL
    from tests.tiny_config import TINY_UNET
    from tests.util import load_synth
    from viewcrafter_amd import ops
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    m = m.to(DEV)
    x, ctx, ts, fs, gold = _shared_inputs()
    answers, real_ok = [], ops.conv2d_ups_folded_ok
    monkeypatch.setattr(ops, "conv2d_ups_folded_ok", lambda *a, **k: answers.append(real_ok(*a, **k)) or answers[-1])
    monkeypatch.setattr(ops, "UPS_FOLD", True)
    y_on = _forward(m, x, ctx, ts, fs)
    assert any(answers), f"no Upsample layer took the folded route: {answers}"
    folded = sum(answers)
    answers.clear()
    monkeypatch.setattr(ops, "UPS_FOLD", False)
    y_off = _forward(m, x, ctx, ts, fs)
    assert answers and not any(answers)
    e_on, e_off, d = rel_l2(y_on, gold), rel_l2(y_off, gold), rel_l2(y_on, y_off)
    print(f"\n[ups fold] tiny UNet, {folded} layer(s) folded: rel-L2 vs reference golden on {e_on:.3e} off {e_off:.3e}; on against off {d:.3e}")
    assert e_on <= UNET_TOL and e_off <= UNET_TOL
    assert d < min(e_on, e_off)
    monkeypatch.setattr(ops, "UPS_FOLD", True)
    y01 = torch.cat([_forward(m, x, ctx, ts, fs, slice(0, 1)), _forward(m, x, ctx, ts, fs, slice(1, 2))])
    assert torch.equal(y_on, y01), "fold on: the B = 2 forward differs from two B = 1 forwards"
