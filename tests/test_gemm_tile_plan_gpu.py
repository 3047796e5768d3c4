"""The tile plan of the DMA GEMM engine (csrc/gemm.hip plan_tiles) and the 64-row tail configurations (knob GEMM_CFG 4, 5, 6).

The tile shape does not enter a row's arithmetic: the plan's output (GEMM_CFG = -1) and every forced tail configuration must be
torch.equal to ONE forced 128-row configuration (1 where N % 160 == 0, else / GEGLU 0) - outputs and, for COLSTATS, the column
moments.  Shapes are sized from the device's CU count so that the problem has whole rounds of large tiles plus a remainder: the
three forms of a badly filled last round (a few left-over row tiles, a remainder just above one round of small tiles, 1.77 rounds).
K is 128 ... 640: every case is a few launches of well under a millisecond.
"""
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rnd(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale + offset


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _under_each(run, ref_cfg, new_cfgs, capfd=None):
    """run() under the forced reference configuration, under the plan and under each forced tail configuration.  Returns
    (reference, {cfg: result}, the plan's segments as [(cfg, m_begin, rows, grid)]) - results are tuples of tensors."""
    from viewcrafter_amd import ops
    got, segs = {}, []
    try:
        ops.tune_set("GEMM_CFG", ref_cfg)
        ref = run()
        torch.cuda.synchronize()
        for cfg in (-1, *new_cfgs):
            ops.tune_set("GEMM_CFG", cfg)
            if cfg == -1 and capfd is not None:
                capfd.readouterr()
                os.environ["VCX_GEMM_PLAN_TRACE"] = "1"
            try:
                got[cfg] = run()
                torch.cuda.synchronize()
            finally:
                if cfg == -1 and capfd is not None:
                    os.environ.pop("VCX_GEMM_PLAN_TRACE", None)
                    err = capfd.readouterr().err
                    segs = [tuple(int(v) for v in m) for m in re.findall(r"cfg (\d+) rows (\d+)\+(\d+) grid (\d+)", err)]
    finally:
        ops.tune_set("GEMM_CFG", -1)
    return ref, got, segs


def _assert_equal(ref, got, what):
    for cfg, res in got.items():
        for i, (r, g) in enumerate(zip(ref, res)):
            assert torch.equal(r, g), f"{what}: GEMM_CFG {cfg} output {i}: {int((r != g).sum())} of {r.numel()} elements differ from the reference configuration"


def _assert_covers(segs, M):
    """Whatever the plan chose: one or two launches whose row ranges tile [0, M) in order, the first one on large tiles when there are two."""
    assert 1 <= len(segs) <= 2, segs
    assert segs[0][1] == 0 and segs[-1][1] + segs[-1][2] == M, segs
    if len(segs) == 2:
        assert segs[0][0] in (2, 3) and segs[1][1] == segs[0][2] and segs[1][1] % 256 == 0, segs
    assert all(g >= 1 for (_, _, _, g) in segs), segs


def _rows_tiny_tail():
    return (2 * _ncu() + 8) * 256 - 37            # N = 320: two whole rounds of 256 x 320 tiles + 8 row tiles, ragged


@pytest.mark.parametrize("variant", ["plain", "bias+res"])
def test_linear_320_tiny_tail(variant, capfd):
    from viewcrafter_amd import ops
    M, N, K = _rows_tiny_tail(), 320, 128
    x = _rnd((M, K), 1).half()
    w = (_rnd((N, K), 2) / math.sqrt(K)).half()
    b = _rnd((N,), 3, 0.1) if variant != "plain" else None
    res = _rnd((M, N), 4, 0.5).half() if variant != "plain" else None
    ref, got, segs = _under_each(lambda: (ops.linear(x, w, b, residual=res),), 1, (4, 5), capfd)
    print(f"linear {M}x{N}x{K} {variant}: plan {segs}")
    _assert_equal(ref, got, f"linear {M}x{N}x{K} {variant}")
    _assert_covers(segs, M)
    # the split is really taken: whole rounds of large tiles, then the 8 left-over row tiles (a quarter-filled round of large tiles
    # costs a whole one under any cost table)
    assert len(segs) == 2 and segs[0][0] == 3 and segs[0][2] == 2 * _ncu() * 256 and segs[1][1] == segs[0][2] and segs[1][1] + segs[1][2] == M, segs


def test_linear_320_guard_band_stays_untouched():
    """Rows >= M and columns >= N of a wider / taller output buffer: no configuration writes them (ragged M: the last tile of every
    configuration hangs over the end)."""
    from viewcrafter_amd import ops
    M, N, K = _rows_tiny_tail(), 320, 128
    x = _rnd((M, K), 1).half()
    w = (_rnd((N, K), 2) / math.sqrt(K)).half()
    for cfg in (-1, 4, 5):
        buf = torch.full((M + 256, N + 64), 77.0, dtype=torch.float16, device=DEV)
        ops.tune_set("GEMM_CFG", cfg)
        try:
            ops.linear(x, w, None, out=buf[:M, :N])
            torch.cuda.synchronize()
        finally:
            ops.tune_set("GEMM_CFG", -1)
        assert bool((buf[M:] == 77.0).all()) and bool((buf[:, N:] == 77.0).all()), f"GEMM_CFG {cfg} wrote outside its [M, N] block"
        assert bool((buf[:M, :N] != 77.0).any())


def test_linear_640_remainder_just_above_one_round_of_small_tiles(capfd):
    from viewcrafter_amd import ops
    ncu = _ncu()
    tiles_m = (2 * ncu + ncu // 2 + 4) // 2       # 256 x 320 tiles: two per row tile; remainder ~ ncu / 2 + 4 large = 4x as many 128 x 160 tiles
    M, N, K = tiles_m * 256 - 37, 640, 128
    x = _rnd((M, K), 5).half()
    w = (_rnd((N, K), 6) / math.sqrt(K)).half()
    b = _rnd((N,), 7, 0.1)
    ref, got, segs = _under_each(lambda: (ops.linear(x, w, b),), 1, (4, 5), capfd)
    print(f"linear {M}x{N}x{K}: plan {segs}")
    _assert_equal(ref, got, f"linear {M}x{N}x{K}")
    _assert_covers(segs, M)


def test_linear_1280_unsplit_one_and_three_quarter_rounds(capfd):
    from viewcrafter_amd import ops
    tiles_m = max(1, round(452 * _ncu() / 256 / 4))      # 113 row tiles x 4 column tiles of 256 x 320 at 256 CUs
    M, N, K = tiles_m * 256 - 128, 1280, 192
    x = _rnd((M, K), 8).half()
    w = (_rnd((N, K), 9) / math.sqrt(K)).half()
    b = _rnd((N,), 10, 0.1)
    res = _rnd((M, N), 11, 0.5).half()
    ref, got, segs = _under_each(lambda: (ops.linear(x, w, b, residual=res),), 1, (4, 5), capfd)
    print(f"linear {M}x{N}x{K}: plan {segs}")
    _assert_equal(ref, got, f"linear {M}x{N}x{K}")
    _assert_covers(segs, M)


def _conv_frames():
    return ((2 * _ncu() + 8) * 256 + 959) // 960      # frames of 24 x 40: the boundary after two rounds of row tiles is no multiple of 40


@pytest.mark.parametrize("kind", ["conv3x3", "conv3x3+tail", "conv3x3+colstats"])
def test_conv3x3_tail_boundary_inside_an_image_row(kind, capfd):
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv
    n, H, W, C, N = _conv_frames(), 24, 40, 64, 320
    M = n * H * W
    assert (2 * _ncu() * 256) % W != 0 and M % 64 == 0
    x = _rnd((n, H, W, C), 12).half()
    w = pack_conv(_rnd((N, C, 3, 3), 13).cpu() / math.sqrt(9 * C)).to(DEV).half()
    b = _rnd((N,), 14, 0.1)
    kw = {}
    if kind == "conv3x3+tail":
        kw["tail"] = [_rnd((M, 64), 15).half()]
        w = torch.cat([w, (_rnd((N, 64), 16) / 8).half()], dim=1).contiguous()

    def run():
        if kind == "conv3x3+colstats":
            cs = ops.colstats_buffer(M, N, DEV)
            return ops.conv2d(x, w, b, kh=3, kw=3, colstats=cs), cs
        return (ops.conv2d(x, w, b, kh=3, kw=3, **kw),)
    ref, got, segs = _under_each(run, 1, (4, 5), capfd)
    print(f"{kind} M={M}: plan {segs}")
    _assert_equal(ref, got, kind)
    _assert_covers(segs, M)
    assert len(segs) == 2 and segs[1][1] % 64 == 0 and segs[1][1] % W != 0, segs


def test_temporal_conv_3_1_1(capfd):
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_conv
    T, C, N = 5, 64, 320
    P = ((2 * _ncu() + 8) * 256 + T - 1) // T // 8 * 8 + 8
    x = _rnd((1, T, P, C), 17).half()
    w = pack_conv(_rnd((N, C, 3, 1, 1), 18).cpu() / math.sqrt(3 * C)).to(DEV).half()
    b = _rnd((N,), 19, 0.1)
    ref, got, segs = _under_each(lambda: (ops.temporal_conv3(x, w, b),), 1, (4, 5), capfd)
    print(f"tconv M={T * P}: plan {segs}")
    _assert_equal(ref, got, "(3,1,1) convolution")
    _assert_covers(segs, T * P)


def test_linear_colstats_moments_are_the_same_bits(capfd):
    from viewcrafter_amd import ops
    M, N, K = (2 * _ncu() + 8) * 256, 320, 128
    x = _rnd((M, K), 20).half()
    w = (_rnd((N, K), 21) / math.sqrt(K)).half()
    b = _rnd((N,), 22, 0.1, 2.0)
    res = _rnd((M, N), 23, 0.5).half()

    def run():
        cs = ops.colstats_buffer(M, N, DEV)
        return ops.linear(x, w, b, residual=res, colstats=cs), cs
    ref, got, segs = _under_each(run, 1, (4, 5), capfd)
    print(f"linear+colstats {M}x{N}x{K}: plan {segs}")
    _assert_equal(ref, got, "linear + COLSTATS")
    _assert_covers(segs, M)
    assert len(segs) == 2 and segs[1][1] % 64 == 0, segs      # a moment strip is 64 rows of ONE configuration


def test_geglu_projection(capfd):
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import pack_geglu
    ncu = _ncu()
    tiles_m = (2 * ncu + 40 + 4) // 5                    # 256 x 256 tiles, 5 per row tile: two rounds + ~40
    M, C = tiles_m * 256 - 37, 160
    x = _rnd((M, 128), 24).half()
    wp, bp = pack_geglu(_rnd((8 * C, 128), 25) / math.sqrt(128), _rnd((8 * C,), 26))
    wp = wp.half()
    ref, got, segs = _under_each(lambda: (ops.linear(x, wp, bp, geglu=True),), 0, (6,), capfd)
    print(f"geglu {M}x{8 * C}x128: plan {segs}")
    _assert_equal(ref, got, "GEGLU")
    _assert_covers(segs, M)


def test_lnfold_projection(capfd):
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import fold_layernorm
    ncu = _ncu()
    M, N, K = (2 * ncu + 12) // 2 * 256 - 37 + 1, 640, 128      # 256 x 320 tiles, two per row tile: two rounds + 12
    x = _rnd((M, K), 27, 2.0).half()
    wf, cs, bf = fold_layernorm(_rnd((N, K), 28) / math.sqrt(K), 1 + 0.3 * _rnd((K,), 29), 0.2 * _rnd((K,), 30), _rnd((N,), 31))
    st = ops.row_stats(x, 1e-5)
    ref, got, segs = _under_each(lambda: (ops.linear(x, wf, bf, ln_stats=st, ln_colsum=cs),), 1, (4, 5), capfd)
    print(f"lnfold {M}x{N}x{K}: plan {segs}")
    _assert_equal(ref, got, "LNFOLD")
    _assert_covers(segs, M)
