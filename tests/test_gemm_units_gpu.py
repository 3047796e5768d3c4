"""vcx_gemm_units_f16 on the tiled engine: all units of a call under ONE tile plan (csrc/gemm_dma.hip UNITS, csrc/gemm.hip).

The tile shape does not enter a row's arithmetic (tests/test_gemm_tile_plan_gpu.py), so the grouped launch must be torch.equal to what it
replaces: the unit-by-unit loop (VCX_GEMM_UNITS_LOOP=1) and ops.linear on each unit with that unit's weights - under the plan and under
every forced tile configuration 0-5 (6 is the GEGLU configuration: no plain epilogue, refused for a linear layer before and after).
Every run writes into a [M + 256, N + 64] buffer filled with a sentinel: nothing outside [M, N] may change.  Tolerance against fp32:
the one tests/test_kernels_gpu.py uses for a plain linear layer (check_rows' default, rel-L2 <= 2e-3).
"""
import math
import os
import re

import pytest
import torch

from tests.test_kernels_gpu import check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 77.0
CFGS = (-1, 0, 1, 2, 3, 4, 5)

# (units, unit_rows, N, K, lda - K, name)
SHAPES = [
    (3, 3600, 640, 128, 0, "ragged against 256, 128 and 64"),
    (6, 3600, 1280, 1280, 0, "level 3, k = 3 clip batching with CFG, long K"),
    (2, 57600, 640, 640, 0, "level 1 under CFG, whole tiles"),
    (50, 576, 1280, 128, 0, "per-frame units, level 3"),
    (50, 2304, 640, 64, 0, "per-frame units, level 2"),
    (7, 200, 128, 64, 0, "units below a 256-row tile"),
    (9, 40, 64, 64, 0, "units below every tile"),
    (5, 1000, 328, 64, 0, "N % 8 == 0, no multiple of a tile width"),
    (4, 1000, 192, 128, 64, "lda > K"),
]


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale


def _problem(units, unit_rows, N, K, pad, seed=0):
    M = units * unit_rows
    xb = _rnd((M, K + pad), 100 + seed).half()
    x = xb[:, :K]                                                  # row stride K + pad
    wn = (_rnd((units, N, K), 101 + seed) / math.sqrt(K)).half()   # a different weight and bias set per unit
    bn = _rnd((units, N), 102 + seed)
    return M, x, wn, bn


def _grouped(x, wn, bn, unit_rows, loop=False):
    """gemm_units into a sentinel-filled [M + 256, N + 64] buffer -> (the [M, N] block, the buffer)."""
    from viewcrafter_amd import ops
    M, N = x.shape[0], wn.shape[1]
    buf = torch.full((M + 256, N + 64), SENTINEL, dtype=torch.float16, device=DEV)
    if loop:
        os.environ["VCX_GEMM_UNITS_LOOP"] = "1"
    try:
        ops.gemm_units(x, wn, bn, unit_rows=unit_rows, out=buf[:M, :N])
        torch.cuda.synchronize()
    finally:
        os.environ.pop("VCX_GEMM_UNITS_LOOP", None)
    return buf[:M, :N], buf


def _per_unit(x, wn, bn, unit_rows):
    from viewcrafter_amd import ops
    return torch.cat([ops.linear(x[u * unit_rows:(u + 1) * unit_rows], wn[u], bn[u]) for u in range(wn.shape[0])])


def _fp32_rows(x, wn, bn, unit_rows):
    def rows(r0, r1):
        parts, r = [], r0
        while r < r1:
            u = r // unit_rows
            e = min(r1, (u + 1) * unit_rows)
            parts.append(x[r:e].float() @ wn[u].float().t() + bn[u])
            r = e
        return torch.cat(parts)
    return rows


@pytest.mark.parametrize("units,unit_rows,N,K,pad,what", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in SHAPES])
def test_grouped_equals_loop_and_per_unit_linear(units, unit_rows, N, K, pad, what):
    from viewcrafter_amd import ops
    M, x, wn, bn = _problem(units, unit_rows, N, K, pad)
    ref_rows = _fp32_rows(x, wn, bn, unit_rows)
    try:
        for cfg in CFGS:
            ops.tune_set("GEMM_CFG", cfg)
            out, buf = _grouped(x, wn, bn, unit_rows)
            name = f"{units} x {unit_rows} rows, N {N}, K {K} ({what}), GEMM_CFG {cfg}"
            assert bool((buf[M:] == SENTINEL).all()) and bool((buf[:, N:] == SENTINEL).all()), f"{name}: wrote outside its [M, N] block"
            per_unit = _per_unit(x, wn, bn, unit_rows)
            assert torch.equal(out, per_unit), f"{name}: {int((out != per_unit).sum())} of {out.numel()} elements differ from ops.linear unit by unit"
            loop, lbuf = _grouped(x, wn, bn, unit_rows, loop=True)
            assert torch.equal(out, loop), f"{name}: {int((out != loop).sum())} of {out.numel()} elements differ from the unit-by-unit loop"
            assert bool((lbuf[M:] == SENTINEL).all()) and bool((lbuf[:, N:] == SENTINEL).all())
            e = check_rows(out, ref_rows, name=name)
            if cfg == -1:
                print(f"{name}: rel-L2 vs fp32 {e:.3e}")
    finally:
        ops.tune_set("GEMM_CFG", -1)


def test_first_row_of_each_unit_uses_its_own_weights():
    """3 x 3600 rows: 3600 = 14 x 256 + 16 = 28 x 128 + 16 = 56 x 64 + 16, so the last tile of a unit hangs over the next unit's first rows
    under every configuration.  Those rows must carry the next unit's weights, not the overhanging tile's."""
    from viewcrafter_amd import ops
    units, R, N, K = 3, 3600, 640, 128
    M, x, wn, bn = _problem(units, R, N, K, 0)
    try:
        for cfg in CFGS:
            ops.tune_set("GEMM_CFG", cfg)
            out, _ = _grouped(x, wn, bn, R)
            for u in range(1, units):
                own = ops.linear(x[u * R:u * R + 16], wn[u], bn[u])
                prev = ops.linear(x[u * R:u * R + 16], wn[u - 1], bn[u - 1])
                assert not torch.equal(own, prev)
                assert torch.equal(out[u * R:u * R + 16], own), f"GEMM_CFG {cfg}: the first rows of unit {u} are not computed with its weights"
                assert not torch.equal(out[u * R:u * R + 16], prev), f"GEMM_CFG {cfg}: the first rows of unit {u} carry unit {u - 1}'s weights"
    finally:
        ops.tune_set("GEMM_CFG", -1)


def _traced(capfd, run):
    capfd.readouterr()
    os.environ["VCX_GEMM_PLAN_TRACE"] = "1"
    try:
        out = run()
        torch.cuda.synchronize()
    finally:
        os.environ.pop("VCX_GEMM_PLAN_TRACE", None)
    return out, [l for l in capfd.readouterr().err.splitlines() if "gemm plan" in l]


@pytest.mark.parametrize("units,unit_rows,N,K", [(3, 3600, 640, 128), (50, 576, 1280, 128)])
def test_all_units_run_under_one_plan(units, unit_rows, N, K, capfd):
    """One plan for the whole call: at most two segment lines, each ending in `units <U> unit_rows <R>` (the units of that segment), their
    row ranges tiling [0, M) in order.  (The unit-by-unit loop prints one plan per unit and no units field.)"""
    from viewcrafter_amd import ops
    M, x, wn, bn = _problem(units, unit_rows, N, K, 0)
    _, lines = _traced(capfd, lambda: ops.gemm_units(x, wn, bn, unit_rows=unit_rows))
    print("\n".join(lines))
    assert 1 <= len(lines) <= 2, lines
    at, seen = 0, 0
    for l in lines:
        m = re.search(r"cfg (\d+) rows (\d+)\+(\d+) grid (\d+) units (\d+) unit_rows (\d+)$", l)
        assert m, f"no `units <U> unit_rows <R>` at the end of: {l}"
        _, m_begin, rows, grid, u, r = (int(v) for v in m.groups())
        assert m_begin == at and r == unit_rows and rows == u * unit_rows and u >= 1 and grid >= 1, l
        at += rows
        seen += u
    assert at == M and seen == units, lines


def test_n_k_320_keeps_the_weight_stationary_route(capfd):
    """N = K = 320, 8 units of 1024 rows: the weight-stationary one-launch form keeps priority - no tile plan is printed - and its bits
    are those of each unit on its own."""
    from viewcrafter_amd import ops
    M, x, wn, bn = _problem(8, 1024, 320, 320, 0)
    assert ops.units_route(M, 320, 320, 1024) == "ws320"
    out, lines = _traced(capfd, lambda: ops.gemm_units(x, wn, bn, unit_rows=1024))
    assert not any("units" in l for l in lines), lines
    assert torch.equal(out, _per_unit(x, wn, bn, 1024))


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_soak_every_new_instantiation(cfg):
    """50 calls on one input under each tile configuration of the per-unit form: every result the same bits."""
    from viewcrafter_amd import ops
    M, x, wn, bn = _problem(5, 1000, 328, 128, 0, seed=7)
    try:
        ops.tune_set("GEMM_CFG", cfg)
        first = ops.gemm_units(x, wn, bn, unit_rows=1000)
        for i in range(49):
            again = ops.gemm_units(x, wn, bn, unit_rows=1000)
            assert torch.equal(first, again), f"GEMM_CFG {cfg}: call {i + 2} differs in {int((first != again).sum())} elements"
    finally:
        ops.tune_set("GEMM_CFG", -1)


# ---------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def unet():
    from tests.tiny_config import TINY_UNET
    from tests.util import load_synth
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    return m.to(DEV)


def _shared_inputs():
    """The B = 2 forward of tests/test_model_gpu.py::test_unet_forward_vs_reference_golden[shared] and its golden."""
    from oracle.weights import synth_input
    from tests.tiny_config import TINY_UNET
    from tests.util import golden
    b, t, h, w, L = 2, 3, 16, 32, 77 + 40
    x = synth_input("unet_x_shared", (b, 8, t, h, w)).to(DEV)
    ctx = synth_input("unet_ctx_shared", (b, L, TINY_UNET["context_dim"])).to(DEV)
    ts, fs = torch.tensor([999, 399], device=DEV), torch.tensor([10, 3], device=DEV)
    return x, ctx, ts, fs, golden("unet_tiny")["unet_out_shared"]


def _forward(m, x, ctx, ts, fs, sl=slice(None)):
    with torch.no_grad():
        y = m(x[sl], ts[sl], context=ctx[sl].contiguous(), fs=fs[sl])
    torch.cuda.synchronize()
    return y


def test_unet_b2_grouped_equals_loop_and_two_b1_forwards(unet, monkeypatch):
    """The temporal fold at every level (GN_FOLD_MIN_BYTES = 0): B = 2 puts two videos under one tile plan.  Same bits as the loop and as
    two B = 1 forwards (one unit: vcx_gemm_f16)."""
    from viewcrafter_amd.lvdm.modules import attention as A
    monkeypatch.setattr(A, "GN_FOLD_MIN_BYTES", 0)
    x, ctx, ts, fs, _ = _shared_inputs()
    y = _forward(unet, x, ctx, ts, fs)
    monkeypatch.setenv("VCX_GEMM_UNITS_LOOP", "1")
    y_loop = _forward(unet, x, ctx, ts, fs)
    monkeypatch.delenv("VCX_GEMM_UNITS_LOOP")
    assert torch.equal(y, y_loop), "B = 2 forward: the grouped route differs from the unit-by-unit loop"
    y01 = torch.cat([_forward(unet, x, ctx, ts, fs, slice(0, 1)), _forward(unet, x, ctx, ts, fs, slice(1, 2))])
    assert torch.equal(y, y01), "B = 2 forward differs from two B = 1 forwards"


def test_unet_spatial_fold_opt_in(unet, monkeypatch):
    """GN_FOLD_SPATIAL = 2: SpatialTransformer.norm folded into proj_in at every width (unit = frame).  Rounding changes, so the bound is the
    one tests/test_model_gpu.py asserts for this forward against its golden (UNET_TOL); B = 2 still equals two B = 1 forwards bit for bit."""
    from tests.test_model_gpu import UNET_TOL
    from tests.util import rel_l2
    from viewcrafter_amd.lvdm.modules import attention as A
    monkeypatch.setattr(A, "GN_FOLD_MIN_BYTES", 0)
    x, ctx, ts, fs, gold = _shared_inputs()
    y_default = _forward(unet, x, ctx, ts, fs)
    monkeypatch.setattr(A, "GN_FOLD_SPATIAL", 2)
    assert A.spatial_fold_ok(3, 16 * 32, 64, 64) and A.spatial_fold_ok(3, 8, 256, 256)      # taken at every level of the tiny graph
    y = _forward(unet, x, ctx, ts, fs)
    e = rel_l2(y, gold)
    print(f"unet shared, spatial fold opt-in: rel-L2 vs reference golden {e:.3e} (default route {rel_l2(y_default, gold):.3e})")
    assert e <= UNET_TOL
    assert not torch.equal(y, y_default), "the opt-in changed nothing: the spatial fold was not taken"
    y01 = torch.cat([_forward(unet, x, ctx, ts, fs, slice(0, 1)), _forward(unet, x, ctx, ts, fs, slice(1, 2))])
    assert torch.equal(y, y01), "opt-in: B = 2 forward differs from two B = 1 forwards"
