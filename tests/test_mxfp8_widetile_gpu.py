"""The 128 x 160 tile configuration of the MXFP8 GEMM kernel (csrc/gemm_mx.hip Cfg160; include/vcx.h vcx_gemm_mxfp8_cfg) on the GPU.  The tile
shape must not enter a row's arithmetic: VCX_GEMM_MX_CFG=1 (the wide tile wherever it exists) gives the bytes of VCX_GEMM_MX_CFG=0 (128 x
128 everywhere) for every epilogue of the three entry points - output, guard bands and column moments -, matches the fp64 value of exactly
summable operands, addresses outputs past 2^31 bytes, and the rule (knob unset) leaves a ResBlock at width 320 bit-identical.  The knob is
read once per process, so tests/mxfp8_widetile_cases.py runs in one child process per knob value (three in all, shared by the tests)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import mx_emulation as MX
from tests import mxfp8_widetile_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(path, groups, **env_extra):
    env = {k: v for k, v in os.environ.items() if k != "VCX_GEMM_MX_CFG"}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-m", "tests.mxfp8_widetile_cases", str(path), groups], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(str(path))


MX_ON = dict(VCX_RESCONV_MXFP8="1", VCX_TCONV_MXFP8="1", VCX_TCONV_MXFP8_SKIP_DIMS="", VCX_RESCONV_MXFP8_SKIP_DIMS="")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("widetile")
    return {"0": _child(d / "cfg0.pt", "bytes,extent,graph", VCX_GEMM_MX_CFG="0", **MX_ON),
            "1": _child(d / "cfg1.pt", "bytes,exact,extent", VCX_GEMM_MX_CFG="1"),
            "rule": _child(d / "rule.pt", "graph", **MX_ON)}


def _same(a, b, name):
    assert a.shape == b.shape and a.dtype == b.dtype, name
    same = torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == torch.float16 else torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same, f"{name}: {int((a != b).sum())} of {a.numel()} elements differ between the tile configurations"


# ------------------------------------------------------------------------------------------------------------------ a. byte equality
@pytest.mark.parametrize("call", ["linear", "t3", "c9"])
def test_wide_tile_gives_the_bytes_of_the_square_tile(runs, call):
    narrow, wide = runs["0"], runs["1"]
    names = [k for k in narrow if k.startswith(call + " ")]
    want = {"linear": len(C.NS) * len(C.KS) * len(C.MS) * 2, "t3": len(C.NS) * 3 * 2 * 2 - len(C.NS) * 2, "c9": len(C.NS) * (7 + 4)}[call]
    assert len(names) == want and sorted(names) == sorted(k for k in wide if k.startswith(call + " "))
    for k in names:
        a, b = narrow[k], wide[k]
        _same(a, b, k)
        N = int(k.split(" N")[1].split()[0])
        if k.endswith("moments"):
            # [strips, N + 64, 2] with this call's columns at 32 .. 32 + N: written and finite there, untouched around
            assert bool((b[:, :32] == 5.0).all()) and bool((b[:, 32 + N:] == 5.0).all()), f"{k}: moments written outside their columns"
            assert bool(torch.isfinite(b[:, 32:32 + N]).all()) and not bool((b[:, 32:32 + N, 0] == 5.0).all()), f"{k}: moments not written"
        else:
            # [M + 2, N + 24]: a guard row in front and behind, 24 guard columns behind column N
            assert bool((b[0] == C.GUARD).all()) and bool((b[-1] == C.GUARD).all()) and bool((b[:, N:] == C.GUARD).all()), f"{k}: a guard element was written"
            assert bool(torch.isfinite(b).all()) and not bool((b[1:-1, :N] == C.GUARD).any()), f"{k}: an output element was not written"
            assert float(b[1:-1, :N].float().abs().max()) > 0.1, k


# ------------------------------------------------------------------------------------------------------------------ b. exact tier
def _shift_t(a, tau):
    out = torch.zeros_like(a)
    if tau == 0:
        out[:, 1:] = a[:, :-1]
    elif tau == 1:
        out.copy_(a)
    else:
        out[:, :-1] = a[:, 1:]
    return out


def _shift_yx(a, ky, kx):
    n, H, W, _ = a.shape
    out = torch.zeros_like(a)
    dy, dx = ky - 1, kx - 1
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[:, yd, xd] = a[:, ys, xs]
    return out


def _exact_ref(mode):
    """fp64 value of the stored operands of tests/mxfp8_widetile_cases.exact_problems, and the number of taps"""
    N = C.EXACT_N
    (_, _, a), (_, ws, w), bias, res, rowadd = C.exact_problems()[mode]
    M, cin = a.shape
    taps = {"linear": 1, "t3": 3, "c9": 9}[mode]
    w = w.view(N, taps, cin)
    ref = bias.double().unsqueeze(0).expand(M, -1).clone() + res.double()
    if mode == "linear":
        ref += a @ w[:, 0].t()
    elif mode == "t3":
        B, T, P, _ = C.EXACT_T3
        for tau in range(3):
            ref += _shift_t(a.view(B, T, P, cin), tau).reshape(M, cin) @ w[:, tau].t()
    else:
        n, H, W, _ = C.EXACT_C9
        for tap in range(9):
            ref += _shift_yx(a.view(n, H, W, cin), tap // 3, tap % 3).reshape(M, cin) @ w[:, tap].t()
        ref += rowadd.double()[torch.arange(M) // (H * W)]
    return ref, ws.view(N, -1), taps, cin


@pytest.mark.parametrize("mode", ["linear", "t3", "c9"])
def test_wide_tile_is_exact_on_the_integer_grid(runs, mode):
    """Conditions on the inputs, not tolerances: every product is a multiple of 2^-2 of magnitude <= 21 x 2^5, so every partial sum in any order
    (bias, addend and residual included) is a multiple of 2^-2 below 2^24 x 2^-2 and exact in fp32; |ref| < 65504.  The weight scale bytes of
    the rows of the second scale-DMA pass (columns 128 .. 159 of a tile) are 128 .. 130, all others 125 .. 127."""
    ref, ws, taps, cin = _exact_ref(mode)
    product_max = 7 * C.W_ELEM_MAX * 2 ** 5
    assert taps * cin * product_max + 3 * 64 < (1 << 24) * MX.GRID
    assert float(ref.abs().max()) < 65504 and torch.equal(ref / MX.GRID, (ref / MX.GRID).round())
    hi = (torch.arange(C.EXACT_N) % 160) >= 128
    used = ws.view(C.EXACT_N, taps, -1)[:, :, :cin // 32]          # (a tap's K padding carries scale byte 127 in every row)
    assert int(used[hi].min()) >= 128 and int(used[~hi].max()) <= 127 and int(hi.sum()) == 64
    got, want = runs["1"][f"exact {mode}"], ref.half()
    assert got.dtype == torch.float16 and got.shape == want.shape
    bad = torch.nonzero(got.view(torch.int16) != want.view(torch.int16))
    assert bad.shape[0] == 0, f"{mode}: {bad.shape[0]} of {got.numel()} differ from the fp64 reference, first at {bad[0].tolist()}"


# ------------------------------------------------------------------------------------------------------------------ c. extent
def test_wide_tile_addresses_outputs_beyond_2_gib(runs):
    M, N, K, ldc = C.EXTENT
    assert (M - 1) * ldc * 2 > 1 << 31
    narrow, wide = runs["0"], runs["1"]
    for part in ("first tile", "last tile"):
        a, b = narrow[f"extent {part}"], wide[f"extent {part}"]
        _same(a, b, f"extent {part}")
        assert bool((b[:, N:] == C.GUARD).all()) and bool(torch.isfinite(b).all()) and not bool((b[:, :N] == C.GUARD).any()), part
    assert not torch.equal(wide["extent first tile"], wide["extent last tile"])
    assert bool((wide["extent guard behind row 4096"] == C.GUARD).all()) and bool((narrow["extent guard behind row 4096"] == C.GUARD).all())


# ------------------------------------------------------------------------------------------------------------------ d. host graph
def test_resblock_at_width_320_is_bit_identical_under_the_rule(runs):
    rule, narrow = runs["rule"], runs["0"]
    assert rule["graph cfg"].tolist() == [1, 1] and narrow["graph cfg"].tolist() == [0, 0], "the rule takes the wide tile at N = 320, the knob's 0 does not"
    assert rule["graph mx packs"].tolist() == [2, 4] == narrow["graph mx packs"].tolist(), "both convolutions and the temporal block ran on the MX route"
    assert bool(torch.isfinite(rule["graph B=2"]).all())
    _same(rule["graph B=2"], narrow["graph B=2"], "ResBlock(320), knob unset against VCX_GEMM_MX_CFG=0")
    _same(rule["graph B=2"], rule["graph 2 x B=1"], "ResBlock(320), B = 2 against two B = 1 calls")
