"""vcx_gemm_mxfp8_cfg (include/vcx.h, ABI 18) without a GPU: the tile configuration the three MXFP8 GEMM launchers switch on, asked directly -
the rule's table, the environment knob VCX_GEMM_MX_CFG (read once per process: each value gets a process of its own), and the shape
predicates, whose answers the second configuration must not have moved."""
import json
import os
import re
import subprocess
import sys

import pytest

from viewcrafter_amd import _lib

G = _lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIAS = G.GEMM_BIAS_N
RES, ROW, CS = G.GEMM_RESIDUAL, G.GEMM_ROWADD, G.GEMM_COLSTATS
LINEAR_FLAGS = [BIAS, BIAS | RES]
T3_FLAGS = [BIAS, BIAS | RES, BIAS | CS, BIAS | RES | CS]
C9_FLAGS = T3_FLAGS + [BIAS | ROW, BIAS | ROW | CS, BIAS | ROW | RES, BIAS | ROW | RES | CS]
GEGLU_FLAGS = [BIAS | G.GEMM_GEGLU, BIAS | G.GEMM_GEGLU | G.GEMM_MXFP8_OUT]
WIDE_N = [160, 320, 480, 960, 800]
SQUARE_N = [128, 640, 1280, 1920, 2560]
RAGGED_N = [200, 8, 136, 328]
QUERIES = [(N, f, gm) for gm, fl in ((0, LINEAR_FLAGS + GEGLU_FLAGS), (1, T3_FLAGS), (2, C9_FLAGS)) for f in fl for N in WIDE_N + SQUARE_N + RAGGED_N]

_CHILD = ("import json, sys; from viewcrafter_amd import _lib; L = _lib.lib(); "
          "print('ANSWERS', json.dumps([L.vcx_gemm_mxfp8_cfg(*q) for q in json.loads(sys.argv[1])]))")


def _answers(knob):
    """vcx_gemm_mxfp8_cfg of every query in a fresh process with VCX_GEMM_MX_CFG = knob (None: unset)"""
    env = {k: v for k, v in os.environ.items() if k != "VCX_GEMM_MX_CFG"}
    if knob is not None:
        env["VCX_GEMM_MX_CFG"] = knob
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(QUERIES)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(zip(QUERIES, json.loads(re.search(r"ANSWERS (.*)", r.stdout).group(1))))


def test_abi_is_18_in_header_library_and_binding():
    src = open(os.path.join(ROOT, "include", "vcx.h")).read()
    assert int(re.search(r"#define VCX_ABI_VERSION (\d+)", src).group(1)) == 18
    assert _lib.ABI_VERSION == 18 and _lib.lib().vcx_abi_version() == 18
    assert "vcx_gemm_mxfp8_cfg" in _lib.SYMBOLS and re.search(r"int vcx_gemm_mxfp8_cfg\(int64_t N, int flags, int gather_mode\);", src)


def test_rule_is_wide_iff_n_is_whole_tiles_of_160_and_not_of_128():
    got = _answers(None)
    for (N, f, gm), cfg in got.items():
        plain = f not in GEGLU_FLAGS
        assert cfg == (1 if plain and N in WIDE_N else 0), f"N={N} flags=0x{f:x} gather_mode={gm}: configuration {cfg}"
    # spelled out: the level-0 widths take the wide tile in every plain epilogue, the other levels and every GEGLU call do not
    assert all(got[(N, f, 0)] == 1 for N in WIDE_N for f in LINEAR_FLAGS) and all(got[(N, f, 0)] == 0 for N in WIDE_N + SQUARE_N for f in GEGLU_FLAGS)
    assert all(got[(N, f, 1)] == 1 for N in WIDE_N for f in T3_FLAGS) and all(got[(N, f, 2)] == 1 for N in WIDE_N for f in C9_FLAGS)
    assert all(got[(N, f, gm)] == 0 for N in SQUARE_N for gm, fl in ((0, LINEAR_FLAGS), (1, T3_FLAGS), (2, C9_FLAGS)) for f in fl)


def test_knob_0_is_always_the_square_tile():
    assert set(_answers("0").values()) == {0}


def test_knob_1_is_the_wide_tile_wherever_its_epilogue_exists():
    for (N, f, gm), cfg in _answers("1").items():
        assert cfg == (0 if f in GEGLU_FLAGS else 1), f"N={N} flags=0x{f:x} gather_mode={gm}: configuration {cfg}"


def test_answers_that_do_not_depend_on_the_knob():
    """Flag words and column counts an entry point refuses have no configuration (0); an unknown gather mode is an error."""
    L = _lib.lib()
    from viewcrafter_amd import ops
    for gm in (0, 1, 2):
        assert L.vcx_gemm_mxfp8_cfg(320, 0, gm) == 0 and L.vcx_gemm_mxfp8_cfg(320, RES, gm) == 0 and L.vcx_gemm_mxfp8_cfg(320, BIAS | G.GEMM_OUT_F32, gm) == 0
        assert L.vcx_gemm_mxfp8_cfg(0, BIAS, gm) == 0 and L.vcx_gemm_mxfp8_cfg(-160, BIAS, gm) == 0 and L.vcx_gemm_mxfp8_cfg(324, BIAS, gm) == 0
    assert L.vcx_gemm_mxfp8_cfg(320, BIAS | ROW, 0) == 0 and L.vcx_gemm_mxfp8_cfg(320, BIAS | ROW, 1) == 0 and L.vcx_gemm_mxfp8_cfg(320, BIAS | CS, 0) == 0
    assert L.vcx_gemm_mxfp8_cfg(320, BIAS, 3) < 0 and b"gather mode" in L.vcx_last_error() and L.vcx_gemm_mxfp8_cfg(320, BIAS, -1) < 0
    assert ops.gemm_mxfp8_cfg(640) == 0 and ops.gemm_mxfp8_cfg(640, BIAS | CS, 2) == 0
    with pytest.raises(_lib.VcxError):
        ops.gemm_mxfp8_cfg(320, BIAS, 7)


# ------------------------------------------------------------------------------------------------------------------ the predicates stay put
# Expected answers worked out from the rules as include/vcx.h states them (LIM = 0xFFFF0000: "below 4 GiB"), not from the library: the wide
# tile reaches 159 weight rows past N, the predicates keep vouching for 127 - a configuration that cannot take that reach is the launchers'
# business (they keep the square tile), never a refusal.
LIM = 0xFFFF0000


def test_linear_predicate_answers_are_unchanged():
    ok = _lib.lib().vcx_gemm_mxfp8_ok
    table = [((256, 320, 320, BIAS), 1), ((1, 160, 32, BIAS | RES), 1), ((130, 200, 64, BIAS), 1), ((256, 324, 320, BIAS), 0), ((256, 320, 48, BIAS), 0),
             ((256, 320, 320, BIAS | CS), 0), ((256, 320, 320, BIAS | ROW), 0), ((0, 320, 320, BIAS), 0), ((460800, 320, 1280, BIAS | RES), 1),
             ((460800, 960, 320, BIAS), 1), ((256, 2560, 320, BIAS | G.GEMM_GEGLU), 1), ((256, 2592, 320, BIAS | G.GEMM_GEGLU), 0),
             # the weight extent is N Kp, with no reach past N: Kp = 2^22 -> N <= 1023
             ((8, 1016, 1 << 22, BIAS), 1), ((8, 960, 1 << 22, BIAS), 1), ((8, 1024, 1 << 22, BIAS), 0),
             # the output: rows rounded up to 128, times N, times 2 bytes
             ((1 << 22, 480, 32, BIAS), 1), ((1 << 22, 512, 32, BIAS), 0)]
    assert 1016 * (1 << 22) < LIM <= 1024 * (1 << 22) and (1 << 22) * 480 * 2 < LIM <= (1 << 22) * 512 * 2
    for args, want in table:
        assert ok(*args) == want, (args, _lib.lib().vcx_last_error())


def test_temporal_convolution_predicate_answers_are_unchanged():
    def ok(B, T, P, cin, N, flags=BIAS, ldc=None, ldr=None, ldcs=None, col=0):
        return _lib.lib().vcx_conv_t3_mxfp8_ok(B, T, P, cin, N, N if ldc is None else ldc, N if ldr is None else ldr, N if ldcs is None else ldcs, col, flags)
    assert ok(2, 3, 5, 32, 160) == 1 and ok(2, 3, 5, 32, 200) == 1 and ok(2, 3, 5, 32, 204) == 0 and ok(2, 3, 5, 48, 160) == 0
    assert ok(1, 4, 32, 320, 320, BIAS | CS) == 1 and ok(2, 3, 5, 32, 320, BIAS | CS) == 0            # 30 rows: no whole moment strip
    assert ok(1, 4, 32, 320, 320, BIAS | CS, ldcs=384, col=32) == 1 and ok(1, 4, 32, 320, 320, BIAS | CS, ldcs=340, col=32) == 0
    assert ok(2, 3, 5, 32, 320, BIAS | RES, ldc=344, ldr=328) == 1 and ok(2, 3, 5, 32, 320, BIAS | RES, ldr=312) == 0 and ok(2, 3, 5, 32, 320, BIAS | ROW) == 0
    assert ok(1, 25, 9216, 320, 320, BIAS | RES | CS) == 1 and ok(2, 25, 9216, 320, 320) == 1           # the level-0 block of 576 x 1024 x 25
    # the weight: (N + 127) 3 Kp below LIM.  Kp = 2^22: N + 127 <= 341, N <= 214 - N = 200 stays accepted although 200 + 159 = 359 > 341
    kp = 1 << 22
    assert (208 + 127) * 3 * kp < LIM <= (216 + 127) * 3 * kp and (200 + 159) * 3 * kp >= LIM
    assert ok(1, 1, 8, kp, 208) == 1 and ok(1, 1, 8, kp, 200) == 1 and ok(1, 1, 8, kp, 160) == 1 and ok(1, 1, 8, kp, 216) == 0


def test_3x3_convolution_predicate_answers_are_unchanged():
    def ok(n, H, W, cin, N, flags=BIAS, ldc=None, ldr=None, ldcs=None, col=0, div=1):
        return _lib.lib().vcx_conv3x3_mxfp8_ok(n, H, W, cin, N, N if ldc is None else ldc, N if ldr is None else ldr, N if ldcs is None else ldcs, col, div, flags)
    assert ok(2, 3, 5, 32, 160) == 1 and ok(2, 3, 5, 320, 200) == 1 and ok(2, 3, 5, 320, 204) == 0 and ok(2, 3, 5, 48, 320) == 0
    assert ok(2, 8, 8, 64, 320, BIAS | CS) == 1 and ok(2, 3, 5, 64, 320, BIAS | CS) == 0
    assert ok(2, 8, 8, 64, 320, BIAS | ROW, div=64) == 1 and ok(2, 8, 8, 64, 320, BIAS | ROW, div=48) == 1 and ok(2, 8, 8, 64, 320, BIAS | ROW, div=0) == 0
    assert ok(2, 8, 8, 64, 480, BIAS | ROW | RES | CS, ldc=504, ldr=488, ldcs=544, col=32, div=64) == 1
    assert ok(25, 72, 128, 320, 320, BIAS | ROW | CS, div=25 * 72 * 128) == 1 and ok(25, 72, 128, 960, 320, BIAS | ROW | RES | CS, div=25 * 72 * 128) == 1
    # the weight: (N + 127) 9 Kp below LIM.  Kp = 2^20: N + 127 <= 455, N <= 328 - N = 320 stays accepted although 320 + 159 = 479 > 455
    kp = 1 << 20
    assert (328 + 127) * 9 * kp < LIM <= (336 + 127) * 9 * kp and (320 + 159) * 9 * kp >= LIM
    assert ok(1, 8, 8, kp, 328) == 1 and ok(1, 8, 8, kp, 320) == 1 and ok(1, 8, 8, kp, 160) == 1 and ok(1, 8, 8, kp, 336) == 0
