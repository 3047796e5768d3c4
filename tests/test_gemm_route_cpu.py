"""vcx_gemm_route (include/vcx.h, ABI 10): the route function the GEMM launchers switch on, asked directly.  Null pointers, no GPU - the
launchers run the same validate + gemm_route (csrc/gemm.hip), so for the refused calls the launcher is asked too (fake pointers: the
refusal comes before any launch) and must give the same text."""
import ctypes

import pytest

from viewcrafter_amd import _lib as G

FAKE = 1 << 20            # 16-byte aligned, never dereferenced
CONV8 = dict(mode=1, in_h=8, in_w=8, out_h=8, out_w=8, cin=8, kh=3, kw=3, stride=1, pad_h=1, pad_w=1)


def _desc(**kw):
    d = G.GemmDesc(alpha=1.0)
    for k, v in kw.items():
        setattr(d, k, v)
    d.ldw = d.ldw or d.K
    d.lda = d.lda or (d.cin if d.mode else d.K)
    d.ldc = d.ldc or (d.N // 2 if d.flags & G.GEMM_GEGLU else d.N)
    return d


def _route(unit_rows=0, **kw):
    L = G.lib()
    return L.vcx_gemm_route(ctypes.byref(_desc(**kw)), unit_rows), L.vcx_last_error()


# (descriptor fields, unit_rows) -> route at default knobs
TABLE = [
    ("geglu_level0", dict(M=460800, N=2560, K=320, flags=G.GEMM_GEGLU | G.GEMM_BIAS_N), 0, G.ROUTE_WS320_GEGLU),
    ("lnfold_960", dict(M=460800, N=960, K=320, flags=G.GEMM_LNFOLD | G.GEMM_BIAS_N), 0, G.ROUTE_WS320_LNF),
    ("lnfold_640", dict(M=460800, N=640, K=320, flags=G.GEMM_LNFOLD | G.GEMM_BIAS_N), 0, G.ROUTE_TILED),       # a half-empty third column block
    ("ws320_from_8192", dict(M=8192, N=320, K=320, flags=G.GEMM_BIAS_N), 0, G.ROUTE_WS320),
    ("tiled_below", dict(M=8191, N=320, K=320, flags=G.GEMM_BIAS_N), 0, G.ROUTE_TILED),
    ("rowstats", dict(M=8192, N=320, K=320, ldr=320, flags=G.GEMM_ROWSTATS | G.GEMM_BIAS_N | G.GEMM_RESIDUAL), 0, G.ROUTE_WS320),
    ("register_k72", dict(M=1000, N=64, K=72), 0, G.ROUTE_REGISTER),
    ("conv3x3", dict(M=128, N=64, K=9 * 64, flags=G.GEMM_CONV_SLABK | G.GEMM_COLSTATS, **dict(CONV8, cin=64)), 0, G.ROUTE_TILED),
    ("units_ws320", dict(M=8 * 1024, N=320, K=320, flags=G.GEMM_BIAS_N | G.GEMM_ROWSTATS), 1024, G.ROUTE_UNITS_WS320),
    ("units_grouped", dict(M=3 * 3600, N=640, K=128, flags=G.GEMM_BIAS_N), 3600, G.ROUTE_UNITS_GROUPED),
    ("units_loop", dict(M=4 * 8192, N=640, K=320, flags=G.GEMM_BIAS_N), 8192, G.ROUTE_UNITS_LOOP),      # vcx_gemm_f16 takes each unit weight-stationary
    ("units_single", dict(M=57600, N=640, K=640, flags=G.GEMM_BIAS_N), 57600, G.ROUTE_TILED),           # one unit is vcx_gemm_f16's call
    ("units_single_ws", dict(M=9216, N=320, K=320, flags=G.GEMM_BIAS_N | G.GEMM_ROWSTATS), 9216, G.ROUTE_WS320),
]
# -> refused, with the word the reason carries
REFUSED = [
    ("rowstats_n640", dict(M=9000, N=640, K=320, flags=G.GEMM_ROWSTATS), 0, b"ROWSTATS needs the weight-stationary kernel"),
    ("colstats_k72", dict(M=128, N=64, K=72, flags=G.GEMM_COLSTATS), 0, b"COLSTATS needs the DMA kernel"),
    ("lnfold_k72", dict(M=128, N=64, K=72, flags=G.GEMM_LNFOLD), 0, b"LNFOLD needs the DMA kernel"),
    ("tail_cin8", dict(M=64, N=64, K=72 + 64, tail_k0=64, tail_lda0=64, **CONV8), 0, b"a K tail needs the DMA kernel"),
    ("units_rowstats", dict(M=4 * 1000, N=320, K=320, flags=G.GEMM_BIAS_N | G.GEMM_ROWSTATS), 1000, b"ROWSTATS needs the one-launch weight-stationary form"),
]


@pytest.mark.parametrize("name,fields,unit_rows,want", TABLE, ids=[t[0] for t in TABLE])
def test_route_table(name, fields, unit_rows, want, monkeypatch):
    monkeypatch.delenv("VCX_GEMM_UNITS_LOOP", raising=False)
    assert _route(unit_rows, **fields)[0] == want


@pytest.mark.parametrize("name,fields,unit_rows,word", REFUSED, ids=[t[0] for t in REFUSED])
def test_refused_with_the_launchers_reason(name, fields, unit_rows, word, monkeypatch):
    monkeypatch.delenv("VCX_GEMM_UNITS_LOOP", raising=False)
    rc, msg = _route(unit_rows, **fields)
    assert rc == G.ROUTE_REFUSED and word in msg, (rc, msg)
    # the launcher: the same refusal, the same text
    L = G.lib()
    d = _desc(A=FAKE, W=FAKE, C=FAKE, bias=FAKE, rowstats=FAKE, colstats=FAKE, ln_stats=FAKE, ln_colsum=FAKE, tail_a0=FAKE, **fields)
    rc = L.vcx_gemm_units_f16(ctypes.byref(d), unit_rows, d.N * d.K, d.N, None) if unit_rows else L.vcx_gemm_f16(ctypes.byref(d), None)
    assert rc == -1 and L.vcx_last_error() == msg


def test_invalid_descriptors_are_not_routes():
    """What the launcher's validation rejects is VCX_EINVAL here too (not a route, not REFUSED); only the pointer checks are skipped."""
    L = G.lib()
    assert _route(M=128, N=64, K=70)[0] == -1 and b"multiples of 8" in L.vcx_last_error()
    assert _route(M=100, N=64, K=64, flags=G.GEMM_COLSTATS)[0] == -1 and b"M % 64" in L.vcx_last_error()
    assert _route(1000, M=4096, N=64, K=64)[0] == -1 and b"whole number of units" in L.vcx_last_error()
    assert _route(-1, M=4096, N=64, K=64)[0] == -1
    assert L.vcx_gemm_route(None, 0) == -1
    d = _desc(M=128, N=64, K=64)
    assert L.vcx_gemm_route(ctypes.byref(d), 0) == G.ROUTE_TILED                                   # null A / W / C: fine here ...
    assert L.vcx_gemm_f16(ctypes.byref(d), None) == -1 and b"null A/W/C" in L.vcx_last_error()     # ... and refused by the launcher


def test_route_is_a_function_of_descriptor_and_knobs_only(monkeypatch):
    """Set a knob, ask, restore: the answer follows the knob and comes back - gemm_route keeps no state and reads the knobs per call."""
    from viewcrafter_amd import ops
    monkeypatch.delenv("VCX_GEMM_UNITS_LOOP", raising=False)
    ws = dict(M=8192, N=320, K=320, flags=G.GEMM_BIAS_N)
    geglu = dict(M=460800, N=2560, K=320, flags=G.GEMM_GEGLU | G.GEMM_BIAS_N)
    lnf640 = dict(M=460800, N=640, K=320, flags=G.GEMM_LNFOLD | G.GEMM_BIAS_N)
    grouped = dict(M=3 * 3600, N=640, K=128, flags=G.GEMM_BIAS_N)
    cases = [("GEMM_WS", 0, ws, 0, G.ROUTE_TILED, G.ROUTE_WS320), ("GEMM_DMA", 0, ws, 0, G.ROUTE_REGISTER, G.ROUTE_WS320),
             ("GEMM_CFG", 2, ws, 0, G.ROUTE_TILED, G.ROUTE_WS320), ("GEMM_CFG", 7, ws, 0, G.ROUTE_REFUSED, G.ROUTE_WS320),
             ("GEMM_WS", 2, geglu, 0, G.ROUTE_TILED, G.ROUTE_WS320_GEGLU), ("GEMM_WS", 3, geglu, 0, G.ROUTE_WS320_GEGLU, G.ROUTE_WS320_GEGLU),
             ("GEMM_WS", 5, lnf640, 0, G.ROUTE_WS320_LNF, G.ROUTE_TILED), ("GEMM_WS", 4, dict(lnf640, N=960), 0, G.ROUTE_TILED, G.ROUTE_WS320_LNF),
             ("GEMM_CFG", 6, grouped, 3600, G.ROUTE_UNITS_LOOP, G.ROUTE_UNITS_GROUPED), ("GEMM_CFG", 4, grouped, 3600, G.ROUTE_UNITS_GROUPED, G.ROUTE_UNITS_GROUPED),
             ("GEMM_DMA", 0, grouped, 3600, G.ROUTE_UNITS_LOOP, G.ROUTE_UNITS_GROUPED),
             ("GEMM_WS", 0, dict(M=4 * 8192, N=640, K=320, flags=G.GEMM_BIAS_N), 8192, G.ROUTE_UNITS_GROUPED, G.ROUTE_UNITS_LOOP)]
    for knob, value, fields, unit_rows, with_knob, default in cases:
        assert _route(unit_rows, **fields)[0] == default, (knob, value)
        before = ops.tune_set(knob, value)
        try:
            assert _route(unit_rows, **fields)[0] == with_knob, (knob, value)
        finally:
            ops.tune_set(knob, before)
        assert _route(unit_rows, **fields)[0] == default, (knob, value)
    monkeypatch.setenv("VCX_GEMM_UNITS_LOOP", "1")
    assert _route(3600, **grouped)[0] == G.ROUTE_UNITS_LOOP and _route(1024, M=8192, N=320, K=320)[0] == G.ROUTE_UNITS_WS320
    monkeypatch.setenv("VCX_GEMM_UNITS_LOOP", "0")
    assert _route(3600, **grouped)[0] == G.ROUTE_UNITS_GROUPED


def test_python_names_of_the_routes_follow_the_header():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vcx.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"VCX_ROUTE_([A-Z0-9_]+) = (\d+)", src)}
    assert len(header) == 9 and header == {k[len("ROUTE_"):]: v for k, v in vars(G).items() if k.startswith("ROUTE_")}
