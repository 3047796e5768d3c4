"""Host side of the per-unit GEMM routes: ops.units_route / ops.units_one_launch_ok mirror the dispatcher of vcx_gemm_units_f16
(csrc/gemm.hip), and the spatial GroupNorm fold keeps its default decisions (VCX_GN_FOLD_SPATIAL=2 is opt-in).  Arithmetic only: no GPU."""
import pytest

# (units, unit_rows, N, K, lda, ldc) -> route at default knobs
ROUTES = [
    ((3, 3600, 640, 128, None, None), "grouped"),
    ((6, 3600, 1280, 1280, None, None), "grouped"),
    ((2, 57600, 640, 640, None, None), "grouped"),
    ((50, 576, 1280, 128, None, None), "grouped"),
    ((50, 2304, 640, 64, None, None), "grouped"),
    ((7, 200, 128, 64, None, None), "grouped"),
    ((9, 40, 64, 64, None, None), "grouped"),
    ((5, 1000, 328, 64, None, None), "grouped"),
    ((4, 1000, 192, 128, 192, 256), "grouped"),
    ((2, 14400, 1280, 1280, None, None), "grouped"),       # level 2 of the benchmark forward under CFG
    ((8, 1024, 320, 320, None, None), "ws320"),            # N = K = 320 keeps the weight-stationary one-launch form
    ((2, 230400, 320, 320, None, None), "ws320"),          # level 0 of the benchmark forward under CFG
    ((1, 57600, 640, 640, None, None), "single"),          # one unit: vcx_gemm_f16
    ((4, 8192, 640, 320, None, None), "loop"),             # vcx_gemm_f16 takes each such unit weight-stationary
    ((4, 1000, 640, 72, None, None), "loop"),              # K % 64 != 0: no DMA kernel
    ((4, 1000, 324, 64, 64, 328), "loop"),                 # N % 8 != 0
    ((65536, 8, 64, 64, None, None), "loop"),              # more than 65535 units
]


@pytest.mark.parametrize("shape,route", ROUTES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s, _ in ROUTES])
def test_units_route_table(shape, route, monkeypatch):
    from viewcrafter_amd import ops
    monkeypatch.delenv("VCX_GEMM_UNITS_LOOP", raising=False)
    units, unit_rows, N, K, lda, ldc = shape
    M = units * unit_rows
    assert ops.units_route(M, N, K, unit_rows, lda=lda, ldc=ldc) == route
    assert ops.units_one_launch_ok(M, N, K, unit_rows, lda=lda, ldc=ldc) == (route in ("grouped", "ws320"))
    monkeypatch.setenv("VCX_GEMM_UNITS_LOOP", "1")      # forces the loop where the tiled engine's per-unit form would run, nothing else
    assert ops.units_route(M, N, K, unit_rows, lda=lda, ldc=ldc) == ("loop" if route == "grouped" else route)


def test_units_route_at_the_extent_limit(monkeypatch):
    """Output offsets up to 256 rows past the end must stay below 0xFFFF0000 bytes (the rule of vcx_gemm_f16's `dma_ok`): with 64-column
    rows the last M that passes is 33 553 663 (11 units), one row more (2 units) goes to the loop."""
    from viewcrafter_amd import ops
    monkeypatch.delenv("VCX_GEMM_UNITS_LOOP", raising=False)
    lim, N, K = 0xFFFF0000, 64, 64
    m_last = (lim - 1) // (2 * N) - 256
    assert 2 * (m_last + 256) * N < lim <= 2 * (m_last + 1 + 256) * N
    assert m_last % 11 == 0 and (m_last + 1) % 2 == 0
    assert ops.units_route(m_last, N, K, m_last // 11) == "grouped" and ops.units_one_launch_ok(m_last, N, K, m_last // 11)
    assert ops.units_route(m_last + 1, N, K, (m_last + 1) // 2) == "loop" and not ops.units_one_launch_ok(m_last + 1, N, K, (m_last + 1) // 2)
    # the operand's own extent: rows of 8 x 64 columns reach the limit first
    lda = 8 * K
    a_last = (lim - 1 - 2 * K) // (2 * lda) + 1          # largest M with 2 ((M - 1) lda + K) < lim
    assert 2 * ((a_last - 1) * lda + K) < lim <= 2 * (a_last * lda + K)
    for M, want in ((a_last - a_last % 2, "grouped"), (a_last - a_last % 2 + 2, "loop")):
        assert ops.units_route(M, N, K, M // 2, lda=lda) == want, M


# (height, width) of the latent at 576 x 1024 and 320 x 512, 25 frames: per level (pixels, channels)
LEVELS = {"576x1024x25": [(72 * 128, 320), (36 * 64, 640), (18 * 32, 1280), (9 * 16, 1280)],
          "320x512x25": [(40 * 64, 320), (20 * 32, 640), (10 * 16, 1280), (5 * 8, 1280)]}
DEFAULT = {"576x1024x25": [True, False, False, False], "320x512x25": [True, False, False, False]}
# opt-in: wherever a video's tensor reaches GN_FOLD_MIN_BYTES (16 MiB) and the frames go through the tiled engine's per-unit form
OPT_IN = {"576x1024x25": [True, True, True, False], "320x512x25": [True, True, False, False]}


@pytest.mark.parametrize("config", sorted(LEVELS))
def test_spatial_fold_decisions_of_the_shipped_configs(config, monkeypatch):
    from viewcrafter_amd.lvdm.modules import attention as A
    monkeypatch.delenv("VCX_GEMM_UNITS_LOOP", raising=False)
    assert A.GN_FOLD and A.GN_FOLD_SPATIAL == 1 and A.GN_FOLD_MIN_BYTES == 16 << 20      # the defaults (the suite runs without VCX_GN_* set)
    assert [A.spatial_fold_ok(25, px, C, C) for px, C in LEVELS[config]] == DEFAULT[config]
    monkeypatch.setattr(A, "GN_FOLD_SPATIAL", 2)
    assert [A.spatial_fold_ok(25, px, C, C) for px, C in LEVELS[config]] == OPT_IN[config]
    monkeypatch.setattr(A, "GN_FOLD_SPATIAL", 0)
    assert not any(A.spatial_fold_ok(25, px, C, C) for px, C in LEVELS[config])
