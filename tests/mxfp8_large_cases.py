"""The MXFP8 kernel family where byte offsets pass 2 GiB: ONE table of named cases for tests/test_mxfp8_large_cpu.py (which checks the table
against the library's predicates and against the rules below) and tests/test_mxfp8_large_extent_gpu.py (which runs them).  No GPU code.

Regimes, named in the test ids:  `2g` - the named extent lies in [2^31, LIM);  `lim` - the largest shape the predicate accepts (one step
further - M + 1, T + 1 or H + 1 - is refused);  `past_4g` - past 2^32 bytes (the quantisers index with 64 bits and have no limit).

The 32-bit rules, restated from include/vcx.h and the comments of mx_takes / mx_gather_takes (csrc/gemm_mx.hip) - never read from the
library:  LIM = 0xFFFF0000;  mt(M) = M rounded up to 128 (the tile grid reaches 127 rows past M);
  linear:    M Kp < LIM, N Kp < LIM, mt(M) Kp < 2^32;  mt(M) ld 2 < LIM for the fp16 output and residual;  mt(M) Kp(N / 2) < LIM for the
             MXFP8 output of the GEGLU epilogue
  gathered:  (M + 127 + reach) Kp < LIM with reach = P (temporal) or W + 1 (3x3);  (N + 127) taps Kp < LIM;  mt(M) ld 2 < LIM;
             tailed: (M + 127) Kp(Ct) < LIM, (N + 127) (9 Kp + Kp(Ct)) < LIM
  attention: output rows x Kp(64 heads) < 2^32."""
LIM = 0xFFFF0000
G31, G32 = 1 << 31, 1 << 32
SLICE_MAX = G31               # rule (b): every operand and output of a slice call stays below this many bytes


def kp_of(K):
    return (K + 127) // 128 * 128


def mt(M):
    return (M + 127) // 128 * 128


def _case(form, name, regime, named, **kw):
    c = dict(form=form, id=f"{form}_{name}_{regime}", regime=regime, named=named, flags=frozenset(), exact=True, step=None)
    c.update(kw)
    c["flags"] = frozenset(c["flags"])
    return c


def _first_multiple_of_64_past_2g(ldc):
    """the smallest M, a multiple of 64, whose last row starts at or past byte 2^31 of an fp16 buffer of pitch ldc"""
    m = -(-G31 // (2 * ldc)) + 1
    return -(-m // 64) * 64


# ---------------------------------------------------------------------------------------------------------------- vcx_gemm_mxfp8
def _linear():
    out = [
        _case("linear", "activation", "2g", "activation", M=2_200_001, N=8, K=1024),
        _case("linear", "activation", "lim", "activation", M=4_194_176, N=8, K=1024, step=dict(M=4_194_177)),
    ]
    for tile, N, m_lim in (("wide_tile", 320, 6_710_656), ("square_tile", 256, 8_388_352)):
        m2g = _first_multiple_of_64_past_2g(N + 8)
        out.append(_case("linear", f"output_residual_{tile}", "2g", "output", M=m2g, N=N, K=32, flags={"residual"}, ldc=N + 8, ldr=N + 8))
        out.append(_case("linear", f"output_residual_{tile}", "lim", "output", M=m_lim, N=N, K=32, flags={"residual"}, ldc=N, ldr=N, step=dict(M=m_lim + 1)))
    out.append(_case("linear", "output_residual_wide_tile_ragged", "2g", "output", M=_first_multiple_of_64_past_2g(328) + 37, N=320, K=32, flags={"residual"},
                     ldc=328, ldr=328))
    out += [
        _case("linear", "geglu_mx_out", "2g", "mx_output", M=2_200_064, N=2048, K=32, flags={"geglu", "mx_out"}, exact=False),
        _case("linear", "geglu_mx_out", "lim", "mx_output", M=4_194_176, N=2048, K=32, flags={"geglu", "mx_out"}, exact=False, step=dict(M=4_194_177)),
        _case("linear", "geglu_f16_out", "2g", "output", M=1_100_033, N=2048, K=32, flags={"geglu"}, exact=False),
        _case("linear", "geglu_f16_out", "lim", "output", M=2_097_024, N=2048, K=32, flags={"geglu"}, exact=False, step=dict(M=2_097_025)),
    ]
    return out


# ---------------------------------------------------------------------------------------------------------------- the gathered forms
def _gathered():
    return [
        _case("t3", "activation", "2g", "activation", B=2, T=300, P=4096, Cin=1024, N=8),
        _case("t3", "activation", "lim", "activation", B=2, T=511, P=4096, Cin=1024, N=8, step=dict(T=512)),
        _case("t3", "wide_target", "2g", "output", B=4, T=35, P=8192, Cin=32, N=320, flags={"residual", "colstats"}, ldc=960, ldr=960, ldcs=960, cs_col=320),
        _case("c9", "activation", "2g", "activation", n=8, H=140, W=2048, Cin=1024, N=8),
        _case("c9", "activation", "lim", "activation", n=8, H=255, W=2048, Cin=1024, N=8, step=dict(H=256)),
        # the production pattern: a level-0 convolution of a batched clip writing into the 960-column concat target
        _case("c9", "concat_target", "2g", "output", n=80, H=112, W=128, Cin=32, N=320, flags={"rowadd", "residual", "colstats"}, ldc=960, ldr=960, ldcs=960,
              cs_col=320, rowadd_div=112 * 128),
        # the gathered source is the large one (tests/test_mxfp8_resconv_tail_gpu.py has the tail source past 2^31)
        _case("tail", "gathered_source", "2g", "activation", n=8, H=140, W=2048, Cin=1024, Ct=32, N=8),
        _case("tail", "gathered_source", "lim", "activation", n=8, H=255, W=2048, Cin=1024, Ct=32, N=8, step=dict(H=256)),
    ]


GEMM_CASES = _linear() + _gathered()


def geometry(c):
    """-> (M, rows per slice unit, units, taps, reach): a slice of rule (b) is a range of units - rows (linear), whole videos (t3), whole
    frames (c9, tailed)"""
    f = c["form"]
    if f == "linear":
        return c["M"], 1, c["M"], 1, 0
    if f == "t3":
        return c["B"] * c["T"] * c["P"], c["T"] * c["P"], c["B"], 3, c["P"]
    return c["n"] * c["H"] * c["W"], c["H"] * c["W"], c["n"], 9, c["W"] + 1


def n_out(c):
    return c["N"] // 2 if "geglu" in c["flags"] else c["N"]


def pitches(c):
    """(ldc, ldr) in elements as the call passes them (ldr 0 without a residual)"""
    return c.get("ldc") or n_out(c), (c.get("ldr") or n_out(c)) if "residual" in c["flags"] else 0


def k_of(c):
    return c["K"] if c["form"] == "linear" else c["Cin"]


def rule_extents(c):
    """[(name, value, limit)]: the call is taken iff every value is below its limit (module docstring)"""
    M, _, _, taps, reach = geometry(c)
    kp, N = kp_of(k_of(c)), c["N"]
    ldc, ldr = pitches(c)
    if c["form"] == "linear":
        r = [("activation", M * kp, LIM), ("weight", N * kp, LIM), ("activation, tile reach", mt(M) * kp, G32)]
        if "mx_out" in c["flags"]:
            return r + [("MXFP8 output, tile reach", mt(M) * kp_of(n_out(c)), LIM)]
    else:
        r = [("activation, tile and tap reach", (M + 127 + reach) * kp, LIM), ("weight, tile reach", (N + 127) * taps * kp, LIM)]
        if c["form"] == "tail":
            kpt = kp_of(c["Ct"])
            r += [("tail, tile reach", (M + 127) * kpt, LIM), ("tailed weight, tile reach", (N + 127) * (taps * kp + kpt), LIM)]
    r.append(("output, tile reach", mt(M) * ldc * 2, LIM))
    if ldr:
        r.append(("residual, tile reach", mt(M) * ldr * 2, LIM))
    return r


def buffer_bytes(c, M=None):
    """name -> bytes of every operand and output of the call on M rows (default: the case's own), pitches as the case has them"""
    M = geometry(c)[0] if M is None else M
    kp = kp_of(k_of(c))
    ldc, ldr = pitches(c)
    b = {"activation": M * kp, "activation scales": M * kp // 32}
    if c["form"] == "tail":
        b["tail"] = M * kp_of(c["Ct"])
    if "mx_out" in c["flags"]:
        b["mx_output"] = M * kp_of(n_out(c))
    else:
        b["output"] = ((M - 1) * ldc + n_out(c)) * 2
    if ldr:
        b["residual"] = ((M - 1) * ldr + n_out(c)) * 2
    if "colstats" in c["flags"]:
        b["column moments"] = (M // 64) * c["ldcs"] * 8
    return b


def named_extent(c):
    """the extent the case's id speaks of: an operand's bytes, or for an fp16 output the byte offset of its last row"""
    M = geometry(c)[0]
    if c["named"] == "output":
        return (M - 1) * pitches(c)[0] * 2
    return buffer_bytes(c)[c["named"]]


def in_regime(extent, regime):
    return extent >= G32 if regime == "past_4g" else G31 <= extent < LIM


def split(units, parts):
    """[(lo, hi)]: `units` in `parts` nearly equal ranges"""
    return [(units * i // parts, units * (i + 1) // parts) for i in range(parts)]


def slices(c):
    """rule (b): ranges of slice units (geometry) - the fewest nearly equal parts, two or more, whose every buffer stays below SLICE_MAX"""
    _, per, units, _, _ = geometry(c)
    for parts in range(2, units + 1):
        s = split(units, parts)
        if all(max(buffer_bytes(c, (hi - lo) * per).values()) < SLICE_MAX for lo, hi in s):
            return s
    raise AssertionError(f"{c['id']}: no slicing keeps every buffer below 2^31 bytes")


def stepped(c):
    """the `lim` case one step further"""
    d = dict(c)
    d.update(c["step"])
    return d


# ---------------------------------------------------------------------------------------------------------------- quantisers (64-bit indexing)
ROWS_2G, ROWS_4G = (1 << 24) + 4099, (1 << 25) + 4099          # x Kp = 128: q past 2^31 / past 2^32 bytes; odd row counts
GN_PIXELS = 12_000_000                                          # x 128: frame 1 straddles byte 2^31 of q, frame 2 byte 2^32

QUANT_CASES = [
    dict(form="quant", id="quant_2g", regime="2g", rows=ROWS_2G, K=64, ldx=72),
    dict(form="quant", id="quant_past_4g", regime="past_4g", rows=ROWS_4G, K=64, ldx=72),
    dict(form="layernorm", id="layernorm_2g", regime="2g", rows=ROWS_2G, K=64),
    dict(form="layernorm", id="layernorm_past_4g", regime="past_4g", rows=ROWS_4G, K=64),
] + [dict(form="groupnorm", id=f"groupnorm_{'apply2' if split_ else 'apply'}{'_raw' if raw else ''}_past_4g", regime="past_4g", n_outer=3, pixels=GN_PIXELS,
          K=64, c1=32 if split_ else 64, groups=32, raw=raw) for split_ in (False, True) for raw in (False, True)]


def quant_rows_of(c):
    return c["n_outer"] * c["pixels"] if c["form"] == "groupnorm" else c["rows"]


def quant_slices(c):
    """rule (b): row ranges (quant, layernorm) or whole statistics units (groupnorm) whose q stays below SLICE_MAX"""
    if c["form"] == "groupnorm":
        return [(i, i + 1) for i in range(c["n_outer"])]
    rows, kp = c["rows"], kp_of(c["K"])
    return split(rows, -(-rows * kp // (SLICE_MAX - (1 << 20))))


# ---------------------------------------------------------------------------------------------------------------- quantising attention
TATTN_P = (1 << 23) + 4096
FLASH_G, FLASH_NQ = 4100, 4096                                  # 4100 x 4096 rows x Kp = 128: 2 149 580 800 bytes

ATTN_CASES = [dict(form="tattn", id=f"tattn_heads{h}_{'causal' if causal else 'plain'}_2g", regime="2g", B=1, T=2, P=TATTN_P, heads=h, causal=causal)
              for h in (1, 2) for causal in (False, True)] + [
    # one case per kernel behind vcx_attn_flash_d64_mxfp8; the knobs are those of SINGLE in tests/test_mxfp8_sattn_gpu.py (nq / 256 is whole:
    # the natural dispatch takes two query blocks per wave; the long-sequence kernel is forced at the key count SINGLE forces it at)
    dict(form="flash", id="flash_qb2_2g", regime="2g", n_groups=FLASH_G, heads=1, nq=FLASH_NQ, nk=64, knobs={}),
    dict(form="flash", id="flash_qb1_2g", regime="2g", n_groups=FLASH_G, heads=1, nq=FLASH_NQ, nk=64, knobs={"FLASH_QB": 1}),
    dict(form="flash", id="flash_flash2_2g", regime="2g", n_groups=FLASH_G, heads=1, nq=FLASH_NQ, nk=192, knobs={"FLASH_IMPL": 2}),
    # text (+) image keys shared by the 25 frames of a video: the LDS-resident second-form kernel, the one production runs
    dict(form="dual", id="flash_dual_resident2_2g", regime="2g", n_groups=FLASH_G, heads=1, nq=FLASH_NQ, nk1=77, kv_rows1=80, nk2=64, kv_div=25),
]


def attn_rows(c):
    return c["B"] * c["T"] * c["P"] if c["form"] == "tattn" else c["n_groups"] * c["nq"]


def attn_buffer_bytes(c, units=None):
    """name -> bytes of the large buffers of a call on `units` pixels (temporal; q | k | v in one dense buffer of 3 x 64 heads columns) or
    frame groups (flash, dual; dense q of 64 heads columns) - default: the case's own"""
    kp = kp_of(64 * c["heads"])
    if c["form"] == "tattn":
        rows = c["B"] * c["T"] * (c["P"] if units is None else units)
        return {"qkv": rows * 3 * 64 * c["heads"] * 2, "output": rows * kp}
    rows = (c["n_groups"] if units is None else units) * c["nq"]
    return {"q": rows * 64 * c["heads"] * 2, "output": rows * kp}


def attn_geo(c, groups=None):
    """the keywords of the flash / dual entry for the case on `groups` frame groups (default: all)"""
    G, D = c["n_groups"] if groups is None else groups, 64 * c["heads"]
    if c["form"] == "flash":
        return dict(n_groups=G, heads=c["heads"], nq=c["nq"], nk=c["nk"], kv_rows=c["nk"], kv_div=1, ldq=D, ldk=D, ldvt=G * c["nk"])
    v = G // c["kv_div"]
    return dict(n_groups=G, heads=c["heads"], nq=c["nq"], nk1=c["nk1"], kv_rows1=c["kv_rows1"], kv_div1=c["kv_div"], ldk1=D, ldvt1=v * c["kv_rows1"],
                nk2=c["nk2"], kv_rows2=c["nk2"], kv_div2=c["kv_div"], ldk2=D, ldvt2=v * c["nk2"], ldq=D)


def attn_slices(c):
    """rule (b): ranges of pixels (temporal: a pixel's T rows are one group) or of frame groups (flash; dual: whole videos) - the fewest nearly
    equal parts, two or more, whose every buffer stays below SLICE_MAX"""
    per = c.get("kv_div", 1)
    units = c["P"] if c["form"] == "tattn" else c["n_groups"] // per
    for parts in range(2, 65):
        s = [(lo * per, hi * per) for lo, hi in split(units, parts)]
        if all(max(attn_buffer_bytes(c, hi - lo).values()) < SLICE_MAX for lo, hi in s):
            return s
    raise AssertionError(f"{c['id']}: no slicing keeps every buffer below 2^31 bytes")


# ---------------------------------------------------------------------------------------------------------------- operands shared by both test files
SEED_A, SEED_T, SEED_W, SEED_B, SEED_R, SEED_RA = 101, 102, 103, 104, 105, 106      # activation, tail, weight, bias, residual, row addend
ADDEND_MAX = 64.0             # |bias|, |residual|, |row addend| of an exact problem: multiples of GRID up to 256 GRID


def weights(c):
    """The small operands of a GEMM case, built on the CPU from fixed seeds (tests/mx_emulation.exact_operand): -> (w pair as the kernel reads
    it, fp64 values [N, taps, K] - with a tail ([N, 9, Cin], [N, Ct]) -, bias fp32 [N]).  Exact cases: the integer grid.  GEGLU cases (slice
    equality only): the same draws six binades down, so that gates of a few units exercise the GELU and the outputs many scale bytes."""
    import torch

    from tests import cpu_kernels_mx_tail as CT
    from tests import mx_emulation as MX
    N, K, form = c["N"], k_of(c), c["form"]
    taps = geometry(c)[3]
    off = 0 if c["exact"] else -6
    q, s, v = MX.exact_operand(taps * N, K, SEED_W, e_offset=off)
    bias = torch.randint(-256, 257, (N,), generator=torch.Generator().manual_seed(SEED_B)).float() * MX.GRID * 2.0 ** off
    vals = v.view(N, taps, K)
    if form in ("linear", "t3"):
        pair = (q.view(N, -1).contiguous(), s.view(N, -1).contiguous())
    else:
        pair = CT.slab_major(q, s, N)
        if form == "tail":
            tq, ts, tv = MX.exact_operand(N, c["Ct"], SEED_W + 1, e_offset=-1)
            pair, vals = CT.join_weight(pair, (tq, ts)), (vals, tv)
    return pair, vals, bias


def exact_sum_bound(c):
    """the largest magnitude a partial sum of an exact case can reach, in any order: every product, then every addend"""
    from tests import mx_emulation as MX
    taps = geometry(c)[3]
    addends = 1 + ("residual" in c["flags"]) + ("rowadd" in c["flags"])
    return (taps * k_of(c) + c.get("Ct", 0)) * MX.PRODUCT_MAX + addends * ADDEND_MAX


ALL_CASES = GEMM_CASES + QUANT_CASES + ATTN_CASES
