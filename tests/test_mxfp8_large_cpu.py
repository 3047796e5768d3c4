"""What tests/test_mxfp8_large_extent_gpu.py stands on, checked without a GPU: the device reference (tests/mx_device_ref.py) equals the
format's definition (tests/mx_emulation.py) byte for byte, the integer-grid operands meet the conditions under which every partial sum is
exact, every case of tests/mxfp8_large_cases.py is accepted by the library's predicate, lies in the regime its id claims and - `lim` -
is refused one step further, every slice of rule (b) stays below 2^31 bytes, and a batched clip never leaves the MX route its solo run takes."""
import types

import pytest
import torch

from tests import mx_device_ref as D
from tests import mx_emulation as MX
from tests import mxfp8_large_cases as C

G31, G32, LIM = C.G31, C.G32, C.LIM
EXACT = [c for c in C.GEMM_CASES if c["exact"]]
ids = lambda cases: [c["id"] for c in cases]


# ------------------------------------------------------------------------------------------------------------------ 1. reference = definition
@pytest.mark.parametrize("K", [32, 64, 320, 1280])
def test_device_reference_equals_the_definition(K):
    """Random rows whose blocks are 2^-20 .. 2^13 loud with the format's edges planted, through quant_rows in chunks that do not divide the
    row count, and back through dequant_rows."""
    rows = 1003
    g = torch.Generator().manual_seed(K)
    x = (torch.randn((rows, K), generator=g) * torch.exp2(torch.randint(-20, 14, (rows, K // 32), generator=g).float()).repeat_interleave(32, 1)).half()
    where = MX.plant_boundaries(x)
    assert len(where) == len(MX.boundary_blocks()) and rows % 77 != 0
    q, s = MX.quant(x)
    for name, (r, b) in where.items():          # (the definition itself, on the planted blocks: the scale bytes the table states)
        assert int(s[r, b]) == MX.boundary_blocks()[name][1], name
    q2, s2 = D.quant_rows(x, chunk=77)
    assert torch.equal(q2, q), f"elements differ in {int((q2 != q).sum())} bytes"
    assert torch.equal(s2, s), f"scales differ in {int((s2 != s).sum())} bytes"
    for dtype in (torch.float64, torch.float32):
        a, b = MX.dequant(q, s, K, dtype), torch.cat([D.dequant_rows(q[r0:r0 + 77], s[r0:r0 + 77], K, dtype) for r0 in range(0, rows, 77)])
        assert a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_device_reference_rounds_every_fp16_value_as_the_definition_does():
    """all 65536 fp16 bit patterns, once grouped by magnitude (block maxima near their elements) and once shuffled (small elements under large maxima)"""
    allh = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    for x in (allh.view(-1, 32), allh[torch.randperm(65536, generator=torch.Generator().manual_seed(1))].view(-1, 32)):
        q, s = MX.quant(x)
        q2, s2 = D.quant_rows(x, chunk=999)
        assert torch.equal(q2, q) and torch.equal(s2, s)


# ------------------------------------------------------------------------------------------------------------------ 2. exact-data conditions
@pytest.mark.parametrize("K,e_offset", [(32, 0), (96, 1), (1024, 0)])
def test_exact_operand_dev_meets_the_stated_conditions(K, e_offset):
    """mx_emulation's conditions: integer elements in [-7, 7] as exact e4m3 bytes, scale exponents in {-1, 0, 1} (+ e_offset) per (row, block),
    padding 0 / 127 - and every element value, every exponent in use, rows and blocks different from each other; several draws per tensor."""
    rows, kp = 300, MX.kp_of(K)
    q, s = D.exact_operand_dev(rows, K, 5, "cpu", draw=64 * K + 1, e_offset=e_offset)          # 64 rows per draw, a ragged last one
    assert q.shape == (rows, kp) and s.shape == (rows, kp // 32) and q.dtype == s.dtype == torch.uint8
    assert bool((q[:, K:] == 0).all()) and bool((s[:, K // 32:] == 127).all())
    v = q[:, :K].contiguous().view(torch.float8_e4m3fn).float()
    assert torch.equal(v, v.round()) and float(v.abs().max()) == MX.ELEM_MAX and set(v.flatten().tolist()) == set(range(-MX.ELEM_MAX, MX.ELEM_MAX + 1))
    assert set(s[:, :K // 32].flatten().tolist()) == {127 + e + e_offset for e in MX.EXPONENTS}
    val = D.dequant_rows(q, s, K)
    assert torch.equal(val, v.double().view(rows, -1, 32).mul(torch.exp2(s[:, :K // 32].double() - 127)[..., None]).view(rows, K))
    assert torch.unique(q[:, :K], dim=0).shape[0] == rows, "rows repeat"
    assert torch.unique(q[:, :K].reshape(-1, 32), dim=0).shape[0] == rows * K // 32, "blocks repeat"
    q2, _ = D.exact_operand_dev(rows, K, 6, "cpu", draw=64 * K + 1, e_offset=e_offset)
    assert not torch.equal(q, q2), "the seed does not move the draws"
    assert MX.PRODUCT_MAX == MX.ELEM_MAX ** 2 * 4 and MX.GRID == 0.25


def _long_exact_operands():
    """(K, bytes) of every exact_operand_dev tensor of the table that reaches 2^31 bytes: activations, and tail sources"""
    out = set()
    for c in C.GEMM_CASES:
        b = C.buffer_bytes(c)
        for name, K in (("activation", C.k_of(c)), ("tail", c.get("Ct"))):
            if name in b and b[name] > G31 + 4096:
                out.add((K, b[name] > G32 + 4096))
    return sorted(out)


def test_exact_operand_dev_is_different_everywhere():
    """A read from `offset mod 2^31` (or `mod 2^32`) must fetch other bytes: for every operand width whose tensor is long enough, the 4096
    bytes at offsets 0, 2^31 and - where the tensor is that long - 2^32 differ from each other.  (Drawn here on the CPU up to the offset in
    question: the function has one body for every device.)"""
    long_ones = _long_exact_operands()
    assert long_ones, "the table has operands past 2^31 bytes"
    for K, past_4g in long_ones:
        kp = MX.kp_of(K)
        offsets = [0, G31] + ([G32] if past_4g else [])
        q, _ = D.exact_operand_dev(offsets[-1] // kp + 4096 // kp + 1, K, C.SEED_A, "cpu")
        flat = q.view(-1)
        blocks = [flat[o:o + 4096] for o in offsets]
        for i in range(len(blocks)):
            for j in range(i):
                assert not torch.equal(blocks[i], blocks[j]), f"K = {K}: the bytes at offsets {offsets[j]} and {offsets[i]} are equal"
        for o in offsets[1:]:          # nor is any 128-byte row around the offset a copy of the row `offset` bytes before it
            r = o // kp
            assert not bool((q[r:r + 4096 // kp] == q[:4096 // kp]).all(dim=1).any())


@pytest.mark.parametrize("c", EXACT, ids=ids(EXACT))
def test_exact_cases_keep_every_partial_sum_exact(c):
    """From the case's own numbers: taps x Cin (+ Ct) products of at most PRODUCT_MAX plus the addends stay below 2^24 GRID, so every fp32
    partial sum, in any order, is exact.  |ref| < 65504 (no fp16 overflow in the output) cannot follow from that worst case; it is
    asserted on every row by the GPU test, and here on a sample: 512 output rows from 512 x taps activation rows drawn as the GPU test draws them."""
    assert C.exact_sum_bound(c) < (1 << 24) * MX.GRID, (c["id"], C.exact_sum_bound(c))
    taps, K, N = C.geometry(c)[3], C.k_of(c), c["N"]
    _, vals, bias = C.weights(c)
    w, wt = vals if c["form"] == "tail" else (vals, None)
    assert w.shape == (N, taps, K) and torch.equal(w / MX.GRID * 2, (w / MX.GRID * 2).round())
    a = D.dequant_rows(*D.exact_operand_dev(512 * taps, K, C.SEED_A, "cpu"), K).view(taps, 512, K)
    ref = bias.double() + sum(a[t] @ w[:, t].t() for t in range(taps))
    if wt is not None:
        ref = ref + D.dequant_rows(*D.exact_operand_dev(512, c["Ct"], C.SEED_T, "cpu", e_offset=1), c["Ct"]) @ wt.t()
    assert torch.equal(ref / MX.GRID, (ref / MX.GRID).round())
    assert float(ref.abs().max()) + 2 * C.ADDEND_MAX < 65504 / 2, "the sample leaves no room below the fp16 maximum"


# ------------------------------------------------------------------------------------------------------------------ 3. the case table
def _flags(c):
    from viewcrafter_amd import ops as G
    names = dict(residual=G.GEMM_RESIDUAL, geglu=G.GEMM_GEGLU, mx_out=G.GEMM_MXFP8_OUT, rowadd=G.GEMM_ROWADD, colstats=G.GEMM_COLSTATS)
    f = G.GEMM_BIAS_N
    for n in c["flags"]:
        f |= names[n]
    return f


def _library_takes(c):
    """the library's own _ok predicate on the case's shape, flags and pitches"""
    from viewcrafter_amd import _lib
    L = _lib.lib()
    ldc, ldr = C.pitches(c)
    cs = "colstats" in c["flags"]
    ldcs, col = (c["ldcs"], c["cs_col"]) if cs else (0, 0)
    if c["form"] == "linear":
        return L.vcx_gemm_mxfp8_ok(c["M"], c["N"], c["K"], _flags(c)) == 1
    if c["form"] == "t3":
        return L.vcx_conv_t3_mxfp8_ok(c["B"], c["T"], c["P"], c["Cin"], c["N"], ldc, ldr, ldcs, col, _flags(c)) == 1
    if c["form"] == "c9":
        return L.vcx_conv3x3_mxfp8_ok(c["n"], c["H"], c["W"], c["Cin"], c["N"], ldc, ldr, ldcs, col, c.get("rowadd_div", 0), _flags(c)) == 1
    return L.vcx_conv3x3_tail_mxfp8_ok(c["n"], c["H"], c["W"], c["Cin"], c["Ct"], c["N"], ldc, ldcs, col, _flags(c)) == 1


def _last_error():
    from viewcrafter_amd import _lib
    return _lib.lib().vcx_last_error()


def _reach_probe(c):
    """The step of a gathered `lim` case (a whole frame per video / an image row per frame) is coarser than the reach, so it would be refused
    with or without the reach term.  The same operands as one video of one frame (temporal: reach P = all of M) / one frame of two image rows
    (3x3: reach W + 1 = half of M): the library takes the widest shape the rules allow and refuses one pixel more - a predicate without the
    reach term would take half as much again."""
    key, fixed = ("P", dict(B=1, T=1)) if c["form"] == "t3" else ("W", dict(n=1, H=2))
    fits = lambda v: all(val < lim for _, val, lim in C.rule_extents(dict(c, **fixed, **{key: v})))
    lo, hi = 1, 1 << 24
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    assert _library_takes(dict(c, **fixed, **{key: lo})), _last_error()
    assert not _library_takes(dict(c, **fixed, **{key: hi})) and b"4 GiB" in _last_error(), (key, hi, _last_error())


@pytest.mark.parametrize("c", C.GEMM_CASES, ids=ids(C.GEMM_CASES))
def test_gemm_case_is_taken_and_lies_in_its_regime(c):
    assert _library_takes(c), _last_error()
    rules = C.rule_extents(c)
    assert all(v < lim for _, v, lim in rules), [r for r in rules if r[1] >= r[2]]
    ext = C.named_extent(c)
    assert C.in_regime(ext, c["regime"]), f"{c['id']}: {c['named']} extent {ext} is not in the regime"
    if c["regime"] == "lim":
        d = C.stepped(c)
        over = [r for r in C.rule_extents(d) if r[1] >= r[2]]
        assert over, f"{c['id']}: the rules still hold at {c['step']}: not the largest shape"
        assert not _library_takes(d) and b"4 GiB" in _last_error(), (c["step"], _last_error())
        if c["form"] != "linear":
            _reach_probe(c)
    else:
        assert c["step"] is None
    if c["form"] == "linear" and c["named"] == "output" and c["regime"] == "2g" and "geglu" not in c["flags"]:
        M, ldc = c["M"], c["ldc"]
        assert ldc == c["N"] + 8 and (M - 1) * ldc * 2 >= G31
        if M % 64 == 0:
            assert (M - 64 - 1) * ldc * 2 < G31, "the smallest multiple of 64 whose last row starts past 2^31"


def test_the_table_has_the_cases_it_should():
    by = {c["id"]: c for c in C.ALL_CASES}
    assert len(by) == len(C.ALL_CASES), "ids repeat"
    assert any(c["form"] == "linear" and c["named"] == "output" and c["M"] % 128 for c in C.GEMM_CASES), "a ragged M among the output cases"
    assert by["linear_activation_2g"]["M"] % 128, "ragged last tile"
    for form in ("t3", "c9", "tail"):
        assert {c["regime"] for c in C.GEMM_CASES if c["form"] == form and c["named"] == "activation"} == {"2g", "lim"}
    c = by["c9_concat_target_2g"]
    assert c["rowadd_div"] == c["H"] * c["W"] and c["ldc"] == c["ldr"] == c["ldcs"] == 960


@pytest.mark.parametrize("c", C.GEMM_CASES, ids=ids(C.GEMM_CASES))
def test_gemm_slices_stay_below_2_gib(c):
    M, per, units, _, _ = C.geometry(c)
    s = C.slices(c)
    assert len(s) >= 2 and s[0][0] == 0 and s[-1][1] == units and all(a[1] == b[0] for a, b in zip(s, s[1:])) and all(lo < hi for lo, hi in s)
    for lo, hi in s:
        for name, b in C.buffer_bytes(c, (hi - lo) * per).items():
            assert b < G31, (c["id"], lo, hi, name, b)
        if "colstats" in c["flags"]:
            assert (lo * per) % 64 == 0 and (hi * per) % 64 == 0, "whole 64-row strips"
    assert max(C.buffer_bytes(c).values()) >= G31 or C.named_extent(c) >= G31


@pytest.mark.parametrize("c", C.QUANT_CASES, ids=ids(C.QUANT_CASES))
def test_quantiser_case_lies_in_its_regime(c):
    kp = C.kp_of(c["K"])
    rows = C.quant_rows_of(c)
    assert kp == 128 and c["K"] == 64, "half of every row is padding"
    if c["form"] == "groupnorm":
        p = c["pixels"]
        assert c["n_outer"] == 3 and p * kp < G31 < 2 * p * kp < G32 < 3 * p * kp, "frame 1 straddles 2^31 bytes of q, frame 2 straddles 2^32"
    else:
        assert rows % 2 == 1 and (G31 < rows * kp < LIM if c["regime"] == "2g" else rows * kp > G32)
    s = C.quant_slices(c)
    assert s[0][0] == 0 and s[-1][1] == (c["n_outer"] if c["form"] == "groupnorm" else rows) and all(a[1] == b[0] for a, b in zip(s, s[1:]))
    per = c["pixels"] if c["form"] == "groupnorm" else 1
    assert all((hi - lo) * per * max(kp, 2 * c.get("ldx", c["K"])) < G31 for lo, hi in s)


def _attn_takes(c, units=None):
    from viewcrafter_amd import ops
    D_ = 64 * c["heads"]
    if c["form"] == "tattn":
        return ops.temporal_attn_mxfp8_ok(c["B"], c["T"], c["P"] if units is None else units, c["heads"], 3 * D_, causal=c["causal"])
    return (ops.flash_attn_mxfp8_ok if c["form"] == "flash" else ops.flash_attn_dual_mxfp8_ok)(**C.attn_geo(c, units))


@pytest.mark.parametrize("c", C.ATTN_CASES, ids=ids(C.ATTN_CASES))
def test_attention_case_is_taken_and_lies_in_its_regime(c):
    assert _attn_takes(c), _last_error()
    out = C.attn_buffer_bytes(c)["output"]
    assert out == C.attn_rows(c) * C.kp_of(64 * c["heads"]) and G31 <= out < G32
    if c["form"] != "tattn":
        assert out == 2_149_580_800
    if c["form"] == "dual":
        assert c["n_groups"] % c["kv_div"] == 0
    s = C.attn_slices(c)
    assert len(s) >= 2 and s[0][0] == 0 and s[-1][1] == (c["P"] if c["form"] == "tattn" else c["n_groups"]) and all(a[1] == b[0] for a, b in zip(s, s[1:]))
    for lo, hi in s:
        assert all(b < G31 for b in C.attn_buffer_bytes(c, hi - lo).values()) and _attn_takes(c, hi - lo)


# ------------------------------------------------------------------------------------------------------------------ 4. the clip-batch cap
def test_a_batched_clip_never_leaves_the_mx_route_of_its_solo_run():
    """channel_mult (1, 2, 4, 4), model_channels 320 at 576 x 1024 x 25 (latents 72 x 128): every MX predicate the model consults - the
    feed-forward's two layers, q | k | v, V^T and to_out of the spatial and temporal transformers, the quantising attention kernels, the
    temporal convolutions, the 3x3 convolutions plain, into a concat pitch and tailed - accepts n = 1 .. max_videos_per_forward videos
    whenever it accepts one: the cap of clip_batch.py holds for the MX switches too."""
    from viewcrafter_amd import clip_batch, ops
    mc, mult, T, h0, w0 = 320, (1, 2, 4, 4), 25, 72, 128
    unet = types.SimpleNamespace(model_channels=mc, channel_mult=mult, attention_resolutions=(4, 2, 1))
    cap = clip_batch.max_videos_per_forward(unet, T, h0, w0)
    assert cap == 7
    asked = 0

    def predicates(ds, ch, n):
        """name -> answer, for n videos at the level of downsampling ds and width ch"""
        H, W = (h0 + ds - 1) // ds, (w0 + ds - 1) // ds
        P, frames = H * W, n * T
        rows, heads = frames * P, ch // 64
        p = {}
        if ds in unet.attention_resolutions:
            p["ff.0"] = ops.linear_mxfp8_ok(rows, 8 * ch, ch, geglu=True, mx_out=True)
            p["ff.2"] = ops.linear_mxfp8_ok(rows, ch, 4 * ch, residual=True)
            p["q|k"] = ops.linear_mxfp8_ok(rows, 2 * ch, ch)
            p["q"] = ops.linear_mxfp8_ok(rows, ch, ch)
            p["q|k|v"] = ops.linear_mxfp8_ok(rows, 3 * ch, ch)
            p["V^T"] = ops.linear_t_mxfp8_ok(rows, ch, ch)
            p["to_out"] = ops.linear_mxfp8_ok(rows, ch, ch, residual=True)
            p["temporal attention"] = ops.temporal_attn_mxfp8_ok(n, T, P, heads, 3 * ch)
            p["temporal attention, causal"] = ops.temporal_attn_mxfp8_ok(n, T, P, heads, 3 * ch, causal=True)
            p["flash self"] = ops.flash_attn_mxfp8_ok(n_groups=frames, heads=heads, nq=P, nk=P, kv_rows=P, kv_div=1, ldq=2 * ch, ldk=2 * ch, ldvt=rows)
            p["flash text"] = ops.flash_attn_mxfp8_ok(n_groups=frames, heads=heads, nq=P, nk=77, kv_rows=80, kv_div=T, ldq=ch, ldk=ch, ldvt=n * 80)
            for per_frame in (False, True):
                sets = frames if per_frame else n
                p[f"flash dual, image keys per {'frame' if per_frame else 'video'}"] = ops.flash_attn_dual_mxfp8_ok(
                    n_groups=frames, heads=heads, nq=P, nk1=77, kv_rows1=80, kv_div1=T, ldk1=ch, ldvt1=n * 80, nk2=16, kv_rows2=16,
                    kv_div2=1 if per_frame else T, ldk2=ch, ldvt2=sets * 16, ldq=ch)
        for cin in (ch, 2 * ch, 3 * ch, ch // 2):
            for cs in (False, True):
                p[f"t3 {cin} residual={cs}"] = ops.temporal_conv3_mxfp8_ok(n, T, P, ch, ch, residual=cs, colstats=cs and (T * P) % 64 == 0)
                cs9 = cs and P % 64 == 0
                p[f"c9 {cin}->{ch} rowadd colstats={cs9}"] = ops.conv3x3_mxfp8_ok(frames, H, W, cin, ch, rowadd=True, rowadd_div=T * P, colstats=cs9)
                for pitch in (None, 2 * ch, 3 * ch):
                    kw = dict(ldc=pitch, colstats=cs9, colstats_ld=pitch, colstats_col=0 if pitch is None else pitch - ch)
                    p[f"c9 {ch}->{ch} residual pitch={pitch} colstats={cs9}"] = ops.conv3x3_mxfp8_ok(frames, H, W, ch, ch, residual=True, ldr=ch, **kw)
                    p[f"c9 tailed {ch}+{cin} pitch={pitch} colstats={cs9}"] = ops.conv3x3_tail_mxfp8_ok(frames, H, W, ch, cin, ch, **kw)
        return p

    for lvl, m in enumerate(mult):
        solo = predicates(2 ** lvl, mc * m, 1)
        assert any(solo.values()), f"level {lvl}: no MX predicate accepts the solo run - the enumeration asks the wrong shapes"
        for n in range(2, cap + 1):
            many = predicates(2 ** lvl, mc * m, n)
            left = [k for k in solo if solo[k] and not many[k]]
            assert not left, f"level {lvl}, {n} videos: {left} leave the route of the solo run ({_last_error()})"
            asked += len(many)
    assert asked > 500
