"""Kernels against EXACT references, element by element (inputs and conditions: tests/exact_inputs.py, tests/test_exact_cpu.py).

 - GEMM / convolution: small-integer fp16 inputs make every product and fp32 partial sum exact, so the output must equal an int64
   reference bit for bit on every kernel, tile configuration and units route - no tolerance.
 - attention: one-hot softmaxes (the output is ONE row of V, V holds distinct integer codes) and uniform softmaxes (Q = 0: the output is
   the mean of exactly nk keys), with the readable padding of K / V^T poisoned.
 - norms: constant rows / groups (variance exactly 0) and rows of +-a (mean exactly 0).
Every bound below is exact or derived in the docstring of its test; none is taken from what a kernel was seen to do.
"""
import contextlib
import math
import os
import re

import pytest
import torch

from tests import exact_inputs as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


@contextlib.contextmanager
def knobs(**kv):
    """Force experiment knobs (include/vcx.h VCX_TUNE_*) for the length of the block; restored in a finally."""
    from viewcrafter_amd import ops
    prev = {}
    try:
        for k, v in kv.items():
            prev[k] = ops.tune_set(k, v)
        yield
        torch.cuda.synchronize()
    finally:
        for k, v in prev.items():
            ops.tune_set(k, v)


@contextlib.contextmanager
def environ(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


GUARD = 7.0


def run_linear(c, p, out_f32=None, padded=True):
    """One vcx_gemm_f16 call of a linear case: A with a row stride beyond K (the rest holds 5.0), C inside a larger buffer of GUARD
    values (5 rows behind, 8 columns beside) that must survive, rowadd as a column slice of a wider matrix (rowadd_ld)."""
    from viewcrafter_amd import ops
    M, K = p["x"].shape
    N = p["w"].shape[0]
    f32 = c["out_f32"] if out_f32 is None else out_f32
    xbig = torch.full((M, K + (8 if padded else 0)), 5.0, dtype=torch.float16, device=DEV)
    xbig[:, :K] = p["x"].to(DEV)
    big = torch.full((M + 5, N + (8 if padded else 0)), GUARD, dtype=torch.float32 if f32 else torch.float16, device=DEV)
    kw = {}
    if p["rowadd"] is not None:
        wide = torch.full((p["rowadd"].shape[0], 3 * N + 8), 9.0, device=DEV)
        wide[:, N + 4:2 * N + 4] = p["rowadd"].to(DEV)
        kw.update(rowadd=wide[:, N + 4:2 * N + 4], rowadd_div=c["rowadd_div"])
    if p["residual"] is not None:
        kw.update(residual=p["residual"].to(DEV), ldr=N)
    ops.gemm(xbig, p["w"].to(DEV), M=M, N=N, K=K, lda=xbig.stride(0), out=big, ldc=big.stride(0), alpha=c["alpha"], out_f32=f32,
             bias=None if p["bias"] is None else p["bias"].to(DEV), bias_m=c["bias"] == "m", **kw)
    torch.cuda.synchronize()
    assert bool((big[M:] == GUARD).all()) and bool((big[:, N:] == GUARD).all()), "wrote behind or beside its [M, N] block"
    return big[:M, :N]


def plan_lines(err):
    return re.findall(r"\[vcx\] gemm plan[^\n]*", err)


# ================================================================================================================ linear layers
@pytest.mark.parametrize("name,dma", [("reg_k64", 0), ("reg_k72", 0), ("reg_k72", 1), ("reg_k72_f32", 1), ("reg_k8_n4", 1), ("k1280", 0)])
def test_linear_register_staged_kernel_is_exact(name, dma, capfd):
    """csrc/gemm.hip gemm_kernel: knob GEMM_DMA = 0, and every K % 64 != 0 under the default knobs (no plan line is printed: the tiled
    engine did not run).  Two row tiles + 37 rows, one column tile + 8 columns, strided A, padded C with a guard band."""
    c = X.LINEAR_CASES[name]
    p = X.lin_problem(c)
    capfd.readouterr()
    with knobs(GEMM_DMA=dma), environ("VCX_GEMM_PLAN_TRACE", "1"):
        out = run_linear(c, p)
    assert not plan_lines(capfd.readouterr().err), "the tiled engine took a shape meant for the register-staged kernel"
    X.assert_exact(out, p["ref"], f"register-staged linear {name}")


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_linear_dma_kernel_is_exact_under_every_forced_configuration(cfg, capfd):
    """gemm_dma_kernel under knob GEMM_CFG = 0 ... 5 (6 is GEGLU only): 2 tiles + 37 rows, one column tile + 8 columns, alpha 1 / 0.5 / 2,
    bias + residual; fp16 output and (configurations 0 - 3: the 64-row ones have no fp32 epilogue) fp32 output."""
    c = X.LINEAR_CASES[f"cfg{cfg}"]
    p = X.lin_problem(c)
    capfd.readouterr()
    with knobs(GEMM_CFG=cfg), environ("VCX_GEMM_PLAN_TRACE", "1"):
        out = run_linear(c, p)
        out32 = run_linear(c, p, out_f32=True) if cfg <= 3 else None
    lines = plan_lines(capfd.readouterr().err)
    print("\n".join(lines))
    assert lines and all(f"cfg {cfg} " in l for l in lines), lines
    X.assert_exact(out, p["ref"], f"DMA linear, GEMM_CFG {cfg}")
    if out32 is not None:
        X.assert_exact(out32, p["ref"], f"DMA linear, GEMM_CFG {cfg}, fp32 output")


@pytest.mark.parametrize("name", ["bias_m", "rowadd", "f32", "k1280"])
def test_linear_epilogues_are_exact_on_the_automatic_plan(name, capfd):
    """BIAS_M (the transposed V projection), ROWADD through rowadd_ld, RESIDUAL, OUT_F32, K = 1280 ({-1, 0, 1} inputs) under the plan."""
    c = X.LINEAR_CASES[name]
    p = X.lin_problem(c)
    capfd.readouterr()
    with environ("VCX_GEMM_PLAN_TRACE", "1"):
        out = run_linear(c, p)
    lines = plan_lines(capfd.readouterr().err)
    print("\n".join(lines))
    assert lines, "expected the tiled engine"
    X.assert_exact(out, p["ref"], f"linear {name}")


def test_linear_is_exact_on_a_plan_of_two_segments(capfd):
    """The automatic plan where it splits: two whole rounds of 256 x 320 tiles + 8 row tiles, ragged (the shape of
    tests/test_gemm_tile_plan_gpu.py::test_linear_320_tiny_tail) - the seam between the segments and the last ragged tile against the
    integer reference, not against another route of the same engine."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    M = (2 * ncu + 8) * 256 - 37
    c = dict(X.LINEAR_CASES["plan_split"], K=128)
    assert X.lin_bounds(c)[1] <= X.F16_EXACT
    p = X.lin_problem(c, M=M)
    capfd.readouterr()
    with environ("VCX_GEMM_PLAN_TRACE", "1"):
        out = run_linear(c, p, padded=False)
    lines = plan_lines(capfd.readouterr().err)
    print("\n".join(lines))
    assert len(lines) == 2 and "seg 1/2" in lines[0] and "seg 2/2" in lines[1], lines
    X.assert_exact(out, p["ref"], f"linear {M} x 320 x 128 on {lines}")


@pytest.mark.parametrize("name", ["ws320", "ws960"])
def test_weight_stationary_kernels_are_exact(name, capfd):
    """csrc/gemm_ws.hip: N = K = 320 and the wide form N = 960 at M = 8192 + 37, bias + residual, padded output with a guard band.  The
    tiled engine prints no plan line: the weight-stationary kernel took the call."""
    c = X.LINEAR_CASES[name]
    p = X.lin_problem(c)
    capfd.readouterr()
    with environ("VCX_GEMM_PLAN_TRACE", "1"):
        out = run_linear(c, p, padded=name == "ws320")
    assert not plan_lines(capfd.readouterr().err)
    X.assert_exact(out, p["ref"], f"weight-stationary {name}")
    with knobs(GEMM_WS=0):                                     # the same problem on the tiled engine
        X.assert_exact(run_linear(c, p), p["ref"], f"{name} on the tiled engine")


@pytest.mark.parametrize("name,route,cfg", [("3x200", "grouped", -1), ("3x200", "loop", -1), ("5x70", "grouped", -1), ("5x70", "loop", -1),
                                            ("3x200", "grouped", 0), ("3x200", "grouped", 1), ("3x200", "grouped", 4), ("5x70", "grouped", 5),
                                            ("3x200", "grouped", 2), ("5x70", "grouped", 3), ("ws_8x1024", "ws320", -1), ("ws_8x1024", "grouped", 4)])
def test_gemm_units_is_exact_on_every_route(name, route, cfg, capfd):
    """vcx_gemm_units_f16 with ANOTHER integer weight and bias set per unit: a tile that reads the next unit's weights, or stores into the
    next unit's rows, is an exact mismatch.  unit_rows (200, 70) is no multiple of any tile height; the grouped route (the tiled engine's
    per-unit form, also under forced configurations), VCX_GEMM_UNITS_LOOP=1, and the one-launch weight-stationary route."""
    from viewcrafter_amd import ops
    units, unit_rows, N, K = X.UNITS_CASES[name]
    x, w, b, ref, _ = X.units_problem(units, unit_rows, N, K)
    capfd.readouterr()
    with knobs(GEMM_CFG=cfg), environ("VCX_GEMM_UNITS_LOOP", "1" if route == "loop" else "0"), environ("VCX_GEMM_PLAN_TRACE", "1"):
        assert ops.units_route(units * unit_rows, N, K, unit_rows) == route
        out = torch.full((units * unit_rows + 8, N), GUARD, dtype=torch.float16, device=DEV)
        ops.gemm_units(x.to(DEV), w.to(DEV), b.to(DEV), unit_rows=unit_rows, out=out[:units * unit_rows])
        torch.cuda.synchronize()
    lines = plan_lines(capfd.readouterr().err)
    print("\n".join(lines))
    if route == "grouped":
        assert lines and all(f" units " in l and f"unit_rows {unit_rows}" in l for l in lines), lines
    elif route == "loop":
        assert len(lines) >= units and not any(" units " in l for l in lines), lines
    else:
        assert not lines
    assert bool((out[units * unit_rows:] == GUARD).all())
    X.assert_exact(out[:units * unit_rows], ref, f"gemm_units {name} {route} GEMM_CFG {cfg}")


# ================================================================================================================ convolutions
def run_conv(c, p):
    from viewcrafter_amd import ops
    from viewcrafter_amd.packing import conv_slab_major, pack_conv
    taps = c["kh"] * c["kw"]
    slabk = conv_slab_major(c["cin"], taps) if c["slabk"] is None else c["slabk"]
    w = p["w"]
    wp = pack_conv(w) if slabk == conv_slab_major(c["cin"], taps) else w.reshape(c["cout"], c["cin"], taps).permute(0, 2, 1).reshape(c["cout"], -1).contiguous()
    if p["tail_w"]:
        wp = torch.cat([wp] + p["tail_w"], dim=1).contiguous()
    Ho, Wo = p["out_hw"]
    M, N, K = c["n"] * Ho * Wo, c["cout"], wp.shape[1]
    geom = dict(in_h=c["H"], in_w=c["W"], out_h=Ho, out_w=Wo, cin=c["cin"], kh=c["kh"], kw=c["kw"], stride=c["stride"], pad_h=c["pad"][0], pad_w=c["pad"][1],
                ups=c["ups"], slabk=slabk)
    big = torch.full((M + 5, N + 8), GUARD, dtype=torch.float16, device=DEV)
    kw = {}
    if p["residual"] is not None:
        kw.update(residual=p["residual"].to(DEV), ldr=N)
    if p["tail_src"]:
        srcs = []
        for t in p["tail_src"]:                                    # sources with a row stride beyond their width
            buf = torch.full((M, t.shape[1] + 8), 5.0, dtype=torch.float16, device=DEV)
            buf[:, :t.shape[1]] = t.to(DEV)
            srcs.append(buf[:, :t.shape[1]])
        kw.update(tail=srcs)
    x = p["x"].to(DEV)
    ops.gemm(x, wp.to(DEV), M=M, N=N, K=K, lda=x.stride(2), out=big, ldc=N + 8, bias=p["bias"].to(DEV), conv=geom, **kw)
    torch.cuda.synchronize()
    assert bool((big[M:] == GUARD).all()) and bool((big[:, N:] == GUARD).all()), "wrote behind or beside its [M, N] block"
    return big[:M, :N].reshape(c["n"], Ho, Wo, N)


@pytest.mark.parametrize("name", sorted(X.CONV_CASES))
def test_convolutions_are_exact(name, capfd):
    """Implicit-GEMM convolutions against F.conv2d on int64: 3 x 3 at stride 1 / 2, fused nearest-2x, the VAE's asymmetric pad, 1 x 1,
    temporal (3,1,1), slab-major and tap-major K order, the K tail with one and two sources, images of 1 x 1, 1 x W and H x 1 pixels.
    cin % 64 == 0 with cout % 8 == 0 runs on the DMA kernel under the plan and under every forced configuration 0 - 5, and (without a
    K tail) on the register-staged kernel under GEMM_DMA = 0; cin = 8 / 72 is the register-staged kernel's."""
    c = X.CONV_CASES[name]
    p = X.conv_problem(c)
    dma = c["cin"] % 64 == 0 and c["cout"] % 8 == 0
    capfd.readouterr()
    with environ("VCX_GEMM_PLAN_TRACE", "1"):
        out = run_conv(c, p)
    lines = plan_lines(capfd.readouterr().err)
    print("\n".join(lines))
    assert bool(lines) == dma, f"cin {c['cin']}: expected the {'DMA' if dma else 'register-staged'} kernel"
    X.assert_exact(out, p["ref"], f"conv {name}")
    if dma:
        for cfg in range(6):
            with knobs(GEMM_CFG=cfg):
                X.assert_exact(run_conv(c, p), p["ref"], f"conv {name}, GEMM_CFG {cfg}")
        if not c["tails"]:
            with knobs(GEMM_DMA=0):
                X.assert_exact(run_conv(c, p), p["ref"], f"conv {name}, register-staged kernel")


# ================================================================================================================ attention
def kv_layout(k, v, kv_rows, pad_k, pad_v, pad_v8=None):
    """k, v [Gk, nk, C] -> K [Gk * kv_rows, C], V^T [C, Gk * kv_rows].  K rows [nk, kv_rows) hold pad_k; V^T columns [nk8, kv_rows) hold
    pad_v and the columns [nk, nk8) up to the next multiple of 8 - which the kernels read in 16-byte pieces - pad_v8 (default pad_v)."""
    Gk, nk, C = k.shape
    nk8 = (nk + 7) // 8 * 8
    kp = torch.full((Gk, kv_rows, C), pad_k, dtype=torch.float16)
    vp = torch.full((Gk, kv_rows, C), pad_v, dtype=torch.float16)
    vp[:, nk:nk8] = pad_v if pad_v8 is None else pad_v8
    kp[:, :nk] = k
    vp[:, :nk] = v
    return kp.view(Gk * kv_rows, C).to(DEV), vp.view(Gk * kv_rows, C).t().contiguous().to(DEV)


NAN, INF = float("nan"), float("inf")
# (name, K padding, V^T padding beyond the next multiple of 8, V^T padding inside the last 16-byte piece).  include/vcx.h: K rows >= nk and
# V^T columns >= nk8 are never used, whatever they hold; V^T columns [nk, nk8) must be FINITE (they meet a probability of exactly 0 on
# the matrix pipe) - any finite value gives the same bits.
PADDINGS = [("finite", X.PAD_FINITE, X.PAD_FINITE, X.PAD_FINITE), ("K NaN", NAN, X.PAD_FINITE, X.PAD_FINITE), ("V^T NaN", X.PAD_FINITE, NAN, -X.PAD_FINITE),
            ("K and V^T Inf", INF, INF, 0.0)]


def log2_q(q, scale):
    return (q.float() * (scale * 1.4426950408889634)).half()


def flash_call(impl, q, kd, vtd, out, *, G, heads, nq, nk, kv_rows, kv_div, scale, log2):
    from viewcrafter_amd import ops
    C = heads * 64
    if impl == "d512":
        ops.flash_attn_d512(q, kd, vtd, out, n_groups=G, nq=nq, nk=nk, kv_rows=kv_rows, ldq=512, ldk=512, ldvt=vtd.shape[1], ldo=512, scale=scale)
    else:
        ops.flash_attn(q, kd, vtd, out, n_groups=G, heads=heads, nq=nq, nk=nk, kv_rows=kv_rows, kv_div=kv_div, ldq=C, ldk=C, ldvt=vtd.shape[1], ldo=C,
                       scale=0.0 if log2 else scale, log2_logits=log2)
    torch.cuda.synchronize()


FLASH_IMPLS = {"qb1": dict(FLASH_IMPL=1, FLASH_QB=1), "qb2": dict(FLASH_IMPL=1, FLASH_QB=2), "qb1_log2": dict(FLASH_IMPL=1, FLASH_QB=1),
               "qb2_log2": dict(FLASH_IMPL=1, FLASH_QB=2), "v2": dict(FLASH_IMPL=2), "d512": {}}


@pytest.mark.parametrize("impl,nk,nq", [("qb1", 135, 100), ("qb2", 135, 300), ("qb1_log2", 77, 100), ("qb2_log2", 200, 300), ("v2", 4096, 256), ("v2", 4160, 300),
                                        ("d512", 135, 136)])
def test_flash_attention_one_hot_selects_the_right_value_row(impl, nk, nq):
    """q_i = 16 k_pi(i) over random +-1 keys: the winning logit leads by >= 30 nats (asserted on the CPU from the inputs), so the softmax is
    one-hot - the winner's probability is 1 up to the packed fp16 rounding when a deferred running max leaves it at 2^x, x <= 8, the
    losers' e^-30 pack to exactly 0 - and O_i = V[pi(i)], distinct integer codes.  Bound 2^-10 |v| per element: two fp16 half-ulps (the
    packed probability, the output rounding); a code of 0 must come out as 0.  4 query groups on 2 key / value groups (kv_div = 2) and
    2 heads: a wrong key tile, head, group or V^T column is off by >= 1."""
    d512 = impl == "d512"
    heads, D = (1, 512) if d512 else (2, 64)
    Gk, kv_div = (2, 1) if d512 else (2, 2)
    G, C = Gk * kv_div, heads * D
    scale = D ** -0.5
    q, k, v, perm = X.one_hot_problem(Gk, heads, nk, kv_div * nq, d=D, seed=nk)
    assert X.one_hot_gap(q[:, :256], k, perm[:, :, :256], scale) >= X.ONE_HOT_GAP_NATS
    log2 = impl.endswith("log2") or impl == "v2"
    qd = q.reshape(G * nq, C)                                  # group g = gk * kv_div + j takes the queries [j nq, (j + 1) nq) of key group gk
    qd = (log2_q(qd, scale) if log2 else qd).to(DEV)
    kv_rows = (nk + 7) // 8 * 8 + 16
    kd, vtd = kv_layout(k.reshape(Gk, nk, C), v.reshape(Gk, nk, C), kv_rows, X.PAD_FINITE, X.PAD_FINITE)
    out = torch.full((G * nq + 8, C), GUARD, dtype=torch.float16, device=DEV)
    with knobs(**FLASH_IMPLS[impl]):
        flash_call(impl, qd, kd, vtd, out, G=G, heads=heads, nq=nq, nk=nk, kv_rows=kv_rows, kv_div=kv_div, scale=scale, log2=log2)
    want = torch.stack([torch.stack([v[gk, perm[gk, h], h] for h in range(heads)], dim=1) for gk in range(Gk)]).double()   # [Gk, kv_div nq, heads, D]
    want = want.reshape(G * nq, C)
    assert bool((out[G * nq:] == GUARD).all())
    X.assert_elementwise(out[:G * nq], want, want.abs() * 2.0 ** -10, f"flash one-hot {impl} nk {nk}")


@pytest.mark.parametrize("impl,nk", [(i, n) for i in ("qb1", "qb2", "qb2_log2", "d512") for n in X.FLASH_UNIFORM_NK] + [("v2", 4096), ("v2", 4160)])
def test_flash_attention_uniform_is_the_mean_of_exactly_nk_keys_whatever_the_padding_holds(impl, nk):
    """Q = 0: every probability is exactly 1 (2^0), the row sum exactly nk, the fp32 sum of nk integer values exact; the output is
    sum * (1 / nk) rounded to fp16 - within ONE fp16 ulp of the fp64 mean (half an ulp of rounding, two fp32 roundings before it).
    Padding of 1000 in K rows / V^T columns [nk, kv_rows): a kernel that counts one padding key is off by far more (CPU test).
    Then the padding poisoned (PADDINGS): the same BITS as with finite padding."""
    d512 = impl == "d512"
    heads, D = (1, 512) if d512 else (2, 64)
    G, C = 2, heads * D
    nq = 40 if nk > 1000 else 70
    kv_rows = (nk + 7) // 8 * 8 + 16
    vals, means = zip(*[X.uniform_values(nk, C, seed=g) for g in range(G)])
    v = torch.stack(vals)                                      # [G, nk, C]
    want = torch.stack(means)[:, None, :].expand(G, nq, C).reshape(G * nq, C)
    k = X.int_tensor((G, nk, C), -1, 1, 77)
    q = torch.zeros((G * nq, C), dtype=torch.float16, device=DEV)
    log2 = impl.endswith("log2") or impl == "v2"
    outs = {}
    with knobs(**FLASH_IMPLS[impl]):
        for pname, pk, pv, pv8 in PADDINGS:
            kd, vtd = kv_layout(k, v, kv_rows, pk, pv, pv8)
            out = torch.full((G * nq, C), GUARD, dtype=torch.float16, device=DEV)
            flash_call(impl, q, kd, vtd, out, G=G, heads=heads, nq=nq, nk=nk, kv_rows=kv_rows, kv_div=1, scale=D ** -0.5, log2=log2)
            outs[pname] = out.cpu()
    X.assert_elementwise(outs["finite"], want, X.f16_ulp(want), f"flash uniform {impl} nk {nk}")
    for pname in outs:
        assert torch.equal(outs[pname], outs["finite"]), f"flash uniform {impl} nk {nk}: padding '{pname}' changed {int((outs[pname] != outs['finite']).sum())} elements"


def dual_sets(nk1, nk2, Gk, heads, nq_total, seed):
    """Two key sets over ONE pool of +-1 keys so that a query is one-hot in both: set 2 holds the pool's keys (some of them where it is
    shorter, extra random ones where it is longer) in another order.  -> q, k1, v1, k2, v2, j1, j2 (the selected keys per set)."""
    g = torch.Generator().manual_seed(seed)
    C = heads * 64
    pool = (torch.randint(0, 2, (Gk, max(nk1, nk2), heads, 64), generator=g) * 2 - 1).to(torch.float16)
    k1 = pool[:, :nk1]
    sig = torch.stack([torch.randperm(max(nk1, nk2), generator=g)[:nk2] for _ in range(Gk)])          # k2[j] = pool[sig[j]]
    k2 = torch.stack([pool[gi, sig[gi]] for gi in range(Gk)])
    j1 = torch.empty((Gk, nq_total), dtype=torch.int64)
    j2 = torch.empty((Gk, nq_total), dtype=torch.int64)
    for gi in range(Gk):
        both = torch.nonzero(sig[gi] < nk1).squeeze(1)         # positions of set 2 whose key is in set 1 as well
        pick = both[torch.randint(0, both.numel(), (nq_total,), generator=g)]
        j2[gi], j1[gi] = pick, sig[gi][pick]
    q = X.ONE_HOT_BETA * torch.stack([k1[gi, j1[gi]] for gi in range(Gk)])                                # [Gk, nq_total, heads, 64]
    v1 = torch.stack([X.v_codes(nk1 + 64)[3 * gi:][:nk1] for gi in range(Gk)])[:, :, None, :].expand(Gk, nk1, heads, 64)
    v2 = torch.stack([X.v_codes(nk2 + 64)[17 + 5 * gi:][:nk2] for gi in range(Gk)])[:, :, None, :].expand(Gk, nk2, heads, 64)
    hs = torch.arange(heads).view(1, 1, heads, 1).to(torch.float16)
    return q, k1, (v1 + hs).contiguous(), k2, (v2 - 2 * hs).contiguous(), j1, j2


@pytest.mark.parametrize("form,T,nk1,nk2,nq,log2", [("resident", 3, 77, 256, 200, True), ("resident_first", 3, 77, 256, 200, True), ("resident", 2, 33, 100, 77, False),
                                                    ("resident_first", 2, 33, 100, 77, False), ("flash_dual_qb1", 1, 77, 16, 100, True), ("flash_dual_qb2", 1, 77, 16, 300, False),
                                                    ("flash_dual_qb1", 1, 135, 300, 100, False)])
def test_dual_cross_attention_one_hot_and_poisoned_padding(form, T, nk1, nk2, nq, log2):
    """vcx_attn_flash_dual_d64_f16 - the LDS-resident forms (knob XATTN_RESIDENT 1 and 2; both sets shared by the T frames of a video)
    and the dual form of the flash kernel: one-hot in BOTH key sets, O_i = V1[j1(i)] + V2[j2(i)] within 2^-10 (|v1| + |v2|) (as in the
    single form; the two results are added in fp32 or as exact fp16 integers); the same bits with the padding poisoned."""
    from viewcrafter_amd import ops
    heads, B = 2, 2
    C, G = heads * 64, B * T
    r1, r2 = (nk1 + 7) // 8 * 8 + 8, (nk2 + 7) // 8 * 8 + 8
    q, k1, v1, k2, v2, j1, j2 = dual_sets(nk1, nk2, B, heads, T * nq, seed=nk1 + nk2)
    assert min(X.one_hot_gap(q, k1, j1[:, None, :].expand(B, heads, T * nq), 0.125), X.one_hot_gap(q, k2, j2[:, None, :].expand(B, heads, T * nq), 0.125)) >= X.ONE_HOT_GAP_NATS
    qd = q.reshape(G * nq, C)
    qd = (log2_q(qd, 0.125) if log2 else qd).to(DEV)
    want = torch.stack([v1[b, j1[b]].double() + v2[b, j2[b]].double() for b in range(B)]).reshape(G * nq, C)
    bound = torch.stack([v1[b, j1[b]].double().abs() + v2[b, j2[b]].double().abs() for b in range(B)]).reshape(G * nq, C) * 2.0 ** -10
    kn = dict(resident=dict(XATTN_RESIDENT=1), resident_first=dict(XATTN_RESIDENT=2), flash_dual_qb1=dict(XATTN_RESIDENT=0, FLASH_QB=1),
              flash_dual_qb2=dict(XATTN_RESIDENT=0, FLASH_QB=2))[form]
    outs = {}
    with knobs(**kn):
        for pname, pk, pv, pv8 in PADDINGS:
            k1d, vt1 = kv_layout(k1.reshape(B, nk1, C), v1.reshape(B, nk1, C), r1, pk, pv, pv8)
            k2d, vt2 = kv_layout(k2.reshape(B, nk2, C), v2.reshape(B, nk2, C), r2, pk, pv, pv8)
            out = torch.full((G * nq + 8, C), GUARD, dtype=torch.float16, device=DEV)
            ops.flash_attn_dual(qd, k1d, vt1, k2d, vt2, out, n_groups=G, heads=heads, nq=nq, nk1=nk1, kv_rows1=r1, kv_div1=T, ldk1=C, ldvt1=B * r1,
                                nk2=nk2, kv_rows2=r2, kv_div2=T, ldk2=C, ldvt2=B * r2, ldq=C, ldo=C, scale=0.125, log2_logits=log2)
            torch.cuda.synchronize()
            outs[pname] = out.cpu()
    assert bool((outs["finite"][G * nq:] == GUARD).all())
    X.assert_elementwise(outs["finite"][:G * nq], want, bound, f"dual one-hot {form}")
    for pname in outs:
        assert torch.equal(outs[pname], outs["finite"]), f"dual {form}: padding '{pname}' changed {int((outs[pname] != outs['finite']).sum())} elements"


def temporal_layout(q, k, v):
    """[B, T, P, heads, 64] each -> qkv [(b t p), 3 C]"""
    B, T, P, heads, _ = q.shape
    C = heads * 64
    return torch.cat([t.reshape(B * T * P, C) for t in (q, k, v)], dim=1).contiguous().to(DEV)


@pytest.mark.parametrize("T", X.TEMPORAL_UNIFORM_T)
@pytest.mark.parametrize("causal", [False, True])
def test_temporal_attention_uniform_means_and_one_hot(T, causal):
    """vcx_attn_temporal_d64[_masked]_f16 over T frames per (pixel, head), T on both sides of the one-tile / 2 x 2-tile switch at 32.
    Uniform (Q = 0): the mean over the T frames - the causal kernel the PREFIX means over frames <= t - within one fp16 ulp of the fp64
    mean (derivation: the flash test above).  One-hot: q_t = 16 k_pi(t) (pi(t) <= t under the causal mask), O_t = V[pi(t)] within
    2^-10 |v|; the codes differ between frames, pixels and heads, so a wrong frame, pixel or head is off by >= 1."""
    from viewcrafter_amd import ops
    B, P, heads = 2, 9, 2
    C = heads * 64
    g = torch.Generator().manual_seed(T)
    v = torch.randint(-30, 31, (B, T, P, heads, 64), generator=g).to(torch.float16)
    k = (torch.randint(0, 2, (B, T, P, heads, 64), generator=g) * 2 - 1).to(torch.float16)
    kw = dict(B=B, T=T, P=P, heads=heads, ld=3 * C, k_off=C, v_off=2 * C, ldo=C, scale=0.125, causal=causal)
    out = torch.full((B * T * P + 8, C), GUARD, dtype=torch.float16, device=DEV)
    ops.temporal_attn(temporal_layout(torch.zeros_like(k), k, v), out, **kw)
    torch.cuda.synchronize()
    vd = v.double()
    want = (vd.cumsum(1) / torch.arange(1, T + 1, dtype=torch.float64).view(1, T, 1, 1, 1)) if causal else vd.mean(1, keepdim=True).expand_as(vd)
    want = want.reshape(B * T * P, C)
    assert bool((out[B * T * P:] == GUARD).all())
    X.assert_elementwise(out[:B * T * P], want, X.f16_ulp(want), f"temporal uniform T {T} causal {causal}")
    # one-hot
    pi = torch.stack([torch.randint(0, t + 1 if causal else T, (B, P, heads), generator=g) for t in range(T)], dim=1)      # [B, T, P, heads]
    idx = pi[..., None].expand(B, T, P, heads, 64)
    q = X.ONE_HOT_BETA * k.gather(1, idx)
    codes = ((7 * torch.arange(T).view(1, T, 1, 1, 1) + 3 * torch.arange(64).view(1, 1, 1, 1, 64) + 11 * torch.arange(P).view(1, 1, P, 1, 1)
              + 5 * torch.arange(heads).view(1, 1, 1, heads, 1) + 13 * torch.arange(B).view(B, 1, 1, 1, 1)) % 61 - 30).to(torch.float16)
    if T > 1:       # the gap, from the inputs: scale * beta * (64 - the best other key's dot product) >= 30 nats
        s = 0.125 * torch.einsum("btphd,bsphd->bphts", q.double(), k.double())
        if causal:
            s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))
        win = s.gather(-1, pi.permute(0, 2, 3, 1)[..., None])
        other = s.scatter(-1, pi.permute(0, 2, 3, 1)[..., None], float("-inf")).max(-1, keepdim=True).values
        assert float((win - other).min()) >= X.ONE_HOT_GAP_NATS
    out.fill_(GUARD)
    ops.temporal_attn(temporal_layout(q, k, codes), out, **kw)
    torch.cuda.synchronize()
    want = codes.gather(1, idx).double().reshape(B * T * P, C)
    X.assert_elementwise(out[:B * T * P], want, want.abs() * 2.0 ** -10, f"temporal one-hot T {T} causal {causal}")


@pytest.mark.parametrize("rows,n,ld", [(37, 135, 144), (100, 512, 520), (5, 1, 8), (70, 33, 48)])
def test_softmax_rows_one_hot_and_uniform(rows, n, ld):
    """vcx_softmax_rows_f16.  One-hot: one logit of 40 over zeros - the winner is 1 / (1 + (n - 1) e^-40) = 1 in fp32, the others e^-40
    round to 0 in fp16: EXACTLY one-hot.  Uniform: equal logits give 1 / n within one fp16 ulp (an fp32 quotient, then the rounding).
    The columns up to the next multiple of 8 become 0, everything behind them is untouched."""
    from viewcrafter_amd import ops
    n8 = (n + 7) // 8 * 8
    g = torch.Generator().manual_seed(n)
    pi = torch.randint(0, n, (rows,), generator=g)
    x = torch.full((rows, ld), 3.0, dtype=torch.float16)
    x[:, :n] = 0
    x[torch.arange(rows), pi] = 40.0
    y = x.clone().to(DEV)
    ops.softmax_rows_(y, n=n)
    want = torch.zeros((rows, n8), dtype=torch.float64)
    want[torch.arange(rows), pi] = 1.0
    X.assert_elementwise(y[:, :n8], want, torch.zeros_like(want), f"softmax one-hot n {n}")
    assert bool((y[:, n8:] == 3.0).all())
    x[:, :n] = -5.0
    y = x.clone().to(DEV)
    ops.softmax_rows_(y, n=n)
    want = torch.zeros((rows, n8), dtype=torch.float64)
    want[:, :n] = 1.0 / n
    X.assert_elementwise(y[:, :n8], want, X.f16_ulp(want) * (want > 0), f"softmax uniform n {n}")
    assert bool((y[:, n8:] == 3.0).all())


def test_projected_context_padding_is_finite_and_zero():
    """include/vcx.h asks for FINITE V^T columns between nk and the next multiple of 8.  The host side guarantees it: every K / V^T operand
    is the OUTPUT of a projection GEMM over ALL kv_rows rows of a zero-initialised, zero-padded input (UNetModel._context_kv ->
    project_context: 77 text rows in 80; SpatialTransformer / AttnBlock pad_frames and the Resampler's kv input are torch.zeros too) -
    no torch.empty buffer reaches a kernel as K or V^T.  Here: the padding rows / columns of the projected text context are exactly 0
    (no bias in to_k / to_v), everything is finite, with a context as long as 77 tokens and with a shorter one."""
    from tests.tiny_config import TINY_UNET
    from tests.util import load_synth
    from oracle.weights import synth_input
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    load_synth(m)
    m = m.to(DEV)
    t = 4
    for L in (77 + 64, 50):
        ctx = synth_input("smoke_ctx", (2, 77 + 64, TINY_UNET["context_dim"]))[:, :L].contiguous().to(DEV)
        with torch.no_grad():
            kvs = m._context_kv(ctx, t)
        n = 0
        for key, per_block in kvs.items():
            if key == "_keepalive":
                continue
            for kv in per_block:
                n += 1
                nt = min(L, 77)
                assert kv.n_txt == nt and kv.n_txt_rows == 2 * 80
                assert bool(torch.isfinite(kv.k_txt).all()) and bool(torch.isfinite(kv.vt_txt).all())
                assert bool((kv.k_txt.view(2, 80, -1)[:, nt:] == 0).all()) and bool((kv.vt_txt.view(-1, 2, 80)[:, :, nt:] == 0).all())
                if kv.k_img is not None:
                    assert kv.n_img % 8 == 0 or kv.img_per_frame
                    assert bool(torch.isfinite(kv.k_img).all()) and bool(torch.isfinite(kv.vt_img).all())
        assert n > 0


# ================================================================================================================ norms
EPS = 1e-5
RSTD_REL = 2.0 ** -22      # fp32 rounding of rstd = rsqrt(var + eps): eps and the sum rounded to fp32, a reciprocal square root good to an ulp or two


@pytest.mark.parametrize("C", [64, 320, 1280])
def test_layernorm_and_rowstats_on_constant_rows(C):
    """A row of C copies of an integer c: the fp32 sum is exact, the mean is c, every deviation is 0 and so is the variance:
    vcx_rowstats_f16 returns (c, 1 / sqrt(eps)) to fp32 rounding and vcx_layernorm_f16 exactly fp16(beta) - (x - mean) rstd gamma is 0."""
    from viewcrafter_amd import ops
    cs = torch.tensor([0, 1, -1, 3, -7, 100, -100, 2047, 12, 5, -64], dtype=torch.float16)
    x = cs[:, None].expand(cs.numel(), C).contiguous().to(DEV)
    st = ops.row_stats(x, EPS).cpu().double()
    X.assert_elementwise(st[:, :1], cs.double()[:, None], cs.double().abs()[:, None] * 2.0 ** -23, f"rowstats mean C {C}")
    r = 1.0 / math.sqrt(EPS)
    X.assert_elementwise(st[:, 1:], torch.full((cs.numel(), 1), r, dtype=torch.float64), torch.full((cs.numel(), 1), r * RSTD_REL, dtype=torch.float64), f"rowstats rstd C {C}")
    g = torch.Generator().manual_seed(C)
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).to(DEV)
    beta = torch.randn(C, generator=g).to(DEV)
    y = ops.layer_norm(x, gamma, beta, EPS).cpu()
    want = beta.cpu().half()[None, :].expand(cs.numel(), C)
    assert torch.equal(y, want), f"layernorm of constant rows, C {C}: {int((y != want).sum())} elements differ from fp16(beta); rows {torch.nonzero((y != want).any(1)).flatten().tolist()}"


@pytest.mark.parametrize("C", [64, 320])
def test_layernorm_on_rows_of_plus_minus_a(C):
    """A row of C / 2 values +a and C / 2 values -a in random order: the mean is exactly 0 (the integer sum is exact), the variance a^2.
    rowstats: (0, 1 / sqrt(a^2 + eps)) to fp32 rounding; layernorm per element against fp64 within one fp16 ulp of the reference (the
    output rounding, with room for the fp32 arithmetic in front of it) + the fp32 rounding of rstd carried by |y - beta|."""
    from viewcrafter_amd import ops
    a = torch.tensor([1, 2, 3, 10, 100, 1000], dtype=torch.float64)
    g = torch.Generator().manual_seed(C + 1)
    sign = torch.stack([torch.cat([torch.ones(C // 2), -torch.ones(C // 2)])[torch.randperm(C, generator=g)] for _ in a]).double()
    x64 = sign * a[:, None]
    x = x64.half().to(DEV)
    st = ops.row_stats(x, EPS).cpu().double()
    assert bool((st[:, 0] == 0).all()), f"mean of +-a rows: {st[:, 0].tolist()}"
    r = 1.0 / torch.sqrt(a * a + EPS)
    X.assert_elementwise(st[:, 1:], r[:, None], r[:, None] * RSTD_REL, f"rowstats rstd of +-a rows, C {C}")
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).to(DEV)
    beta = torch.randn(C, generator=g).to(DEV)
    y = ops.layer_norm(x, gamma, beta, EPS)
    scaled = x64 * r[:, None] * gamma.cpu().double()
    want = scaled + beta.cpu().double()
    X.assert_elementwise(y, want, X.f16_ulp(want) + 4 * RSTD_REL * scaled.abs(), f"layernorm of +-a rows, C {C}")


def _betas_off_the_rounding_ties(C, seed):
    """fp32 betas whose silu (fp64) lies at least 2^-18 (relative) from the nearest fp16 rounding tie: the kernel evaluates silu in fp32
    (an exponential and a reciprocal good to a few ulps, 2^-21 relative at most), which then cannot change the fp16 it rounds to."""
    g = torch.Generator().manual_seed(seed)
    beta = torch.randn(C, generator=g)
    s = torch.nn.functional.silu(beta.double())
    ulp = X.f16_ulp(s)
    frac = (s / ulp) - torch.floor(s / ulp)
    near = (frac - 0.5).abs() * ulp < s.abs() * 2.0 ** -18
    beta[near] = 0.5          # silu(0.5) = 0.3112296656...: 0.46 ulp (2^-12) above fp16 0.31103515625's tie? checked below, not assumed
    s = torch.nn.functional.silu(beta.double())
    ulp = X.f16_ulp(s)
    frac = (s / ulp) - torch.floor(s / ulp)
    assert bool(((frac - 0.5).abs() * ulp >= s.abs() * 2.0 ** -18).all())
    return beta


@pytest.mark.parametrize("n,pix,C", [(3, 77, 64), (2, 1000, 320), (2, 4096, 640)])
def test_groupnorm_on_input_constant_per_image_and_group(n, pix, C):
    """x constant (an integer) per (image, group): the statistics pass gives (c, 0) - the variance EXACTLY 0, never negative, never NaN
    (every deviation from a running mean of c is 0) - and the apply pass exactly fp16(beta) / fp16(silu(beta))."""
    from viewcrafter_amd import ops
    g = torch.Generator().manual_seed(pix)
    c = torch.randint(-100, 101, (n, 1, 32, 1), generator=g).to(torch.float16)
    c[0, 0, 0, 0], c[0, 0, 1, 0] = 2047, 0
    x = c.expand(n, pix, 32, C // 32).reshape(n, pix, C).contiguous().to(DEV)
    st = ops.group_norm_stats(x).cpu().double()
    assert bool((st[..., 1] == 0).all()), f"variance of constant groups: min {float(st[..., 1].min())!r} max {float(st[..., 1].max())!r}"
    X.assert_elementwise(st[..., 0], c.double().view(n, 32), c.double().view(n, 32).abs() * 2.0 ** -23, "groupnorm mean of constant groups")
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).to(DEV)
    beta = _betas_off_the_rounding_ties(C, pix)
    for silu in (False, True):
        y = ops.group_norm(x, gamma, beta.to(DEV), 1e-6, silu).cpu()
        want = (torch.nn.functional.silu(beta.double()) if silu else beta.double()).half()[None, None, :].expand(n, pix, C)
        assert torch.equal(y, want), f"groupnorm apply (silu {silu}) on constant groups: {int((y != want).sum())} of {y.numel()} elements differ"


def test_groupnorm_statistics_from_column_moments_of_a_constant_output():
    """The COLSTATS epilogue + vcx_groupnorm_stats_from_colstats_f32 on an output that is constant per (image, group) - zero weights, an
    integer bias per group, an integer per-image rowadd: mean c to fp32 rounding, variance exactly 0, never negative or NaN."""
    from viewcrafter_amd import ops
    n, pix, K, N = 3, 256, 64, 320
    g = torch.Generator().manual_seed(5)
    x = X.int_tensor((n * pix, K), -3, 3, 11).to(DEV)
    w = torch.zeros((N, K), dtype=torch.float16, device=DEV)
    bias = torch.randint(-50, 51, (32, 1), generator=g).float().expand(32, N // 32).reshape(N).contiguous()
    ra = torch.randint(-50, 51, (n, 1), generator=g).float().expand(n, N).contiguous()
    assert ops.colstats_ok(n * pix, pix, K, N)
    cs = ops.colstats_buffer(n * pix, N, DEV)
    out = ops.linear(x, w, bias.to(DEV), rowadd=ra.to(DEV), rowadd_div=pix, colstats=cs)
    want = (bias[None, :] + ra[:, :1]).to(torch.int64)[:, None, :].expand(n, pix, N).reshape(n * pix, N)
    X.assert_exact(out, want.contiguous(), "constant output")
    st = ops.group_norm_stats_from_colstats(cs, n, pix, N).cpu().double()
    assert bool((st[..., 1] == 0).all()), f"variance from column moments: min {float(st[..., 1].min())!r} max {float(st[..., 1].max())!r}"
    c = want.view(n, pix, 32, N // 32)[:, 0, :, 0].double()
    X.assert_elementwise(st[..., 0], c, c.abs() * 2.0 ** -23, "mean from column moments")
