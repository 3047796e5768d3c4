"""Inputs with exactly known results, and per-element assertions, for tests/test_exact_gpu.py (conditions checked on the CPU by
tests/test_exact_cpu.py).

Small integers in fp16 make every product and every fp32 partial sum of a GEMM or convolution exact (while the sums stay below
2^24), so a correct kernel reproduces an integer reference bit for bit in ANY summation order and on ANY tile plan; one wrong
element, tile or tap is an exact mismatch instead of a change in the fourth digit of a whole-tensor norm.
"""
import torch

F32_EXACT = 1 << 24      # integers up to here are exact in fp32
F16_EXACT = 2048         # ... and up to here in fp16


def int_tensor(shape, lo, hi, seed):
    """Uniform integers in [lo, hi] as fp16 (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float16)


def _where(bad):
    """Count of wrong elements, the first wrong index and its row / column modulo the tile sizes (a tile edge shows here)."""
    bad2 = bad.reshape(-1, bad.shape[-1]) if bad.dim() >= 1 else bad.reshape(1, 1)
    idx = torch.nonzero(bad2)
    r, c = int(idx[0, 0]), int(idx[0, 1])
    first = tuple(int(v) for v in torch.nonzero(bad)[0]) if bad.dim() >= 1 else ()
    mods = ", ".join(f"mod {m}: row {r % m} col {c % m}" for m in (64, 128, 256))
    return (f"{int(bad.sum())} of {bad.numel()} elements wrong; first at {first} = flat row {r}, column {c} ({mods}); "
            f"wrong rows {int(bad2.any(1).sum())}, wrong columns {int(bad2.any(0).sum())}")


def assert_exact(out, ref_int64, name):
    """out (fp16 / fp32, any device) must hold exactly the integers of ref_int64 (CPU)."""
    assert ref_int64.dtype == torch.int64
    got = out.detach().cpu()
    assert tuple(got.shape) == tuple(ref_int64.shape), f"{name}: shape {tuple(got.shape)} != {tuple(ref_int64.shape)}"
    want = ref_int64.to(got.dtype)
    assert torch.equal(want.to(torch.int64), ref_int64), f"{name}: the reference is not representable in {got.dtype} (a mistake of the test)"
    if torch.equal(got, want):
        return
    bad = ~(got == want)                       # (a NaN is wrong too)
    r, c = torch.nonzero(bad.reshape(-1, bad.shape[-1]))[0].tolist()
    g2, w2 = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    raise AssertionError(f"{name}: {_where(bad)}; got {float(g2[r, c])} want {float(w2[r, c])}")


def assert_elementwise(out, ref64, bound64, name):
    """|out - ref| <= bound for every element (fp64, CPU); a non-finite output fails."""
    got = out.detach().cpu().double()
    ref64 = ref64.detach().cpu().double()
    assert tuple(got.shape) == tuple(ref64.shape), f"{name}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    bound = torch.as_tensor(bound64, dtype=torch.float64).expand_as(ref64)
    err = (got - ref64).abs()
    bad = ~(err <= bound)
    if not bool(bad.any()):
        return
    r, c = torch.nonzero(bad.reshape(-1, bad.shape[-1]))[0].tolist()
    g2, w2, b2 = got.reshape(-1, got.shape[-1]), ref64.reshape(-1, got.shape[-1]), bound.reshape(-1, got.shape[-1])
    raise AssertionError(f"{name}: {_where(bad)}; got {float(g2[r, c])!r} want {float(w2[r, c])!r} +- {float(b2[r, c]):.3e}")


def f16_ulp(x64):
    """The spacing of fp16 at |x| (fp64 tensor): 2^(floor(log2 |x|) - 10), 2^-24 in the subnormal range."""
    e = torch.floor(torch.log2(x64.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


# ------------------------------------------------------------------------------------------------------------------ linear layers
# A case: M, N, K, ax / aw = the integer range of inputs / weights, wmul (weights are wmul * integers: 2 under alpha = 0.5 so that
# alpha * sum stays an integer), alpha, bias "n" / "m" / None, rowadd_div (0: none), residual, out_f32.  Addends are integers in
# [-8, 8].  Rows: two row tiles of the configuration under test + a ragged 37; columns: one column tile + 8.
ADD = 8


def lin_case(M, N, K, ax=3, aw=3, wmul=1, alpha=1.0, bias="n", rowadd_div=0, residual=True, out_f32=False, seed=0):
    return dict(M=M, N=N, K=K, ax=ax, aw=aw, wmul=wmul, alpha=alpha, bias=bias, rowadd_div=rowadd_div, residual=residual, out_f32=out_f32, seed=seed)


TILE = {0: (128, 128), 1: (128, 160), 2: (256, 256), 3: (256, 320), 4: (64, 128), 5: (64, 64)}      # knob GEMM_CFG -> (rows, columns)

LINEAR_CASES = {
    # the register-staged kernel: knob GEMM_DMA = 0, and K % 64 != 0 under the default knobs
    "reg_k64": lin_case(293, 136, 64),
    "reg_k72": lin_case(293, 136, 72, alpha=0.5, wmul=2, aw=1),
    "reg_k72_f32": lin_case(293, 168, 72, out_f32=True, residual=False, alpha=2.0),
    "reg_k8_n4": lin_case(130, 4, 8, residual=False),
    # transposed V projection / ResBlock embedding add / fp32 output on the DMA kernel
    "bias_m": lin_case(293, 136, 128, bias="m", residual=False),
    "rowadd": lin_case(300, 168, 64, bias=None, rowadd_div=100, residual=True),
    "f32": lin_case(293, 136, 192, out_f32=True, alpha=2.0),
    "k1280": lin_case(293, 136, 1280, ax=1, aw=1),
}
for _cfg, (_tm, _tn) in TILE.items():          # the DMA kernel under every forced configuration
    LINEAR_CASES[f"cfg{_cfg}"] = lin_case(2 * _tm + 37, _tn + 8, 192, alpha=(1.0, 0.5, 2.0)[_cfg % 3], wmul=2 if _cfg % 3 == 1 else 1, aw=3 if _cfg % 3 == 0 else 1, seed=_cfg)
# weight-stationary kernels (N = K = 320 and the wide form): inputs in {-1, 0, 1} keep |ref| <= 320 + 16
LINEAR_CASES["ws320"] = lin_case(8192 + 37, 320, 320, ax=1, aw=1)
LINEAR_CASES["ws960"] = lin_case(8192 + 37, 960, 320, ax=1, aw=1)
# the automatic plan split into two segments: M comes from the device's CU count in the GPU test; the bounds do not depend on M
LINEAR_CASES["plan_split"] = lin_case(0, 320, 64, residual=False)


def lin_bounds(c):
    """(largest |partial sum| of the accumulator, largest |value| anywhere in the epilogue) - upper bounds from the ranges."""
    acc = c["K"] * c["ax"] * c["aw"] * c["wmul"]
    addends = (c["bias"] is not None) + (c["rowadd_div"] > 0) + bool(c["residual"])
    return acc, max(acc, abs(c["alpha"]) * acc + ADD * addends)


def lin_problem(c, M=None):
    """CPU tensors of a case and its int64 reference.  The matmul runs in fp64: every operand is an integer and every partial sum is
    below 2^24, far below 2^53, so the fp64 result IS the integer result."""
    M, N, K, s = (c["M"] if M is None else M), c["N"], c["K"], 1000 * c["seed"]
    p = dict(x=int_tensor((M, K), -c["ax"], c["ax"], s + 1), w=c["wmul"] * int_tensor((N, K), -c["aw"], c["aw"], s + 2), bias=None, rowadd=None, residual=None)
    ref = c["alpha"] * (p["x"].double() @ p["w"].double().t())
    if c["bias"] == "n":
        p["bias"] = int_tensor((N,), -ADD, ADD, s + 3).float()
        ref = ref + p["bias"].double()
    elif c["bias"] == "m":
        p["bias"] = int_tensor((M,), -ADD, ADD, s + 3).float()
        ref = ref + p["bias"].double()[:, None]
    if c["rowadd_div"]:
        p["rowadd"] = int_tensor(((M + c["rowadd_div"] - 1) // c["rowadd_div"], N), -ADD, ADD, s + 4).float()
        ref = ref + p["rowadd"].double().repeat_interleave(c["rowadd_div"], 0)[:M]
    if c["residual"]:
        p["residual"] = int_tensor((M, N), -ADD, ADD, s + 5)
        ref = ref + p["residual"].double()
    assert bool((ref == ref.round()).all())
    p["ref"] = ref.to(torch.int64)
    return p


# per-unit weights (vcx_gemm_units_f16): (units, unit_rows, N, K)
UNITS_CASES = {"3x200": (3, 200, 136, 128), "5x70": (5, 70, 72, 64), "ws_8x1024": (8, 1024, 320, 320)}


def units_problem(units, unit_rows, N, K, seed=7):
    a = 1 if K > 200 else 3
    x = int_tensor((units * unit_rows, K), -a, a, seed)
    w = int_tensor((units, N, K), -a, a, seed + 1)          # another weight set per unit
    b = int_tensor((units, N), -ADD, ADD, seed + 2).float()
    ref = torch.einsum("urk,unk->urn", x.double().view(units, unit_rows, K), w.double()) + b.double()[:, None, :]
    return x, w, b, ref.reshape(units * unit_rows, N).to(torch.int64), K * a * a + ADD


# ------------------------------------------------------------------------------------------------------------------ convolutions
def conv_case(n, H, W, cin, cout, kh=3, kw=3, stride=1, pad=None, ups=0, asym=False, slabk=None, tails=(), residual=False, ax=None, seed=0):
    taps = kh * kw
    ax = ax if ax is not None else (3 if taps * cin + sum(tails) <= 216 else 1)
    return dict(n=n, H=H, W=W, cin=cin, cout=cout, kh=kh, kw=kw, stride=stride, pad=(kh // 2, kw // 2) if pad is None else pad, ups=ups, asym=asym,
                slabk=slabk, tails=tuple(tails), residual=residual, ax=ax, aw=1 if ax == 1 else 3, seed=seed)


CONV_CASES = {
    # cin = 64 / 128: the DMA kernel (cout % 8 == 0); 8 / 72: the register-staged kernel.  17 x 19 = 323 pixels per image: ragged rows
    "c64_s1": conv_case(2, 17, 19, 64, 136),
    "c64_s1_tapmajor": conv_case(2, 17, 19, 64, 136, slabk=False),
    "c128_s1": conv_case(1, 17, 19, 128, 72),
    "c64_s2": conv_case(2, 17, 19, 64, 72, stride=2),
    "c8_s1": conv_case(2, 17, 19, 8, 136),
    "c72_s2": conv_case(2, 17, 19, 72, 40, stride=2),
    "c64_ups": conv_case(2, 9, 11, 64, 72, ups=1),
    "c8_ups": conv_case(2, 9, 11, 8, 24, ups=1),
    "c64_vae_down": conv_case(2, 16, 18, 64, 72, stride=2, pad=(0, 0), asym=True),
    "c8_vae_down": conv_case(2, 17, 19, 8, 24, stride=2, pad=(0, 0), asym=True),
    "c64_1x1": conv_case(2, 17, 19, 64, 136, kh=1, kw=1, residual=True),
    "c72_1x1": conv_case(2, 17, 19, 72, 136, kh=1, kw=1, residual=True),
    "c64_temporal": conv_case(2, 5, 67, 64, 72, kh=3, kw=1),          # (3,1,1): in_h = T, in_w = P
    "c8_temporal": conv_case(2, 5, 67, 8, 24, kh=3, kw=1),
    "c64_T1_temporal": conv_case(3, 1, 67, 64, 72, kh=3, kw=1),
    "c64_tail1": conv_case(2, 17, 19, 64, 136, tails=(64,)),
    "c64_tail2": conv_case(2, 17, 19, 64, 72, tails=(128, 64)),
    # every tap a border tap
    "c64_1x1img": conv_case(5, 1, 1, 64, 72),
    "c64_1xW": conv_case(3, 1, 21, 64, 72),
    "c64_Hx1": conv_case(3, 21, 1, 64, 72),
    "c8_1x1img": conv_case(5, 1, 1, 8, 24),
    "c8_1xW_s2": conv_case(3, 1, 21, 8, 24, stride=2),
    "c64_Hx1_ups": conv_case(3, 5, 1, 64, 72, ups=1),
}


def conv_bounds(c):
    acc = (c["kh"] * c["kw"] * c["cin"] + sum(c["tails"])) * c["ax"] * c["aw"]
    return acc, acc + ADD * (1 + bool(c["residual"]))


def conv_out_hw(c):
    He, We = c["H"] << c["ups"], c["W"] << c["ups"]
    if c["asym"]:                      # F.pad(x, (0, 1, 0, 1)) then stride 2 without padding (the VAE's Downsample)
        return (He + 1 - c["kh"]) // c["stride"] + 1, (We + 1 - c["kw"]) // c["stride"] + 1
    return (He + 2 * c["pad"][0] - c["kh"]) // c["stride"] + 1, (We + 2 * c["pad"][1] - c["kw"]) // c["stride"] + 1


def conv_problem(c):
    """x [n, H, W, cin] fp16 channels-last, w [cout, cin, kh, kw] fp16, bias fp32, tail sources / weights, residual, int64 reference
    [n, Ho, Wo, cout] from F.conv2d on int64."""
    import torch.nn.functional as F
    s = 1000 * c["seed"] + 50
    x = int_tensor((c["n"], c["H"], c["W"], c["cin"]), -c["ax"], c["ax"], s + 1)
    w = int_tensor((c["cout"], c["cin"], c["kh"], c["kw"]), -c["aw"], c["aw"], s + 2)
    b = int_tensor((c["cout"],), -ADD, ADD, s + 3).float()
    xi = x.to(torch.int64).permute(0, 3, 1, 2)
    if c["ups"]:
        xi = xi.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)          # nearest 2x
    if c["asym"]:
        xi = F.pad(xi, (0, 1, 0, 1))
    ref = F.conv2d(xi, w.to(torch.int64), b.to(torch.int64), stride=c["stride"], padding=(0, 0) if c["asym"] else c["pad"]).permute(0, 2, 3, 1).contiguous()
    Ho, Wo = conv_out_hw(c)
    assert tuple(ref.shape) == (c["n"], Ho, Wo, c["cout"])
    M = c["n"] * Ho * Wo
    srcs, wts = [], []
    for j, k in enumerate(c["tails"]):
        srcs.append(int_tensor((M, k), -c["ax"], c["ax"], s + 10 + j))
        wts.append(int_tensor((c["cout"], k), -c["aw"], c["aw"], s + 20 + j))
        ref = ref + (srcs[-1].double() @ wts[-1].double().t()).to(torch.int64).view(ref.shape)
    res = None
    if c["residual"]:
        res = int_tensor((M, c["cout"]), -ADD, ADD, s + 30)
        ref = ref + res.to(torch.int64).view(ref.shape)
    return dict(x=x, w=w, bias=b, tail_src=srcs, tail_w=wts, residual=res, ref=ref, out_hw=(Ho, Wo))


# ------------------------------------------------------------------------------------------------------------------ attention
def v_codes(nk, d=64):
    """V[j, c] = ((7 j + 3 c) mod 61) - 30: every entry differs from its neighbours in j and in c by at least 1 (7 and 3 are units mod 61
    and neither +-7 nor +-3 is 0 mod 61), so a key, head, group or V^T-column mix-up changes the expected value by >= 1."""
    j = torch.arange(nk)[:, None]
    c = torch.arange(d)[None, :]
    return (((7 * j + 3 * c) % 61) - 30).to(torch.float16)


ONE_HOT_BETA = 16.0
ONE_HOT_GAP_NATS = 30.0


def one_hot_problem(n_kv_groups, heads, nk, nq, d=64, seed=0, beta=ONE_HOT_BETA):
    """Keys: random +-1 vectors, K [n_kv_groups, nk, heads, d].  perm [n_kv_groups, heads, nq]: the key each query selects - a random
    draw over all keys, so consecutive queries jump across key tiles; heads and groups get their own keys and draws.
    Q = beta * K[perm].  V [n_kv_groups, nk, heads, d] = v_codes shifted per (group, head) so that those differ too."""
    g = torch.Generator().manual_seed(seed)
    k = (torch.randint(0, 2, (n_kv_groups, nk, heads, d), generator=g) * 2 - 1).to(torch.float16)
    perm = torch.stack([torch.stack([torch.randperm(max(nk, nq), generator=g)[:nq] % nk for _ in range(heads)]) for _ in range(n_kv_groups)])
    q = torch.empty((n_kv_groups, nq, heads, d), dtype=torch.float16)
    v = torch.empty((n_kv_groups, nk, heads, d), dtype=torch.float16)
    for gi in range(n_kv_groups):
        for h in range(heads):
            q[gi, :, h] = beta * k[gi, perm[gi, h], h]
            v[gi, :, h] = v_codes(nk + 64, d)[(5 * gi + 11 * h) % 61:][:nk]
    return q, k, v, perm


def one_hot_gap(q, k, perm, scale):
    """min over queries of (winning logit - best other logit), in nats, from the inputs (fp64)."""
    gap = float("inf")
    G, nq, heads, d = q.shape
    for gi in range(G):
        for h in range(heads):
            s = scale * (q[gi, :, h].double() @ k[gi, :, h].double().t())          # [nq, nk]
            win = s.gather(1, perm[gi, h][:, None]).squeeze(1)
            # keys identical to the winner give the same logit: they must then carry the same V row, which v_codes does not - so none may exist
            other = s.clone()
            other.scatter_(1, perm[gi, h][:, None], float("-inf"))
            gap = min(gap, float((win - other.max(1).values).min()) if s.shape[1] > 1 else float("inf"))
    return gap


FLASH_UNIFORM_NK = (1, 33, 77, 135, 4097)
TEMPORAL_UNIFORM_T = (1, 25, 33, 57, 64)
PAD_FINITE = 1000.0


def uniform_values(nk, d, seed=0):
    """Integers in [-30, 30] [nk, d] and the fp64 mean over the keys."""
    v = int_tensor((nk, d), -30, 30, 900 + seed + nk)
    return v, v.double().mean(0)
