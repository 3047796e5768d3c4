"""Operand and output LAYOUTS for the attention entry points, and the four assertions every (kernel, layout) case makes
(tests/test_attn_layouts_gpu.py on the kernels, tests/test_attn_layouts_cpu.py on plain-torch stand-ins: no GPU is needed to import this).

Every attention entry takes its operands and its output by base pointer and row pitch.  A logical [rows, cols] matrix is placed at column
`col` of a [guard_rows + rows + guard_rows, pitch] buffer - `embed` - and the kernel gets the window's data_ptr() and `pitch`.  Operand
buffers are filled with NaN: a value used from outside the declared window ruins the output.  Output buffers are filled with the sentinel
GUARD of tests/test_exact_gpu.py: everything outside the window must come back bit-identical.

The assertions of a case (`flash_case`, `temporal_case`, `softmax_case` return them as closures a, b, c, d, so that the CPU test can tell
WHICH one rejects a wrong stand-in):
  a. an independent reference on the strided call itself: one-hot softmaxes (tests/exact_inputs.py), O_i = V[pi(i)] within 2^-10 |v| (the
     bound derived in tests/test_exact_gpu.py); where no one-hot construction exists (accumulate, relative position, the row softmax) the
     fp64 softmax reference within tests/test_fuzz_gpu.py's rel-L2 <= 3e-3, which the fp16-rounded reference alone must meet;
  b. bit identity with the dense call on the same N(0, 1) data: a pitch or a base pointer enters no arithmetic, so no tolerance;
  c. only the output window is written: guard rows in front and behind, the columns left and right of it, the pitch gap;
  d. no operand buffer is written, and the output is finite although everything around the operands is NaN.
"""
import math

import torch

from tests import exact_inputs as X
from tests.test_exact_gpu import GUARD

NAN = float("nan")
GUARD_ROWS = 2          # even: with o at column 4 of pitch C + 4 the FIRST window row is then the one that is only 8-byte aligned
REL_L2 = 3e-3           # tests/test_fuzz_gpu.py: kernel against the fp64 softmax reference
LN2 = math.log(2.0)

# name -> operand -> (column of the window, pitch - window width).  C is the logical width (64 heads, or 512); every pointer obeys the front
# end's alignment rule (csrc/attention.hip flash_refusal / dual_refusal / tattn_launch / vcx_softmax_rows_f16) and nothing more.
#   dense          the control: what the rest of the suite passes
#   wide           q at column 8 of pitch C + 24, k at column 16 of pitch C + 40, V^T at column 8 of pitch groups kv_rows + 24, o at column 16
#                  of pitch C + 72: everything 16-byte aligned, every pitch a multiple of 8, all different (k1 / k2, vt1 / vt2 of the dual entry
#                  take the k / vt rule each)
#   o8             as wide, but o at column 4 of pitch C + 4: o is only 8-byte aligned, ldo % 8 == 4 and successive rows alternate between
#                  8- and 16-byte alignment (flash d64, dual, d512 only: the temporal entries require ldo % 8 == 0)
#   temporal_wide  qkv pointer at column 16 of pitch 3 C + 40 (the window is 3 C + 24 wide), v_off = C + 8, k_off = 2 C + 24 - v in front of k,
#                  gaps between the three - and o at column 8 of pitch C + 24
#   softmax_rows   x at column 8 of pitch n8 + 24, in place
LAYOUTS = {
    "dense": dict(q=(0, 0), k=(0, 0), vt=(0, 0), o=(0, 0)),
    "wide": dict(q=(8, 24), k=(16, 40), vt=(8, 24), o=(16, 72)),
    "o8": dict(q=(8, 24), k=(16, 40), vt=(8, 24), o=(4, 4)),
    "temporal_dense": dict(qkv=(0, 0), o=(0, 0), k_off=lambda C: C, v_off=lambda C: 2 * C, width=lambda C: 3 * C),
    "temporal_wide": dict(qkv=(16, 16), o=(8, 24), k_off=lambda C: 2 * C + 24, v_off=lambda C: C + 8, width=lambda C: 3 * C + 24),
    "softmax_dense": dict(x=(0, 0)),
    "softmax_rows": dict(x=(8, 24)),
}


def embed(mat, *, pitch, col, guard_rows, fill):
    """The logical [rows, cols] matrix at column `col` of a [guard_rows + rows + guard_rows, pitch] buffer of `fill` (same device and type).
    -> (buffer, window view): the view's data_ptr() is what a launcher gets, `pitch` its ld* argument."""
    rows, cols = mat.shape
    assert 0 <= col and col + cols <= pitch, (col, cols, pitch)
    buf = torch.full((guard_rows + rows + guard_rows, pitch), fill, dtype=mat.dtype, device=mat.device)
    view = buf[guard_rows:guard_rows + rows, col:col + cols]
    view.copy_(mat)
    return buf, view


def _bits(t):
    return (t.view(torch.int16) if t.dtype == torch.float16 else t).cpu()


def assert_only_window_written(buf_before, buf_after, rows, col, cols, name="output"):
    """Everything outside the [rows, cols] window at column `col` (guard rows in front and behind, the columns left and right, the pitch
    gap) is bit-identical; compared as int16, so that a NaN equals itself."""
    a, b = _bits(buf_before).clone(), _bits(buf_after).clone()
    assert a.shape == b.shape
    g = (a.shape[0] - rows) // 2
    assert a.shape[0] == rows + 2 * g and col + cols <= a.shape[1]
    a[g:g + rows, col:col + cols] = 0
    b[g:g + rows, col:col + cols] = 0
    if torch.equal(a, b):
        return
    r, c = torch.nonzero(a != b)[0].tolist()
    where = "a guard row in front" if r < g else "a guard row behind" if r >= g + rows else "left of the window" if c < col else "right of the window / the pitch gap"
    raise AssertionError(f"{name}: {int((a != b).sum())} elements outside the window [{rows}, {cols}] at column {col} of pitch {a.shape[1]} were written; first at "
                         f"buffer row {r} (window row {r - g}), column {c}: {where}")


def assert_operands_untouched(before, after):
    """before: name -> clone of an operand buffer made in front of the call, after: name -> the buffer.  No kernel may write an operand."""
    for name in before:
        assert torch.equal(_bits(before[name]), _bits(after[name])), f"operand {name} was written"


class Placed:
    """The operands (name -> logical fp16 matrix) and the output (`out`: its window's content in front of the call) of one call, placed by
    LAYOUTS[layout]: .view[name] / .ld[name], .o / .ldo are what the launcher gets."""

    def __init__(self, layout, operands, out, device, out_name="o", out_fill=GUARD):
        lay = LAYOUTS[layout]
        self.layout, self.buf, self.view, self.ld = layout, {}, {}, {}
        for name, mat in operands.items():
            col, extra = lay[name.rstrip("12")]
            self.ld[name] = mat.shape[1] + extra
            self.buf[name], self.view[name] = embed(mat.to(device), pitch=self.ld[name], col=col, guard_rows=GUARD_ROWS, fill=NAN)
        self.o_col, extra = lay[out_name]
        self.ldo = out.shape[1] + extra
        self.obuf, self.o = embed(out.to(device), pitch=self.ldo, col=self.o_col, guard_rows=GUARD_ROWS, fill=out_fill)
        self.before = {n: b.clone() for n, b in self.buf.items()}
        self.obuf_before = self.obuf.clone()

    def residues(self):
        """name -> (data_ptr() mod 16 of the window, its pitch); the buffers themselves start 16-byte aligned (asserted)."""
        out = {}
        for name in list(self.buf) + ["o"]:
            buf, view, ld = (self.obuf, self.o, self.ldo) if name == "o" else (self.buf[name], self.view[name], self.ld[name])
            assert buf.data_ptr() % 16 == 0
            out[name] = (view.data_ptr() % 16, ld)
        return out

    def check_c(self):
        assert_only_window_written(self.obuf_before, self.obuf, self.o.shape[0], self.o_col, self.o.shape[1], f"layout {self.layout}")

    def check_d(self):
        assert_operands_untouched(self.before, self.buf)
        assert bool(torch.isfinite(self.o.float()).all()), f"layout {self.layout}: the output is not finite - a value from outside an operand's window was used"


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def assert_close_to_fp64(out, ref64, name):
    """a. where no one-hot construction exists: the fp16-rounded fp64 reference alone is inside the bound, and so is the kernel."""
    assert rel_l2(ref64.half(), ref64) <= REL_L2, f"{name}: the bound does not admit the rounded reference itself"
    e = rel_l2(out, ref64)
    assert e <= REL_L2, f"{name}: rel-L2 {e:.3e} against the fp64 reference (bound {REL_L2})"


def assert_same_bits(got, want, name):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape
    if not torch.equal(got, want):
        bad = got != want
        raise AssertionError(f"{name}: differs from the dense call - {X._where(bad)}")


def run_checks(checks):
    for key in "abcd":
        checks[key]()


# ------------------------------------------------------------------------------------------------------------------ flash (d64 / d512)
def kv_layout_cpu(k, v, kv_rows, pad_k, pad_v, pad_v8=None):
    """tests/test_exact_gpu.py kv_layout without the copy to the device (the CPU stand-ins)."""
    Gk, nk, C = k.shape
    nk8 = (nk + 7) // 8 * 8
    kp = torch.full((Gk, kv_rows, C), pad_k, dtype=torch.float16)
    vp = torch.full((Gk, kv_rows, C), pad_v, dtype=torch.float16)
    vp[:, nk:nk8] = pad_v if pad_v8 is None else pad_v8
    kp[:, :nk] = k
    vp[:, :nk] = v
    return kp.view(Gk * kv_rows, C), vp.view(Gk * kv_rows, C).t().contiguous()


def softmax_ref64(q, k, v, logit_scale, mask=None, bias=None):
    """[..., nq, d] x [..., nk, d] x [..., nk, d] in fp64 -> (softmax(logit_scale (q k^T + bias)) v, the probabilities)"""
    s = q.double() @ k.double().transpose(-1, -2)
    if bias is not None:
        s = s + bias
    s = s * logit_scale
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, -1)
    return p @ v.double(), p


def flash_one_hot(Gk, kv_div, heads, nq, nk, d=64, seed=0):
    """The one-hot problem of tests/test_exact_gpu.py::test_flash_attention_one_hot_selects_the_right_value_row (gap asserted from the inputs)
    -> q [G nq, C], k, v [Gk, nk, C] (fp16), want [G nq, C] (fp64): O_i = V[pi(i)]."""
    G, C = Gk * kv_div, heads * d
    q, k, v, perm = X.one_hot_problem(Gk, heads, nk, kv_div * nq, d=d, seed=nk + seed)
    assert X.one_hot_gap(q[:, :256], k, perm[:, :, :256], d ** -0.5) >= X.ONE_HOT_GAP_NATS
    want = torch.stack([torch.stack([v[gk, perm[gk, h], h] for h in range(heads)], dim=1) for gk in range(Gk)]).double().reshape(G * nq, C)
    return q.reshape(G * nq, C), k.reshape(Gk, nk, C), v.reshape(Gk, nk, C), want


def flash_case(launch, layout, *, device, heads, Gk, kv_div, nq, nk, d=64, log2=False, accumulate=False, kv_layout=kv_layout_cpu, seed=0):
    """launch(views, ld, o, ldo, geo): one call of vcx_attn_flash_d64_f16 / _d512_f16 (or a stand-in) on the placed operands.  Runs the one-hot
    problem in `layout` and N(0, 1) data in `layout` and densely; -> the assertions a - d as closures."""
    G, C, scale = Gk * kv_div, heads * d, d ** -0.5
    kv_rows = (nk + 7) // 8 * 8 + 16
    geo = dict(n_groups=G, heads=heads, nq=nq, nk=nk, kv_rows=kv_rows, kv_div=kv_div, scale=scale, log2=log2, accumulate=accumulate, d=d)
    prep_q = (lambda t: (t.float() * (scale * 1.4426950408889634)).half()) if log2 else (lambda t: t)

    def place(lay, q, k, v, o0):
        # K rows >= nk and V^T columns >= nk8 are never used (NaN); V^T columns [nk, nk8) stay finite as include/vcx.h demands
        kd, vtd = kv_layout(k, v, kv_rows, NAN, NAN, X.PAD_FINITE)
        p = Placed(lay, dict(q=q, k=kd, vt=vtd), o0, device)
        launch(p.view, p.ld, p.o, p.ldo, geo)
        return p

    fresh = torch.full((G * nq, C), GUARD, dtype=torch.float16)
    hot = None
    if not accumulate:
        q, k, v, want = flash_one_hot(Gk, kv_div, heads, nq, nk, d, seed)
        hot = place(layout, prep_q(q), k, v, fresh)
    g = torch.Generator().manual_seed(1000 + nk + nq + seed)
    qr = prep_q(torch.randn((G * nq, C), generator=g).half())
    kr, vr = torch.randn((Gk, nk, C), generator=g).half(), torch.randn((Gk, nk, C), generator=g).half()
    o0 = torch.randn((G * nq, C), generator=g).half() if accumulate else fresh
    dense, strided = place("dense", qr, kr, vr, o0), place(layout, qr, kr, vr, o0)

    def a():
        if hot is not None:
            X.assert_elementwise(hot.o, want, want.abs() * 2.0 ** -10, f"flash one-hot, layout {layout}")
            return
        split = lambda t, n: t.double().view(Gk, n, heads, d).permute(0, 2, 1, 3)
        ref, _ = softmax_ref64(split(qr, kv_div * nq), split(kr, nk), split(vr, nk), LN2 if log2 else scale)
        ref = ref.permute(0, 2, 1, 3).reshape(G * nq, C) + o0.double()
        assert_close_to_fp64(strided.o, ref, f"flash accumulate, layout {layout}")

    def b():
        assert_same_bits(strided.o, dense.o, f"flash, layout {layout}")

    def c():
        for p in (hot, dense, strided):
            if p is not None:
                p.check_c()

    def d_():
        for p in (hot, dense, strided):
            if p is not None:
                p.check_d()

    return dict(a=a, b=b, c=c, d=d_, dense=dense, strided=strided)


# ------------------------------------------------------------------------------------------------------------------ temporal
def temporal_one_hot(B, T, P, heads, causal, g):
    """The one-hot problem of tests/test_exact_gpu.py::test_temporal_attention_uniform_means_and_one_hot (gap asserted from the inputs)
    -> q, k, codes [B, T, P, heads, 64] (fp16), want [(b t p), C] (fp64): O_t = codes[pi(t)], pi(t) <= t under the causal mask."""
    k = (torch.randint(0, 2, (B, T, P, heads, 64), generator=g) * 2 - 1).to(torch.float16)
    pi = torch.stack([torch.randint(0, t + 1 if causal else T, (B, P, heads), generator=g) for t in range(T)], dim=1)      # [B, T, P, heads]
    idx = pi[..., None].expand(B, T, P, heads, 64)
    q = X.ONE_HOT_BETA * k.gather(1, idx)
    codes = ((7 * torch.arange(T).view(1, T, 1, 1, 1) + 3 * torch.arange(64).view(1, 1, 1, 1, 64) + 11 * torch.arange(P).view(1, 1, P, 1, 1)
              + 5 * torch.arange(heads).view(1, 1, 1, heads, 1) + 13 * torch.arange(B).view(B, 1, 1, 1, 1)) % 61 - 30).to(torch.float16)
    s = 0.125 * torch.einsum("btphd,bsphd->bphts", q.double(), k.double())
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))
    win = s.gather(-1, pi.permute(0, 2, 3, 1)[..., None])
    other = s.scatter(-1, pi.permute(0, 2, 3, 1)[..., None], float("-inf")).max(-1, keepdim=True).values
    assert float((win - other).min()) >= X.ONE_HOT_GAP_NATS
    return q, k, codes, codes.gather(1, idx).double().reshape(B * T * P, heads * 64)
def temporal_window(q, k, v, layout):
    """[B, T, P, heads, 64] each -> the logical qkv window of LAYOUTS[layout]: [(b t p), width(C)] with q at column 0, k at k_off, v at v_off
    and NaN in the gaps."""
    B, T, P, heads, _ = q.shape
    C, lay = heads * 64, LAYOUTS[layout]
    win = torch.full((B * T * P, lay["width"](C)), NAN, dtype=torch.float16)
    for t, off in ((q, 0), (k, lay["k_off"](C)), (v, lay["v_off"](C))):
        assert bool(torch.isnan(win[:, off:off + C]).all()), "q, k and v overlap"
        win[:, off:off + C] = t.reshape(B * T * P, C)
    return win


def temporal_case(launch, layout, *, device, T, causal, R=0, B=2, P=9, heads=2):
    """launch(qkv, ld, k_off, v_off, o, ldo, geo, relg, relp): one call of vcx_attn_temporal_d64[_masked | _rel]_f16 (or a stand-in).  R > 0: the
    relative-position form on N(0, 1) data against the fp64 reference (relp as well); else the one-hot problem of
    tests/test_exact_gpu.py::test_temporal_attention_uniform_means_and_one_hot.  -> the assertions a - d."""
    C, rows = heads * 64, B * T * P
    geo = dict(B=B, T=T, P=P, heads=heads, scale=0.125, causal=causal, R=R)
    g = torch.Generator().manual_seed(T + 100 * R)
    fresh = torch.full((rows, C), GUARD, dtype=torch.float16)
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool)) if causal else None

    def place(lay, q, k, v, relg=None):
        p = Placed(lay, dict(qkv=temporal_window(q, k, v, lay)), fresh, device)
        p.relg = None if relg is None else relg.to(device)
        p.relp = None if relg is None else torch.zeros((rows, heads, 64), dtype=torch.float16, device=device)
        launch(p.view["qkv"], p.ld["qkv"], LAYOUTS[lay]["k_off"](C), LAYOUTS[lay]["v_off"](C), p.o, p.ldo, geo, p.relg, p.relp)
        return p

    hot = None
    if not R:
        q, k, codes, want = temporal_one_hot(B, T, P, heads, causal, g)
        hot = place(layout, q, k, codes)
    qr, kr, vr = (torch.randn((B, T, P, heads, 64), generator=g).half() for _ in range(3))
    relg = torch.randn((rows, heads, 64), generator=g).half() if R else None
    dense, strided = place("temporal_dense", qr, kr, vr, relg), place(layout, qr, kr, vr, relg)

    def a():
        if hot is not None:
            X.assert_elementwise(hot.o, want, want.abs() * 2.0 ** -10, f"temporal one-hot T {T} causal {causal}, layout {layout}")
            return
        per = lambda t: t.double().permute(0, 2, 3, 1, 4)                                     # [B, P, heads, T, 64]
        dist = (torch.arange(T)[None, :] - torch.arange(T)[:, None]).clamp(-R, R) + R         # [query t, key s] -> slot
        rg = relg.double().view(B, T, P, heads, 64).permute(0, 2, 3, 1, 4)                    # [B, P, heads, T, slot]
        bias = rg.gather(-1, dist.expand(B, P, heads, T, T))
        ref, p = softmax_ref64(per(qr), per(kr), per(vr), 0.125, mask=mask, bias=bias)
        assert_close_to_fp64(strided.o, ref.permute(0, 3, 1, 2, 4).reshape(rows, C), f"temporal rel T {T} causal {causal}, layout {layout}")
        slots = torch.zeros((B, P, heads, T, 64), dtype=torch.float64).scatter_add_(-1, dist.expand(B, P, heads, T, T).contiguous(), p)
        assert_close_to_fp64(strided.relp.reshape(rows, heads * 64), slots.permute(0, 3, 1, 2, 4).reshape(rows, heads * 64), f"relp T {T} causal {causal}, layout {layout}")

    def b():
        assert_same_bits(strided.o, dense.o, f"temporal T {T} causal {causal}, layout {layout}")
        if R:
            assert_same_bits(strided.relp.reshape(rows, -1), dense.relp.reshape(rows, -1), f"relp T {T} causal {causal}, layout {layout}")

    def c():
        for p in (hot, dense, strided):
            if p is not None:
                p.check_c()

    def d_():
        for p in (hot, dense, strided):
            if p is not None:
                p.check_d()
                if R:
                    assert torch.equal(_bits(p.relg), _bits(relg)), "relg was written"

    return dict(a=a, b=b, c=c, d=d_)


# ------------------------------------------------------------------------------------------------------------------ row softmax
def softmax_case(launch, layout, *, device, rows, n):
    """launch(x, rows, n, ld): vcx_softmax_rows_f16 in place (or a stand-in) on N(0, 2^2) logits.  The window is n8 = n rounded up to 8 wide: its
    columns [n, n8) hold 3.0 and become 0; everything around it is NaN and stays.  -> the assertions a - d."""
    n8 = (n + 7) // 8 * 8
    g = torch.Generator().manual_seed(n)
    x = torch.full((rows, n8), 3.0, dtype=torch.float16)
    x[:, :n] = (2.0 * torch.randn((rows, n), generator=g)).half()

    def place(lay):
        p = Placed(lay, {}, x, device, out_name="x", out_fill=NAN)
        launch(p.o, rows, n, p.ldo)
        return p

    dense, strided = place("softmax_dense"), place(layout)

    def a():
        ref = torch.zeros((rows, n8), dtype=torch.float64)
        ref[:, :n] = torch.softmax(x[:, :n].double(), -1)
        assert_close_to_fp64(strided.o, ref, f"softmax rows n {n}, layout {layout}")
        assert bool((strided.o[:, n:] == 0).all()), "the columns [n, n8) must become 0"

    def b():
        assert_same_bits(strided.o, dense.o, f"softmax rows n {n}, layout {layout}")

    def c():
        dense.check_c()
        strided.check_c()

    def d_():
        dense.check_d()
        strided.check_d()

    return dict(a=a, b=b, c=c, d=d_)
