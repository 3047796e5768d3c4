"""The layout checker of tests/attn_layouts.py on plain-torch stand-ins, the LAYOUTS table against the front end's rules, and the
refusals of the fp16 attention front end (csrc/attention.hip) - all without a GPU.

1. Stand-ins of flash_attn, temporal_attn and softmax_rows_ that read and write through as_strided windows of the whole allocation - what a
   C callee sees: a base pointer and a pitch - pass the assertions a - d of every layout; five deliberately wrong ones are each rejected
   by the assertion meant for them.  So tests/test_attn_layouts_gpu.py would notice those bugs in a kernel.
2. Every LAYOUTS entry obeys the % 8 / % 4 / 16-byte / 8-byte rules and only just.
3. vcx_attn_flash_d64_f16, _dual_d64_f16, _d512_f16, the temporal entries and vcx_softmax_rows_f16 refuse what include/vcx.h says they
   refuse, with -1 and a telling vcx_last_error(), before any launch (FAKE pointers: an accepted call would launch).
"""
import pytest
import torch

from tests import attn_layouts as A

CPU = "cpu"


# ================================================================================================================ stand-ins
def _flat(view):
    """(the whole allocation as a 1-D tensor, the view's element offset in it): the callee's pointer"""
    n = view.untyped_storage().nbytes() // view.element_size()
    return torch.as_strided(view, (n,), (1,), 0), view.storage_offset()


def _win(view, rows, cols, ld, shift=0):
    flat, off = _flat(view)
    return torch.as_strided(flat, (rows, cols), (ld, 1), off + shift)


def _store(o, ldo, res, cols, bug):
    """The store tail of every stand-in: res [rows, cols] to o + row * ldo.  The three wrong store tails:
    pitch_c ignores ldo, no_col drops the window's column offset (it stores from the start of the buffer row), row_past writes one row more."""
    rows = res.shape[0]
    flat, off = _flat(o)
    if bug == "pitch_c":
        ldo = cols
    if bug == "no_col":
        off -= off % ldo
    if bug == "row_past":
        res = torch.cat([res, res[-1:]])
        rows += 1
    torch.as_strided(flat, (rows, cols), (ldo, 1), off).copy_(res)


def flash_standin(bug=None):
    def launch(view, ld, o, ldo, geo):
        G, heads, nq, nk, d = geo["n_groups"], geo["heads"], geo["nq"], geo["nk"], geo["d"]
        C, Gk = heads * d, geo["n_groups"] // geo["kv_div"]
        over = 8 if bug == "q_overread" else 0                       # one 8-element chunk past a Q row's width, against zero key columns
        q = _win(view["q"], G * nq, C + over, ld["q"]).double()
        k = _win(view["k"], Gk * geo["kv_rows"], C, ld["k"]).double().view(Gk, geo["kv_rows"], heads, d)[:, :nk]
        v = _win(view["vt"], C, Gk * geo["kv_rows"], ld["vt"]).double().view(heads, d, Gk, geo["kv_rows"])[..., :nk].permute(2, 3, 0, 1)      # [Gk, nk, heads, d]
        qs = q[:, :C].view(Gk, geo["kv_div"] * nq, heads, d).permute(0, 2, 1, 3)
        bias = (q[:, C:] * 0.0).sum(1).view(Gk, 1, geo["kv_div"] * nq, 1) if over else None
        res, _ = A.softmax_ref64(qs, k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), A.LN2 if geo["log2"] else geo["scale"], bias=bias)
        res = res.permute(0, 2, 1, 3).reshape(G * nq, C)
        if geo["accumulate"]:
            res = res + _win(o, G * nq, C, ldo).double()
        _store(o, ldo, res.half(), C, bug)
    return launch


def temporal_standin(bug=None):
    def launch(qkv, ld, k_off, v_off, o, ldo, geo, relg, relp):
        B, T, P, heads = geo["B"], geo["T"], geo["P"], geo["heads"]
        C, rows = heads * 64, B * T * P
        if bug == "no_k_off":
            k_off = 0
        part = lambda off: _win(qkv, rows, C, ld, off).double().view(B, T, P, heads, 64).permute(0, 2, 3, 1, 4)
        mask = torch.tril(torch.ones(T, T, dtype=torch.bool)) if geo["causal"] else None
        res, _ = A.softmax_ref64(part(0), part(k_off), part(v_off), geo["scale"], mask=mask)
        _store(o, ldo, res.permute(0, 3, 1, 2, 4).reshape(rows, C).half(), C, bug)
    return launch


def softmax_standin(x, rows, n, ld):
    n8 = (n + 7) // 8 * 8
    res = torch.zeros((rows, n8), dtype=torch.float64)
    res[:, :n] = torch.softmax(_win(x, rows, n, ld).double(), -1)
    _store(x, ld, res.half(), n8, None)


FLASH_SHAPES = dict(qb1=dict(heads=2, Gk=2, kv_div=2, nq=100, nk=135), log2=dict(heads=2, Gk=2, kv_div=2, nq=100, nk=77, log2=True),
                    accumulate=dict(heads=2, Gk=2, kv_div=2, nq=100, nk=135, accumulate=True), d512=dict(heads=1, Gk=2, kv_div=1, nq=40, nk=35, d=512))


@pytest.mark.parametrize("layout", ["wide", "o8"])
@pytest.mark.parametrize("shape", sorted(FLASH_SHAPES))
def test_a_correct_flash_stand_in_passes_every_assertion(shape, layout):
    A.run_checks(A.flash_case(flash_standin(), layout, device=CPU, **FLASH_SHAPES[shape]))


@pytest.mark.parametrize("T,causal", [(25, False), (25, True), (33, True)])
def test_a_correct_temporal_stand_in_passes_every_assertion(T, causal):
    A.run_checks(A.temporal_case(temporal_standin(), "temporal_wide", device=CPU, T=T, causal=causal, B=2, P=3))


@pytest.mark.parametrize("n", [135, 512])
def test_a_correct_softmax_stand_in_passes_every_assertion(n):
    A.run_checks(A.softmax_case(softmax_standin, "softmax_rows", device=CPU, rows=37, n=n))


def _rejecting(checks):
    out = []
    for key in "abcd":
        try:
            checks[key]()
        except AssertionError:
            out.append(key)
    return out


# (the bug, the family, the assertion MEANT to catch it): c = only the window is written, a = the one-hot reference, d = a NaN arrived
WRONG = [("pitch_c", "flash", "c"), ("no_col", "flash", "c"), ("row_past", "flash", "c"), ("q_overread", "flash", "d"), ("no_k_off", "temporal", "a"),
         ("pitch_c", "temporal", "c"), ("row_past", "temporal", "c")]


@pytest.mark.parametrize("bug,family,meant", WRONG, ids=[f"{b}-{f}" for b, f, _ in WRONG])
def test_each_wrong_stand_in_is_rejected_by_the_assertion_meant_for_it(bug, family, meant):
    """pitch_c: stores with pitch C, ignoring ldo.  no_col: ignores the output's column offset.  row_past: writes one row past the window.
    q_overread: reads one 8-element chunk past a Q row's width (multiplied by zero key columns: harmless densely, NaN in a window).
    no_k_off: ignores k_off (k = q: a finite, in-window, wrong result)."""
    if family == "flash":
        checks = A.flash_case(flash_standin(bug), "wide", device=CPU, **FLASH_SHAPES["qb1"])
    else:
        checks = A.temporal_case(temporal_standin(bug), "temporal_wide", device=CPU, T=25, causal=False, B=2, P=3)
    rejected = _rejecting(checks)
    print(f"{bug} ({family}): rejected by {rejected}, meant for {meant}")
    assert meant in rejected, f"{bug}: assertion {meant} let it pass (rejected by: {rejected})"
    if bug in ("pitch_c", "no_col", "row_past"):
        with pytest.raises(AssertionError, match="outside the window"):
            checks["c"]()
    if bug == "q_overread":
        with pytest.raises(AssertionError, match="not finite"):
            checks["d"]()
        assert "c" not in rejected, "it writes nothing outside the window"
    if bug == "no_k_off":
        assert rejected == ["a"], "finite, inside the window, the same densely (b compares two calls of the same code): only the reference can tell"


def test_the_window_checker_names_where_the_stray_write_went():
    mat = torch.zeros((5, 16), dtype=torch.float16)
    buf, view = A.embed(mat, pitch=40, col=8, guard_rows=2, fill=A.GUARD)
    assert view.data_ptr() == buf.data_ptr() + 2 * (2 * 40 + 8) and bool((buf[:2] == A.GUARD).all()) and bool((buf[2:7, 24:] == A.GUARD).all())
    before = buf.clone()
    view.fill_(1.0)
    A.assert_only_window_written(before, buf, 5, 8, 16)
    for (r, c), word in (((1, 8), "in front"), ((7, 8), "behind"), ((3, 7), "left"), ((3, 24), "right")):
        bad = buf.clone()
        bad[r, c] = 1.0
        with pytest.raises(AssertionError, match=word):
            A.assert_only_window_written(before, bad, 5, 8, 16)
    nan = torch.full((3, 8), A.NAN, dtype=torch.float16)
    A.assert_operands_untouched(dict(x=nan.clone()), dict(x=nan))                # a NaN equals itself: compared as int16
    with pytest.raises(AssertionError, match="operand x"):
        A.assert_operands_untouched(dict(x=nan.clone()), dict(x=torch.zeros_like(nan)))


# ================================================================================================================ the table obeys the front end, only just
@pytest.mark.parametrize("C,kvr", [(128, 2 * 152), (512, 2 * 152), (64, 2064)])
def test_every_layout_obeys_the_front_end_and_only_just(C, kvr):
    """flash / dual / d512 (flash_refusal, dual_refusal, vcx_attn_flash_d512_f16): ldq, ldk, ldvt % 8 == 0, ldo % 4 == 0, q / k / vt 16-byte
    aligned, o 8-byte aligned.  Temporal (tattn_launch): ld, ldo % 8 == 0, qkv and o 16-byte aligned, k_off / v_off non-negative multiples
    of 8.  vcx_softmax_rows_f16: ld % 8 == 0, ld >= n8, x 16-byte aligned."""
    z = lambda r, c: torch.zeros((r, c), dtype=torch.float16)
    for name in ("dense", "wide", "o8"):
        res = A.Placed(name, dict(q=z(5, C), k=z(7, C), vt=z(C, kvr)), z(5, C), CPU).residues()
        for op in ("q", "k", "vt"):
            assert res[op][0] == 0 and res[op][1] % 8 == 0, (name, op, res[op])
        assert res["o"][0] % 8 == 0 and res["o"][1] % 4 == 0, (name, res["o"])
    wide = A.Placed("wide", dict(q=z(5, C), k=z(7, C), vt=z(C, kvr)), z(5, C), CPU).residues()
    assert wide == dict(q=(0, C + 24), k=(0, C + 40), vt=(0, kvr + 24), o=(0, C + 72)) and len({ld for _, ld in wide.values()}) == 4
    o8 = A.Placed("o8", dict(q=z(5, C), k=z(7, C), vt=z(C, kvr)), z(5, C), CPU)
    assert o8.residues()["o"] == (8, C + 4) and o8.ldo % 8 == 4 and o8.o.data_ptr() % 16 == 8          # the second-form resident kernel's rule fails
    assert o8.o[1].data_ptr() % 16 == 0 and o8.o[2].data_ptr() % 16 == 8                               # rows alternate
    for name in ("temporal_dense", "temporal_wide"):
        lay = A.LAYOUTS[name]
        k_off, v_off, W = lay["k_off"](C), lay["v_off"](C), lay["width"](C)
        res = A.Placed(name, dict(qkv=z(6, W)), z(6, C), CPU).residues()
        assert res["qkv"][0] == 0 and res["o"][0] == 0 and res["qkv"][1] % 8 == 0 and res["o"][1] % 8 == 0
        assert k_off >= 0 and v_off >= 0 and k_off % 8 == 0 and v_off % 8 == 0 and max(k_off, v_off) + C <= W
    lay = A.LAYOUTS["temporal_wide"]
    assert A.Placed("temporal_wide", dict(qkv=z(6, lay["width"](C))), z(6, C), CPU).residues() == dict(qkv=(0, 3 * C + 40), o=(0, C + 24))
    assert C < lay["v_off"](C) and lay["v_off"](C) + C < lay["k_off"](C)                                # gaps, and v in front of k
    for n8 in (136, 512):
        assert A.Placed("softmax_rows", {}, z(3, n8), CPU, out_name="x").residues()["o"] == (0, n8 + 24)


# ================================================================================================================ refusals
FAKE = 1 << 20
ACC, LOG2, CAUSAL = 1, 2, 4


def _args(spec, **kw):
    unknown = set(kw) - {k for k, _ in spec}
    assert not unknown, unknown
    return [kw.get(k, d) for k, d in spec]


FLASH = (("q", FAKE), ("k", FAKE), ("vt", FAKE), ("o", FAKE), ("n_groups", 2), ("heads", 1), ("nq", 64), ("nk", 60), ("kv_rows", 64), ("kv_div", 1), ("ldq", 64),
         ("ldk", 64), ("ldvt", 128), ("ldo", 64), ("scale", 0.125), ("flags", 0), ("stream", None))
DUAL = (("q", FAKE), ("k1", FAKE), ("vt1", FAKE), ("k2", FAKE), ("vt2", FAKE), ("o", FAKE), ("n_groups", 4), ("heads", 1), ("nq", 64), ("nk1", 77), ("kv_rows1", 80),
        ("kv_div1", 4), ("ldk1", 64), ("ldvt1", 80), ("nk2", 16), ("kv_rows2", 16), ("kv_div2", 4), ("ldk2", 64), ("ldvt2", 16), ("ldq", 64), ("ldo", 64),
        ("scale", 0.125), ("flags", 0), ("stream", None))
D512 = (("q", FAKE), ("k", FAKE), ("vt", FAKE), ("o", FAKE), ("n_groups", 2), ("nq", 64), ("nk", 60), ("kv_rows", 64), ("ldq", 512), ("ldk", 512), ("ldvt", 128),
        ("ldo", 512), ("scale", 0.04), ("stream", None))
TEMPORAL = (("qkv", FAKE), ("o", FAKE), ("B", 1), ("T", 16), ("P", 9), ("heads", 2), ("ld", 384), ("k_off", 128), ("v_off", 256), ("ldo", 128), ("scale", 0.125))


def _lib():
    from viewcrafter_amd import _lib as L
    return L.lib()


@pytest.mark.parametrize("entry", ["flash", "dual", "d512"])
def test_the_flash_entries_refuse_before_any_launch(entry):
    L = _lib()
    fn, spec, ptrs = dict(flash=(L.vcx_attn_flash_d64_f16, FLASH, ("q", "k", "vt", "o")), dual=(L.vcx_attn_flash_dual_d64_f16, DUAL, ("q", "k1", "vt1", "k2", "vt2", "o")),
                          d512=(L.vcx_attn_flash_d512_f16, D512, ("q", "k", "vt", "o")))[entry]
    s = "1" if entry == "dual" else ""

    def refused(word, **kw):
        assert fn(*_args(spec, **kw)) == -1, kw
        assert word in L.vcx_last_error(), (kw, L.vcx_last_error())

    for name in ptrs:                                              # a null pointer, one at a time
        refused(b"null", **{name: None})
    refused(b"multiples of 8", ldq=68)
    refused(b"multiples of 8", ldo=66)
    refused(b"aligned", o=FAKE + 4)
    refused(b"aligned", q=FAKE + 8)
    refused(b"kv_rows >= nk", **{"kv_rows" + s: 56})               # kv_rows < nk
    refused(b"multiples of 8", **{"kv_rows" + s: 84})              # kv_rows % 8 != 0 (and >= nk)
    if entry != "d512":
        refused(b"empty", heads=0)
    if entry == "dual":
        refused(b"ACCUMULATE", flags=ACC)


def test_the_temporal_entries_refuse_before_any_launch():
    L = _lib()
    plain = lambda **kw: L.vcx_attn_temporal_d64_f16(*_args(TEMPORAL + (("stream", None),), **kw))
    masked = lambda **kw: L.vcx_attn_temporal_d64_masked_f16(*_args(TEMPORAL + (("flags", CAUSAL), ("stream", None)), **kw))
    rel_spec = TEMPORAL[:2] + (("relg", FAKE), ("relp", FAKE), ("R", 3)) + TEMPORAL[2:] + (("flags", 0), ("stream", None))
    rel = lambda **kw: L.vcx_attn_temporal_d64_rel_f16(*_args(rel_spec, **kw))

    def refused(fn, word, **kw):
        assert fn(**kw) == -1, kw
        assert word in L.vcx_last_error(), (kw, L.vcx_last_error())

    for fn in (plain, masked, rel):
        refused(fn, b"null", qkv=None)
        refused(fn, b"null", o=None)
        refused(fn, b"multiples of 8", ldo=68)                     # ldo % 4 == 0 is the FLASH entries' rule: these kernels store 16 bytes
        refused(fn, b"aligned", o=FAKE + 8)
        refused(fn, b"multiples of 8", k_off=4)
        refused(fn, b"T <= 64" if fn is not rel else b"T <= 32", T=65)
        # negative offsets passed % 8 and reached the kernel, which then read in front of the qkv pointer
        refused(fn, b"non-negative", k_off=-8)
        refused(fn, b"non-negative", v_off=-128)
    refused(masked, b"unknown flags", flags=CAUSAL | 8)
    refused(rel, b"unknown flags", flags=LOG2)
    refused(rel, b"1 <= R <= 31", R=0)
    refused(rel, b"1 <= R <= 31", R=32)
    refused(rel, b"T <= 32", T=33)
    refused(rel, b"relg", relg=FAKE + 1)                           # an odd relg pointer
    refused(rel, b"relg", relp=None)


def test_the_row_softmax_refuses_before_any_launch():
    L = _lib()
    call = lambda x=FAKE, rows=37, n=135, ld=136: L.vcx_softmax_rows_f16(x, rows, n, ld, None)
    for kw, word in ((dict(ld=128), b"covers n rounded up to 8"), (dict(ld=132), b"multiple of 8"), (dict(x=FAKE + 8), b"16-byte aligned"), (dict(x=None), b"empty"),
                     (dict(n=0), b"empty")):
        assert call(**kw) == -1, kw
        assert word in L.vcx_last_error(), (kw, L.vcx_last_error())
