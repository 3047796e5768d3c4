"""The MXFP8 temporal attention (VCX_TATTN_MXFP8, include/vcx.h vcx_attn_temporal_d64_mxfp8) without a GPU: the host graph of a
TemporalTransformer with the switch off and on (stand-ins for the ops record the calls), the library's shape predicate, and the launcher's
validation with fake pointers (it returns before any launch)."""
import pytest
import torch

from tests import mx_emulation as MX
from viewcrafter_amd import _lib

CAUSAL = 4          # include/vcx.h VCX_ATTN_CAUSAL


# ------------------------------------------------------------------------------------------------------------------ host graph
class _Recorder:
    """Stand-ins for the ops a TemporalTransformer calls on its way: they record (name, what matters of the arguments) and return tensors
    of the right shape.  The device-free predicates of the fp16 route (lnfold_ok, rowstats_ok, ...) stay the library's own; `accept` is
    the answer of the stand-ins for the three MX predicates."""

    NAMES = ("group_norm", "group_norm_stats", "group_norm_fold_linear", "gemm_units", "linear", "layer_norm", "row_stats", "rowstats_buffer",
             "temporal_attn", "temporal_attn_rel", "gemm", "layer_norm_mxfp8", "linear_mxfp8", "linear_mxfp8_ok", "temporal_attn_mxfp8",
             "temporal_attn_mxfp8_ok", "quant_mxfp8")

    def __init__(self, monkeypatch, accept=True):
        from viewcrafter_amd import ops
        self.calls, self.accept = [], accept
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, getattr(self, name))

    def names(self, skip=("linear_mxfp8_ok", "temporal_attn_mxfp8_ok")):
        return [c[0] for c in self.calls if c[0] not in skip]

    def group_norm(self, x, gamma, beta, eps, silu, groups=32, out=None, stats=None, x2=None):
        self.calls.append(("group_norm", tuple(x.shape)))
        return torch.zeros_like(x, dtype=torch.float16)

    def group_norm_stats(self, x, groups=32):
        self.calls.append(("group_norm_stats",))
        return torch.zeros((x.shape[0], groups, 2))

    def group_norm_fold_linear(self, w32, bias, gamma, beta, stats, eps, groups=32):
        self.calls.append(("group_norm_fold_linear",))
        n = stats.shape[0]
        return torch.zeros((n,) + tuple(w32.shape), dtype=torch.float16), torch.zeros((n, w32.shape[0]))

    def gemm_units(self, a, wn, bn, *, unit_rows, out=None, rowstats=None, rowstats_eps=1e-5):
        self.calls.append(("gemm_units", rowstats is not None))
        return torch.zeros((a.shape[0], wn.shape[1]), dtype=torch.float16)

    def linear(self, x, w, bias=None, **kw):
        self.calls.append(("linear", (x.shape[0], w.shape[0], x.shape[1]), kw.get("residual") is not None, kw.get("rowstats") is not None,
                           kw.get("ln_stats") is not None))
        out = kw.get("out")
        n = w.shape[0] // 2 if kw.get("geglu") else w.shape[0]
        return torch.zeros((x.shape[0], n), dtype=torch.float16) if out is None else out

    def gemm(self, a, w, **kw):
        self.calls.append(("gemm",))
        return kw.get("out")

    def layer_norm(self, x, gamma, beta, eps=1e-5):
        self.calls.append(("layer_norm", tuple(x.shape)))
        return torch.zeros_like(x)

    def row_stats(self, x, eps=1e-5):
        self.calls.append(("row_stats",))
        return torch.zeros((x.shape[0], 2))

    def rowstats_buffer(self, M, device):
        self.calls.append(("rowstats_buffer",))
        return torch.zeros((M, 2))

    def temporal_attn(self, qkv, out, **kw):
        self.calls.append(("temporal_attn", kw["causal"]))
        return out

    def temporal_attn_rel(self, qkv, out, relg, relp, **kw):
        self.calls.append(("temporal_attn_rel",))
        return out

    def quant_mxfp8(self, x):
        self.calls.append(("quant_mxfp8",))
        return self._pair(x.shape[0], x.shape[1])

    @staticmethod
    def _pair(rows, K):
        kp = MX.kp_of(K)
        return torch.zeros((rows, kp), dtype=torch.uint8), torch.zeros((rows, kp // 32), dtype=torch.uint8)

    def layer_norm_mxfp8(self, x, gamma, beta, eps=1e-5):
        self.calls.append(("layer_norm_mxfp8", tuple(x.shape)))
        return self._pair(*x.shape)

    def linear_mxfp8_ok(self, rows, N, K, *, residual=False, geglu=False, mx_out=False):
        self.calls.append(("linear_mxfp8_ok", rows, N, K, residual))
        return self.accept

    def temporal_attn_mxfp8_ok(self, B, T, P, heads, ld, causal=False):
        self.calls.append(("temporal_attn_mxfp8_ok", B, T, P, heads, ld, causal))
        return self.accept

    def linear_mxfp8(self, a, w, bias, *, K, residual=None, geglu=False, mx_out=False):
        assert a[0].shape[1] == MX.kp_of(K) and w[0].shape == (bias.numel(), MX.kp_of(K)) and w[1].shape == (bias.numel(), MX.kp_of(K) // 32)
        assert bias.dtype == torch.float32
        self.calls.append(("linear_mxfp8", (a[0].shape[0], w[0].shape[0], K), residual is not None, bool((bias == 0).all())))
        return torch.zeros((a[0].shape[0], w[0].shape[0]), dtype=torch.float16)

    def temporal_attn_mxfp8(self, qkv, *, B, T, P, heads, ld, k_off, v_off, scale, causal=False):
        assert tuple(qkv.shape) == (B * T * P, 3 * 64 * heads) and ld == 3 * 64 * heads and k_off == 64 * heads and v_off == 2 * 64 * heads
        self.calls.append(("temporal_attn_mxfp8", causal))
        return self._pair(B * T * P, 64 * heads)


def _transformer(C=64, heads=1, **kw):
    from viewcrafter_amd.lvdm.modules import attention as A
    torch.manual_seed(C)
    tr = A.TemporalTransformer(C, heads, 64, **kw).eval()
    with torch.no_grad():
        for blk in tr.transformer_blocks:
            for a in (blk.attn1, blk.attn2):
                a.to_out[0].bias.copy_(0.1 * torch.randn(a.query_dim))
    return A, tr


# what a TemporalTransformer(64, 1, 64) forward of [2, 3, 8, 64] calls on the fp16 route: the per-video norm, proj_in, two self-attentions
# (statistics for the folded q|k|v projection, the projection, the attention kernel, to_out + residual), then the feed-forward with proj_out
ATTN_FP16 = ["row_stats", "linear", "temporal_attn", "linear"]
ATTN_MX = ["layer_norm_mxfp8", "linear_mxfp8", "temporal_attn_mxfp8", "linear_mxfp8"]
HEAD, TAIL = ["group_norm", "linear"], ["layer_norm", "linear", "linear", "linear"]
FP16_CALLS = HEAD + ATTN_FP16 * 2 + TAIL
MX_CALLS = HEAD + ATTN_MX * 2 + TAIL
B, T, P = 2, 3, 8


def _x(C=64, T_=T):
    return torch.zeros((B, T_, P, C), dtype=torch.float16)


def _mx_packs(tr):
    return [a._pk["mx"] for blk in tr.transformer_blocks for a in (blk.attn1, blk.attn2) if a._pk is not None and "mx" in a._pk]


def test_switch_off_makes_the_calls_it_makes_today_and_no_mx_op(monkeypatch):
    A, tr = _transformer()
    assert A.TATTN_MXFP8 is False, "the switch is off by default"
    rec = _Recorder(monkeypatch)
    with torch.no_grad():
        y, cs = tr(_x())
    assert rec.names(skip=()) == FP16_CALLS, "neither an MX op nor an MX predicate with the switch off"
    assert y.shape == (B, T, P, 64) and cs is None and _mx_packs(tr) == []


@pytest.mark.parametrize("causal", [False, True])
def test_switch_on_runs_the_four_mx_ops_per_attention(monkeypatch, causal):
    A, tr = _transformer(causal_attention=causal, temporal_length=T)
    monkeypatch.setattr(A, "TATTN_MXFP8", True)
    monkeypatch.setattr(A, "TATTN_MXFP8_SKIP_DIMS", frozenset())
    rec = _Recorder(monkeypatch)
    with torch.no_grad():
        y, cs = tr(_x())
    assert rec.names() == MX_CALLS
    every = rec.names(skip=())
    first_op = min(i for i, n in enumerate(every) if not n.endswith("_ok"))
    assert all(n.endswith("_ok") for n in every[:first_op]) and not any(n.endswith("_ok") for n in every[first_op:]), "the route is decided before anything runs"
    rows = T * P
    asked = [c for c in rec.calls if c[0].endswith("_ok")]
    assert asked == [("linear_mxfp8_ok", rows, 192, 64, False), ("linear_mxfp8_ok", rows, 64, 64, True), ("temporal_attn_mxfp8_ok", 1, T, P, 1, 192, causal),
                     ("linear_mxfp8_ok", B * rows, 192, 64, False), ("linear_mxfp8_ok", B * rows, 64, 64, True),
                     ("temporal_attn_mxfp8_ok", B, T, P, 1, 192, causal)], "one video's rows, then the call's"
    lin = [c for c in rec.calls if c[0] == "linear_mxfp8"]
    assert [c[1] for c in lin] == [(B * rows, 192, 64), (B * rows, 64, 64)] * 2
    assert [c[2] for c in lin] == [False, True] * 2, "q|k|v has no residual, to_out has the token stream"
    assert [c[3] for c in lin] == [True, False] * 2, "q|k|v gets the zero bias, to_out its own"
    assert [c[1] for c in rec.calls if c[0] == "temporal_attn_mxfp8"] == [causal, causal]
    assert not any(c[0] == "linear" and c[3] for c in rec.calls), "no row statistics are requested on the MX route"
    packs = _mx_packs(tr)
    assert len(packs) == 2
    for mx in packs:
        assert [tuple(t.shape) for t in (*mx["wqkv"], *mx["wo"])] == [(192, 128), (192, 4), (64, 128), (64, 4)]
        assert all(t.dtype == torch.uint8 for t in (*mx["wqkv"], *mx["wo"]))
        assert mx["zero"].dtype == torch.float32 and tuple(mx["zero"].shape) == (192,) and not mx["zero"].any() and tuple(mx["bo"].shape) == (64,)
    # the pair of the un-folded cat(Wq, Wk, Wv)
    a1 = tr.transformer_blocks[0].attn1
    w = torch.cat([a1.to_q.weight, a1.to_k.weight, a1.to_v.weight], 0).detach().half()
    q, s = MX.quant(w)
    assert torch.equal(packs[0]["wqkv"][0], q) and torch.equal(packs[0]["wqkv"][1], s)
    # built once, dropped by load_state_dict
    with torch.no_grad():
        tr(_x())
    assert all(a is b for a, b in zip(_mx_packs(tr), packs))
    tr.load_state_dict(tr.state_dict())
    assert _mx_packs(tr) == [], "loading a state dict drops the MX packs with the fp16 packs"
    assert y.shape == (B, T, P, 64) and cs is None


@pytest.mark.parametrize("why", ["refused", "skipped", "relative_position", "T33"])
def test_a_refusal_keeps_todays_calls_and_builds_no_mx_pack(monkeypatch, why):
    kw = dict(relative_position=True, temporal_length=8) if why == "relative_position" else {}
    A, tr = _transformer(**kw)
    monkeypatch.setattr(A, "TATTN_MXFP8", True)
    monkeypatch.setattr(A, "TATTN_MXFP8_SKIP_DIMS", frozenset([64]) if why == "skipped" else frozenset())
    rec = _Recorder(monkeypatch, accept=why != "refused")
    Tn = 33 if why == "T33" else T
    with torch.no_grad():
        y, _ = tr(_x(T_=Tn))
    if why == "relative_position":
        want = HEAD + ["row_stats", "linear", "gemm", "temporal_attn_rel", "gemm", "linear"] * 2 + TAIL
    else:
        want = FP16_CALLS
    assert rec.names() == want
    assert ("linear_mxfp8_ok" in rec.names(skip=())) == (why == "refused")
    assert _mx_packs(tr) == [] and y.shape == (B, Tn, P, 64)


@pytest.mark.parametrize("switch", [False, True])
def test_the_plan_launches_and_allocates_nothing(monkeypatch, switch):
    from tests.test_mxfp8_sattn_cpu import is_a_question, record_every_op
    A, tr = _transformer(depth=2)
    monkeypatch.setattr(A, "TATTN_MXFP8", switch)
    monkeypatch.setattr(A, "TATTN_MXFP8_SKIP_DIMS", frozenset())
    monkeypatch.setattr(A, "GN_FOLD_MIN_BYTES", 0)
    seen = record_every_op(monkeypatch)
    plans = [tr._plan(_x(T_=Tn)) for Tn in (T, 33)]
    assert seen and all(is_a_question(n) for n in seen), [n for n in seen if not is_a_question(n)]
    assert [p.engine for p in plans] == ["mx" if switch else "fp16", "fp16"], "T = 33 keeps fp16"
    assert all(p.fold is True for p in plans) and ("temporal_attn_mxfp8_ok" in seen) == switch
    assert not any(p.rowstats for p in plans if p.engine == "mx")
    monkeypatch.setattr(A, "GN_FOLD", False)
    assert tr._plan(_x()).fold is False
    with pytest.raises(AttributeError):
        plans[0].engine = "mx"


# ------------------------------------------------------------------------------------------------------------------ the shape predicate
def _ok(B, T, P, heads, ld, flags=0):
    return _lib.lib().vcx_attn_temporal_d64_mxfp8_ok(B, T, P, heads, ld, flags)


def test_the_real_predicate():
    from viewcrafter_amd import ops
    L = _lib.lib()
    assert _ok(2, 25, 9216, 10, 1920) == 1 and _ok(2, 1, 1, 1, 192) == 1 and _ok(2, 25, 9216, 10, 1920, CAUSAL) == 1
    assert _ok(2, 33, 64, 1, 192) == 0 and b"T <= 32" in L.vcx_last_error()
    assert _ok(2, 0, 64, 1, 192) == 0 and b"T <= 32" in L.vcx_last_error()
    assert _ok(2, 3, 64, 1, 196) == 0 and b"ld" in L.vcx_last_error()
    for flags in (1, 2, 8, CAUSAL | 1, 0x800):
        assert _ok(2, 3, 64, 1, 192, flags) == 0 and b"flags" in L.vcx_last_error(), flags
    # B T P x Kp(D) below 4 GiB: D = 320 has Kp = 384
    P = 1 << 20
    assert _ok(1, 32, P, 1, 192) == 0 and b"4 GiB" in L.vcx_last_error()                   # 2^25 rows x 128 = 4 GiB exactly
    assert _ok(1, 31, P, 1, 192) == 1
    assert _ok(1, 10, P, 5, 960) == 1 and _ok(1, 11, P, 5, 960) == 0 and b"4 GiB" in L.vcx_last_error()      # 384 bytes a row: 10.67 x 2^20 rows
    assert 11 * P * 320 < (1 << 32), "refused for the padded pitch, not for D"
    # ops returns the library's answer
    assert ops.temporal_attn_mxfp8_ok(2, 25, 9216, 10, 1920) is True and ops.temporal_attn_mxfp8_ok(2, 33, 64, 1, 192) is False
    assert ops.temporal_attn_mxfp8_ok(2, 25, 64, 1, 192, causal=True) is True


def test_the_launcher_validates_before_any_launch():
    L = _lib.lib()
    FAKE = 1 << 20
    args = lambda **kw: [kw.get(k, d) for k, d in (("qkv", FAKE), ("q", FAKE), ("s", FAKE), ("B", 2), ("T", 3), ("P", 64), ("heads", 1), ("ld", 192), ("k_off", 64),
                                                   ("v_off", 128), ("scale", 0.125), ("flags", 0), ("stream", None))]
    for name in ("qkv", "q", "s"):
        assert L.vcx_attn_temporal_d64_mxfp8(*args(**{name: None})) == -1 and b"null" in L.vcx_last_error(), name
    assert L.vcx_attn_temporal_d64_mxfp8(*args(q=FAKE + 8)) == -1 and b"aligned" in L.vcx_last_error()
    assert L.vcx_attn_temporal_d64_mxfp8(*args(qkv=FAKE + 8)) == -1 and b"aligned" in L.vcx_last_error()
    assert L.vcx_attn_temporal_d64_mxfp8(*args(s=FAKE + 2)) == -1 and b"aligned" in L.vcx_last_error()
    assert L.vcx_attn_temporal_d64_mxfp8(*args(T=33)) == -1 and b"T <= 32" in L.vcx_last_error()
    assert L.vcx_attn_temporal_d64_mxfp8(*args(k_off=65)) == -1 and b"k_off" in L.vcx_last_error()
    assert L.vcx_attn_temporal_d64_mxfp8(*args(v_off=132)) == -1 and b"v_off" in L.vcx_last_error()
    assert L.vcx_attn_temporal_d64_mxfp8(*args(flags=1)) == -1 and b"flags" in L.vcx_last_error()
    assert L.vcx_attn_temporal_d64_mxfp8(*args(ld=196)) == -1
