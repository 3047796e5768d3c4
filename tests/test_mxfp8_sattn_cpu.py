"""The MXFP8 spatial attention (VCX_SATTN_MXFP8, include/vcx.h vcx_attn_flash_d64_mxfp8 / vcx_attn_flash_dual_d64_mxfp8) without a GPU: the
host graph of a SpatialTransformer with the switch off and on (stand-ins for the ops record the calls), the library's predicates, and the
launchers' validation with fake pointers (they return before any launch)."""
import math

import pytest
import torch

from tests import mx_emulation as MX
from viewcrafter_amd import _lib

ACC, LOG2 = 1, 2          # include/vcx.h VCX_ATTN_ACCUMULATE, VCX_ATTN_LOG2_LOGITS
MX_PREDICATES = ("linear_mxfp8_ok", "linear_t_mxfp8_ok", "flash_attn_mxfp8_ok", "flash_attn_dual_mxfp8_ok")


# ------------------------------------------------------------------------------------------------------------------ host graph
class _Recorder:
    """Stand-ins for the ops a SpatialTransformer calls on its way: they record (name, what matters of the arguments) and return tensors of
    the right shape.  The device-free predicates of the fp16 route (lnfold_ok, rowstats_ok, ...) stay the library's own; `accept` is the
    answer of the stand-ins for the MX predicates (a name: that one refuses)."""

    NAMES = ("group_norm", "group_norm_stats", "group_norm_fold_linear", "gemm_units", "linear", "layer_norm", "row_stats", "rowstats_buffer", "gemm",
             "flash_attn", "flash_attn_dual", "repeat_rows", "copy2d", "quant_mxfp8", "layer_norm_mxfp8", "linear_mxfp8", "linear_t_mxfp8", "flash_attn_mxfp8",
             "flash_attn_dual_mxfp8") + MX_PREDICATES

    def __init__(self, monkeypatch, accept=True):
        from viewcrafter_amd import ops
        self.calls, self.accept = [], accept
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, getattr(self, name))

    def names(self, skip=MX_PREDICATES):
        return [c[0] for c in self.calls if c[0] not in skip]

    def _answer(self, name):
        return self.accept is True or (self.accept is not False and self.accept != name)

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

    def gemm(self, a, w, *, M, N, **kw):
        self.calls.append(("gemm", (M, N)))
        return torch.zeros((M, N), dtype=torch.float16)

    def layer_norm(self, x, gamma, beta, eps=1e-5):
        self.calls.append(("layer_norm", tuple(x.shape)))
        return torch.zeros_like(x)

    def row_stats(self, x, eps=1e-5):
        self.calls.append(("row_stats",))
        return torch.zeros((x.shape[0], 2))

    def rowstats_buffer(self, M, device):
        self.calls.append(("rowstats_buffer",))
        return torch.zeros((M, 2))

    def flash_attn(self, q, k, vt, out, **kw):
        self.calls.append(("flash_attn", kw["nq"], kw["nk"], kw["log2_logits"]))
        return out

    def flash_attn_dual(self, q, k1, vt1, k2, vt2, out, **kw):
        self.calls.append(("flash_attn_dual", kw["nq"], kw["nk1"], kw["nk2"]))
        return out

    def repeat_rows(self, x, r):
        self.calls.append(("repeat_rows", r))
        return x.repeat(r, 1)

    def copy2d(self, src, dst, rows, cols, lds, ldd):
        self.calls.append(("copy2d",))

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
        return self._answer("linear_mxfp8_ok")

    def linear_t_mxfp8_ok(self, tokens, D, K):
        self.calls.append(("linear_t_mxfp8_ok", tokens, D, K))
        return self._answer("linear_t_mxfp8_ok")

    def flash_attn_mxfp8_ok(self, **kw):
        self.calls.append(("flash_attn_mxfp8_ok", kw["n_groups"], kw["nq"], kw["nk"]))
        return self._answer("flash_attn_mxfp8_ok")

    def flash_attn_dual_mxfp8_ok(self, **kw):
        self.calls.append(("flash_attn_dual_mxfp8_ok", kw["n_groups"], kw["nq"], kw["nk1"], kw["nk2"]))
        return self._answer("flash_attn_dual_mxfp8_ok")

    def linear_mxfp8(self, a, w, bias, *, K, residual=None, geglu=False, mx_out=False):
        assert a[0].shape[1] == MX.kp_of(K) and w[0].shape == (bias.numel(), MX.kp_of(K)) and w[1].shape == (bias.numel(), MX.kp_of(K) // 32)
        assert bias.dtype == torch.float32
        self.calls.append(("linear_mxfp8", (a[0].shape[0], w[0].shape[0], K), residual is not None, bool((bias == 0).all())))
        return torch.zeros((a[0].shape[0], w[0].shape[0]), dtype=torch.float16)

    def linear_t_mxfp8(self, x, w, *, K):
        assert x[0].shape[1] == MX.kp_of(K) and w[0].shape[1] == MX.kp_of(K)
        self.calls.append(("linear_t_mxfp8", (x[0].shape[0], w[0].shape[0], K)))
        return torch.zeros((w[0].shape[0], x[0].shape[0]), dtype=torch.float16)

    def flash_attn_mxfp8(self, q, k, vt, **kw):
        self.calls.append(("flash_attn_mxfp8", kw["n_groups"], kw["nq"], kw["nk"], kw["kv_div"]))
        return self._pair(kw["n_groups"] * kw["nq"], 64 * kw["heads"])

    def flash_attn_dual_mxfp8(self, q, k1, vt1, k2, vt2, **kw):
        self.calls.append(("flash_attn_dual_mxfp8", kw["n_groups"], kw["nq"], kw["nk1"], kw["nk2"]))
        return self._pair(kw["n_groups"] * kw["nq"], 64 * kw["heads"])


C, CDIM, N_IMG, FPV = 64, 32, 16, 4


def _transformer(depth=1):
    from viewcrafter_amd.lvdm.modules import attention as A
    torch.manual_seed(C)
    st = A.SpatialTransformer(C, 1, 64, depth=depth, context_dim=CDIM, use_checkpoint=False, use_linear=True, image_cross_attention=True).eval()
    with torch.no_grad():
        for blk in st.transformer_blocks:
            for a in (blk.attn1, blk.attn2):
                a.to_out[0].bias.copy_(0.1 * torch.randn(a.query_dim))
    return A, st


def _context(A, st, videos, image=True):
    """The projected context of `videos` videos, as project_context leaves it (without running a GEMM)."""
    out = []
    for _ in st.transformer_blocks:
        kv = A.ContextKV()
        kv.k_txt, kv.vt_txt = torch.zeros((videos * 80, C), dtype=torch.float16), torch.zeros((C, videos * 80), dtype=torch.float16)
        kv.n_txt_rows, kv.n_txt, kv.n_img, kv.img_per_frame = videos * 80, 77, N_IMG if image else 0, False
        kv.k_img = torch.zeros((videos * N_IMG, C), dtype=torch.float16) if image else None
        kv.vt_img = torch.zeros((C, videos * N_IMG), dtype=torch.float16) if image else None
        out.append(kv)
    return out


def _x(n=2 * FPV, H=6, W=8):
    return torch.zeros((n, H, W, C), dtype=torch.float16)


def _mx_packs(st):
    return [a._pk["mx"] for blk in st.transformer_blocks for a in (blk.attn1, blk.attn2) if a._pk is not None and "mx" in a._pk]


# the ten calls of a block on the MX route (the issue's list; repeat_rows three times - t, q2, xin - where cfg_repeat asks for it)
def _block_mx(cfg=False, dual=True):
    return (["layer_norm_mxfp8", "linear_mxfp8", "linear_t_mxfp8", "flash_attn_mxfp8", "linear_mxfp8", "layer_norm_mxfp8", "linear_mxfp8"]
            + (["repeat_rows"] * 3 if cfg else []) + ["flash_attn_dual_mxfp8" if dual else "flash_attn_mxfp8", "linear_mxfp8"])


def _fp16_run(monkeypatch, st, kv, x, **kw):
    """The calls of today's route, recorded with the switch off."""
    with monkeypatch.context() as mp:
        rec = _Recorder(mp)
        with torch.no_grad():
            st(x, context_kv=kv, frames_per_video=FPV, **kw)
    return rec.names(skip=())


def test_switch_off_makes_the_calls_it_makes_today_and_no_mx_op(monkeypatch):
    A, st = _transformer()
    assert A.SATTN_MXFP8 is False and A.SATTN_MXFP8_SKIP_DIMS == frozenset([320]), "off by default, 320 skipped by default"
    names = _fp16_run(monkeypatch, st, _context(A, st, 2), _x())
    assert not any("mxfp8" in n for n in names), "neither an MX op nor an MX predicate with the switch off"
    assert names.count("flash_attn") == 1 and names.count("flash_attn_dual") == 1 and names.count("gemm") == 1
    assert names[0] == "group_norm" and _mx_packs(st) == []


@pytest.mark.parametrize("depth", [1, 2])
def test_switch_on_runs_the_listed_calls_per_block(monkeypatch, depth):
    A, st = _transformer(depth)
    kv, x = _context(A, st, 2), _x()
    today = _fp16_run(monkeypatch, st, kv, x)
    monkeypatch.setattr(A, "SATTN_MXFP8", True)
    monkeypatch.setattr(A, "SATTN_MXFP8_SKIP_DIMS", frozenset())
    rec = _Recorder(monkeypatch)
    with torch.no_grad():
        y, cs = st(x, context_kv=kv, frames_per_video=FPV)
    names = rec.names()
    # head (norm, proj_in) and tail (feed-forward, proj_out) are today's; between them the listed calls per block, a feed-forward between blocks
    head = today[:today.index("linear") + 1]
    assert head == ["group_norm", "linear"] and names[:2] == head
    body = names[2:]
    for b in range(depth):
        assert body[:9] == _block_mx(), f"block {b}: {body[:9]}"          # (nine: no repeat_rows without cfg_repeat)
        body = body[9:]
        if b + 1 < depth:
            nxt = body.index("layer_norm_mxfp8")
            assert 0 < nxt <= 4 and not any("mxfp8" in n for n in body[:nxt]), "the feed-forward between two blocks stays today's"
            body = body[nxt:]
    assert body and not any("mxfp8" in n for n in body), "feed-forward and proj_out keep today's code"
    tail = today[len(today) - len(body):]
    assert body == tail, "the last block's feed-forward + proj_out are the calls of today's route"
    every = rec.names(skip=())
    first_op = min(i for i, n in enumerate(every) if not n.endswith("_ok"))
    assert all(n.endswith("_ok") for n in every[:first_op]) and not any(n.endswith("_ok") for n in every[first_op:]), "the route is decided before anything runs"
    # one video's frames, then the call's
    asked = [c for c in rec.calls if c[0].endswith("_ok")]
    assert [c[1] for c in asked if c[0] == "flash_attn_mxfp8_ok"] == [FPV, 2 * FPV]
    assert [c[1] for c in asked if c[0] == "flash_attn_dual_mxfp8_ok"] == [FPV] * depth + [2 * FPV] * depth
    assert ("linear_t_mxfp8_ok", FPV * 48, C, C) in asked and ("linear_t_mxfp8_ok", 2 * FPV * 48, C, C) in asked
    assert ("linear_mxfp8_ok", FPV * 48, 2 * C, C, False) in asked and ("linear_mxfp8_ok", FPV * 48, C, C, True) in asked
    tokens = 2 * FPV * 48
    lin = [c for c in rec.calls if c[0] == "linear_mxfp8"]
    assert [c[1] for c in lin] == [(tokens, 2 * C, C), (tokens, C, C), (tokens, C, C), (tokens, C, C)] * depth
    assert [c[2] for c in lin] == [False, True, False, True] * depth, "the projections have no residual, both to_out have the token stream"
    assert [c[3] for c in lin] == [True, False, True, False] * depth, "the projections get the zero bias, to_out its own"
    assert [c for c in rec.calls if c[0] == "flash_attn_mxfp8"] == [("flash_attn_mxfp8", 2 * FPV, 48, 48, 1)] * depth
    assert [c for c in rec.calls if c[0] == "flash_attn_dual_mxfp8"] == [("flash_attn_dual_mxfp8", 2 * FPV, 48, 77, N_IMG)] * depth
    assert not any(c[0] == "linear" and c[3] for c in rec.calls) and "rowstats_buffer" not in names and "row_stats" not in names[:12], \
        "no row statistics are requested on the MX route"
    packs = _mx_packs(st)
    assert len(packs) == 2 * depth
    a1, a2 = st.transformer_blocks[0].attn1, st.transformer_blocks[0].attn2
    m1, m2 = packs[0], packs[1]
    assert [tuple(t.shape) for t in (*m1["wqk"], *m1["wv"], *m1["wo"])] == [(128, 128), (128, 4), (64, 128), (64, 4), (64, 128), (64, 4)]
    assert [tuple(t.shape) for t in (*m2["wq"], *m2["wo"])] == [(64, 128), (64, 4), (64, 128), (64, 4)]
    assert tuple(m1["zero"].shape) == (128,) and tuple(m2["zero"].shape) == (64,) and not m1["zero"].any() and not m2["zero"].any()
    # the pairs of the un-folded, pre-scaled weights
    s1 = math.sqrt(a1.scale * 1.4426950408889634)
    q, s = MX.quant((torch.cat([a1.to_q.weight, a1.to_k.weight], 0).detach().float() * s1).half())
    assert torch.equal(m1["wqk"][0], q) and torch.equal(m1["wqk"][1], s)
    q, s = MX.quant(a1.to_v.weight.detach().half())
    assert torch.equal(m1["wv"][0], q) and torch.equal(m1["wv"][1], s)
    q, s = MX.quant((a2.to_q.weight.detach().float() * (a2.scale * 1.4426950408889634)).half())
    assert torch.equal(m2["wq"][0], q) and torch.equal(m2["wq"][1], s)
    # built once, dropped by load_state_dict
    with torch.no_grad():
        st(x, context_kv=kv, frames_per_video=FPV)
    assert all(a is b for a, b in zip(_mx_packs(st), packs))
    st.load_state_dict(st.state_dict())
    assert _mx_packs(st) == [], "loading a state dict drops the MX packs with the fp16 packs"
    assert y.shape == (2 * FPV, 6, 8, C) and cs is None


def test_cfg_repeat_padded_tokens_and_text_only_context(monkeypatch):
    A, st = _transformer()
    monkeypatch.setattr(A, "SATTN_MXFP8", True)
    monkeypatch.setattr(A, "SATTN_MXFP8_SKIP_DIMS", frozenset())
    # the shared CFG prefix: the replication stays in front of the cross-attention, which runs on the replicated rows
    rec = _Recorder(monkeypatch)
    with torch.no_grad():
        y, _ = st(_x(FPV), context_kv=_context(A, st, 2), frames_per_video=FPV, cfg_repeat=2)
    assert rec.names()[2:14] == _block_mx(cfg=True) and y.shape[0] == 2 * FPV
    assert [c for c in rec.calls if c[0] in ("flash_attn_mxfp8", "flash_attn_dual_mxfp8")] == [("flash_attn_mxfp8", FPV, 48, 48, 1),
                                                                                              ("flash_attn_dual_mxfp8", 2 * FPV, 48, 77, N_IMG)]
    assert [c[1] for c in rec.calls if c[0] == "flash_attn_mxfp8_ok"] == [FPV, 2 * FPV], "asked about the replicated call as well"
    # 6 x 10 = 60 tokens a frame: padded to 64 rows, nq = 64 and nk = 60 as today
    rec.calls.clear()
    with torch.no_grad():
        y, _ = st(_x(2 * FPV, 6, 10), context_kv=_context(A, st, 2), frames_per_video=FPV)
    assert ("flash_attn_mxfp8", 2 * FPV, 64, 60, 1) in rec.calls and ("flash_attn_dual_mxfp8", 2 * FPV, 64, 77, N_IMG) in rec.calls
    assert y.shape == (2 * FPV, 6, 10, C)
    # no image context: the single-set entry, keys shared by the frames of a video
    rec.calls.clear()
    with torch.no_grad():
        st(_x(), context_kv=_context(A, st, 2, image=False), frames_per_video=FPV)
    assert rec.names()[2:11] == _block_mx(dual=False)
    assert [c for c in rec.calls if c[0] == "flash_attn_mxfp8"] == [("flash_attn_mxfp8", 2 * FPV, 48, 48, 1), ("flash_attn_mxfp8", 2 * FPV, 48, 77, FPV)]


@pytest.mark.parametrize("why", ["refused", "skipped"] + list(MX_PREDICATES))
def test_a_refusal_keeps_todays_calls_and_builds_no_mx_pack(monkeypatch, why):
    A, st = _transformer()
    kv, x = _context(A, st, 2), _x()
    today = _fp16_run(monkeypatch, st, kv, x)
    monkeypatch.setattr(A, "SATTN_MXFP8", True)
    monkeypatch.setattr(A, "SATTN_MXFP8_SKIP_DIMS", frozenset([C]) if why == "skipped" else frozenset())
    rec = _Recorder(monkeypatch, accept={"refused": False, "skipped": True}.get(why, why))
    with torch.no_grad():
        y, _ = st(x, context_kv=kv, frames_per_video=FPV)
    assert rec.names() == today, "a refusal keeps today's calls, all of them"
    assert any(n.endswith("_ok") for n in rec.names(skip=())) == (why != "skipped")
    assert _mx_packs(st) == [] and y.shape == x.shape


def record_every_op(monkeypatch):
    """Every function of viewcrafter_amd.ops behind a wrapper that notes its name and calls through -> the list of the names called from
    outside ops (what one of them calls inside ops is its own business)."""
    import types

    from viewcrafter_amd import ops
    seen, depth = [], [0]

    def wrap(name, fn):
        def call(*a, **kw):
            if depth[0] == 0:
                seen.append(name)
            depth[0] += 1
            try:
                return fn(*a, **kw)
            finally:
                depth[0] -= 1
        return call
    for name, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_"):
            monkeypatch.setattr(ops, name, wrap(name, fn))
    return seen


def is_a_question(name):
    return name.endswith("_ok") or name in ("tune_get", "units_route")


@pytest.mark.parametrize("switches", ["off", "mx", "pool", "both"])
def test_the_plan_launches_and_allocates_nothing(monkeypatch, switches):
    A, st = _transformer(2)
    monkeypatch.setattr(A, "SATTN_MXFP8", switches in ("mx", "both"))
    monkeypatch.setattr(A, "SATTN_MXFP8_SKIP_DIMS", frozenset())
    monkeypatch.setattr(A, "SATTN_KV_POOL", "mean" if switches in ("pool", "both") else None)
    monkeypatch.setattr(A, "SATTN_KV_POOL_MIN_TOKENS", 96)
    seen = record_every_op(monkeypatch)
    plans = [st._plan(_x(FPV, H, W), _context(A, st, 2), FPV, 2) for H, W in ((6, 8), (6, 10), (8, 12))]
    assert seen and all(is_a_question(n) for n in seen), [n for n in seen if not is_a_question(n)]
    assert [p.N for p in plans] == [48, 64, 96] and all(p.fold is False for p in plans)
    pooled = switches in ("pool", "both")
    small = "mx" if switches in ("mx", "both") else "fp16"          # 6x8 and 6x10 are below the pooling threshold
    assert [p.engine for p in plans] == [small, small, {"off": "fp16", "mx": "mx", "pool": "pool", "both": "pool"}[switches]]
    assert [p.pool for p in plans] == [None, None, (4, 6) if pooled else None]
    assert ("layer_norm_pool2x2_ok" in seen) == pooled and any("mxfp8" in n for n in seen) == (switches in ("mx", "both"))
    assert not any(p.rowstats for p in plans if p.engine == "mx")
    with pytest.raises(AttributeError):
        plans[0].engine = "mx"


# ------------------------------------------------------------------------------------------------------------------ the predicates
def _ok1(n_groups=50, heads=10, nq=2304, nk=2304, kv_rows=2304, kv_div=1, ldq=1280, ldk=1280, ldvt=50 * 2304, flags=LOG2):
    return _lib.lib().vcx_attn_flash_d64_mxfp8_ok(n_groups, heads, nq, nk, kv_rows, kv_div, ldq, ldk, ldvt, flags)


def _ok2(n_groups=50, heads=10, nq=2304, nk1=77, kv_rows1=80, kv_div1=25, ldk1=640, ldvt1=160, nk2=256, kv_rows2=256, kv_div2=25, ldk2=640, ldvt2=512,
         ldq=640, flags=LOG2):
    return _lib.lib().vcx_attn_flash_dual_d64_mxfp8_ok(n_groups, heads, nq, nk1, kv_rows1, kv_div1, ldk1, ldvt1, nk2, kv_rows2, kv_div2, ldk2, ldvt2, ldq, flags)


def test_the_real_predicates():
    from viewcrafter_amd import ops
    L = _lib.lib()
    for ok in (_ok1, _ok2):
        assert ok() == 1
        assert ok(flags=LOG2 | ACC) == 0 and b"ACCUMULATE" in L.vcx_last_error()
        assert ok(flags=0) == 0 and b"LOG2_LOGITS" in L.vcx_last_error()
        assert ok(flags=LOG2 | 8) == 0 and b"flags" in L.vcx_last_error()
        assert ok(heads=0) == 0 and ok(nq=0) == 0 and ok(ldq=1284) == 0
    assert _ok1(n_groups=1, heads=1, nq=64, nk=60, kv_rows=64, ldq=128, ldk=128, ldvt=64) == 1, "padded tokens: nk below kv_rows"
    assert _ok1(nk=2305) == 0 and b"kv_rows" in L.vcx_last_error()
    assert _ok2(kv_rows1=76) == 0 and _ok2(nk2=0) == 0
    # n_groups nq x Kp below 4 GiB: one head has Kp = 128, five heads (D = 320) Kp = 384
    assert _ok1(n_groups=1 << 13, heads=1, nq=1 << 12, nk=64, kv_rows=64, ldq=64, ldk=64, ldvt=1 << 19) == 0 and b"4 GiB" in L.vcx_last_error()      # 2^25 rows x 128 exactly
    assert _ok1(n_groups=(1 << 13) - 1, heads=1, nq=1 << 12, nk=64, kv_rows=64, ldq=64, ldk=64, ldvt=1 << 19) == 1
    assert _ok1(n_groups=2730, heads=5, nq=1 << 12, nk=64, kv_rows=64, ldq=320, ldk=320, ldvt=2730 * 64) == 1            # 384 bytes a row: 10.67 x 2^20 rows
    assert _ok1(n_groups=2731, heads=5, nq=1 << 12, nk=64, kv_rows=64, ldq=320, ldk=320, ldvt=2731 * 64) == 0 and b"4 GiB" in L.vcx_last_error()
    assert 2731 * (1 << 12) * 320 < (1 << 32), "refused for the padded pitch, not for D"
    assert _ok2(n_groups=(1 << 13) * 25, heads=1, nq=1 << 12, ldq=64, ldk1=64, ldk2=64) == 0 and b"4 GiB" in L.vcx_last_error()
    # the first-form resident kernel has no MX store tail: knob XATTN_RESIDENT = 2 refuses what would need it; the knob off uses the flash kernel
    old = ops.tune_get("XATTN_RESIDENT")
    try:
        ops.tune_set("XATTN_RESIDENT", 2)
        assert _ok2() == 0 and b"first-form" in L.vcx_last_error()
        assert _ok2(kv_div2=1, ldvt2=50 * 256) == 1, "image keys per frame: the DUAL flash kernel, whatever the knob"
        ops.tune_set("XATTN_RESIDENT", 0)
        assert _ok2() == 1
    finally:
        ops.tune_set("XATTN_RESIDENT", old)
    assert _ok2() == 1
    # ops returns the library's answers; the transposed projection adds the tile overreach of the token side
    assert ops.flash_attn_mxfp8_ok(n_groups=50, heads=10, nq=2304, nk=2304, kv_rows=2304, kv_div=1, ldq=1280, ldk=1280, ldvt=50 * 2304) is True
    assert ops.flash_attn_mxfp8_ok(n_groups=50, heads=10, nq=2304, nk=2304, kv_rows=2304, kv_div=1, ldq=1280, ldk=1280, ldvt=50 * 2304, accumulate=True) is False
    assert ops.flash_attn_mxfp8_ok(n_groups=50, heads=10, nq=2304, nk=2304, kv_rows=2304, kv_div=1, ldq=1280, ldk=1280, ldvt=50 * 2304, log2_logits=False) is False
    assert ops.flash_attn_dual_mxfp8_ok(n_groups=50, heads=10, nq=2304, nk1=77, kv_rows1=80, kv_div1=25, ldk1=640, ldvt1=160, nk2=256, kv_rows2=256, kv_div2=25,
                                        ldk2=640, ldvt2=512, ldq=640) is True
    assert ops.linear_t_mxfp8_ok(115200, 640, 640) is True and ops.linear_t_mxfp8_ok(600, 64, 64) is True
    assert ops.linear_t_mxfp8_ok(604, 64, 64) is False, "tokens % 8"
    tokens = 6710760          # K = 640: tokens x Kp stays below the library's limit, (tokens + 127) Kp reaches 2^32
    assert tokens * 640 < 0xFFFF0000 <= (1 << 32) <= (tokens + 127) * 640 and L.vcx_gemm_mxfp8_ok(64, tokens, 640, 1) == 1
    assert ops.linear_t_mxfp8_ok(tokens, 64, 640) is False and ops.linear_t_mxfp8_ok(tokens - 8, 64, 640) is True


def test_the_launchers_validate_before_any_launch():
    L = _lib.lib()
    FAKE = 1 << 20
    one = lambda **kw: [kw.get(k, d) for k, d in (("q", FAKE), ("k", FAKE), ("vt", FAKE), ("oq", FAKE), ("os", FAKE), ("n_groups", 2), ("heads", 1), ("nq", 64),
                                                  ("nk", 64), ("kv_rows", 64), ("kv_div", 1), ("ldq", 64), ("ldk", 64), ("ldvt", 128), ("scale", 1.0),
                                                  ("flags", LOG2), ("stream", None))]
    two = lambda **kw: [kw.get(k, d) for k, d in (("q", FAKE), ("k1", FAKE), ("vt1", FAKE), ("k2", FAKE), ("vt2", FAKE), ("oq", FAKE), ("os", FAKE), ("n_groups", 4),
                                                  ("heads", 1), ("nq", 64), ("nk1", 77), ("kv_rows1", 80), ("kv_div1", 4), ("ldk1", 64), ("ldvt1", 80), ("nk2", 16),
                                                  ("kv_rows2", 16), ("kv_div2", 4), ("ldk2", 64), ("ldvt2", 16), ("ldq", 64), ("scale", 1.0), ("flags", LOG2),
                                                  ("stream", None))]
    for fn, args, ptrs in ((L.vcx_attn_flash_d64_mxfp8, one, ("q", "k", "vt", "oq", "os")),
                           (L.vcx_attn_flash_dual_d64_mxfp8, two, ("q", "k1", "vt1", "k2", "vt2", "oq", "os"))):
        for name in ptrs:
            assert fn(*args(**{name: None})) == -1 and b"null" in L.vcx_last_error(), name
        assert fn(*args(oq=FAKE + 8)) == -1 and b"aligned" in L.vcx_last_error()
        assert fn(*args(q=FAKE + 8)) == -1 and b"aligned" in L.vcx_last_error()
        assert fn(*args(os=FAKE + 2)) == -1 and b"aligned" in L.vcx_last_error()
        assert fn(*args(flags=LOG2 | ACC)) == -1 and b"ACCUMULATE" in L.vcx_last_error()
        assert fn(*args(flags=0)) == -1 and b"LOG2_LOGITS" in L.vcx_last_error()
        assert fn(*args(heads=0)) == -1 and fn(*args(nq=0)) == -1 and fn(*args(ldq=68)) == -1
    assert L.vcx_attn_flash_d64_mxfp8(*one(nk=65)) == -1 and b"kv_rows" in L.vcx_last_error()
    assert L.vcx_attn_flash_dual_d64_mxfp8(*two(kv_rows1=76)) == -1 and b"kv_rows" in L.vcx_last_error()
