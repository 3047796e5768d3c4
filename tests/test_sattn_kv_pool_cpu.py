"""The spatial self-attention over 2x2-pooled keys and values (VCX_SATTN_KV_POOL, include/vcx_pool.h vcx_layernorm_pool2x2_f16) without a GPU:
kv_pool_plan, the host graph of a SpatialTransformer with the switch off and on (stand-ins for the ops record the calls), its interplay
with VCX_SATTN_MXFP8, the module on the CPU stand-ins against the fp32 reference tests/kv_pool_ref.py, the stand-in itself, and the
launcher's validation with fake pointers (it returns before any launch)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from oracle import lvdm_oracle as O
from oracle.weights import synth_input
from tests import cpu_kernels as CK
from tests import cpu_kernels_kv_pool as CKP
from tests import kv_pool_ref as REF
from tests.test_mxfp8_sattn_cpu import C, FPV, N_IMG, _Recorder, _block_mx, _context, _fp16_run, _transformer, _x
from tests.util import load_synth, rel_l2
from viewcrafter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNET_TOL = 5e-3          # tests/test_hostgraph_cpu.py / tests/test_model_gpu.py: the un-pooled module against the oracle; the same arithmetic chain


# ------------------------------------------------------------------------------------------------------------------ the plan
def _on(monkeypatch, A, mode="mean", min_tokens=64):
    monkeypatch.setattr(A, "SATTN_KV_POOL", mode)
    monkeypatch.setattr(A, "SATTN_KV_POOL_MIN_TOKENS", min_tokens)


def test_kv_pool_plan(monkeypatch):
    from viewcrafter_amd.lvdm.modules import attention as A
    assert A.SATTN_KV_POOL is None and A.SATTN_KV_POOL_MIN_TOKENS == 4096, "off by default; 4096 tokens a frame by default"
    assert A.kv_pool_plan(72, 128, 320) is None and A.kv_pool_plan(16, 32, 64) is None, "off: nothing pools"
    for mode in ("mean", "nearest"):
        _on(monkeypatch, A, mode)
        table = {(7, 12): None, (8, 11): None,              # odd H, odd W
                 (6, 10): None,                            # 15 pooled tokens: not a multiple of 8
                 (6, 8): None,                             # 48 tokens: below the threshold of 64 (and 12 pooled)
                 (8, 12): (4, 6), (16, 32): (8, 16), (8, 8): (4, 4)}
        for (H, W), want in table.items():
            assert A.kv_pool_plan(H, W, 64) == want, (mode, H, W)
        assert A.kv_pool_plan(8, 12, 60) is None and A.kv_pool_plan(8, 12, 8200) is None, "the library's predicate: C % 8, C <= 8192"
        monkeypatch.setattr(A, "SATTN_KV_POOL_MIN_TOKENS", 97)
        assert A.kv_pool_plan(8, 12, 64) is None and A.kv_pool_plan(16, 32, 64) == (8, 16), "below / above the threshold"
        # the shipped default at the two shipped sizes: level 0 of 576x1024 only
        monkeypatch.setattr(A, "SATTN_KV_POOL_MIN_TOKENS", 4096)
        assert [A.kv_pool_plan(72 >> l, 128 >> l, 320 << min(l, 2)) for l in range(4)] == [(36, 64), None, None, None]
        assert [A.kv_pool_plan(40 >> l, 64 >> l, 320 << min(l, 2)) for l in range(4)] == [None] * 4
        monkeypatch.setattr(A, "SATTN_KV_POOL_MIN_TOKENS", 2048)
        assert [A.kv_pool_plan(72 >> l, 128 >> l, 320 << min(l, 2)) for l in range(4)] == [(36, 64), (18, 32), None, None]
        assert [A.kv_pool_plan(40 >> l, 64 >> l, 320 << min(l, 2)) for l in range(4)] == [(20, 32), None, None, None]


def test_env_values():
    from viewcrafter_amd.lvdm.modules import attention as A
    assert A._parse_kv_pool("0") is None and A._parse_kv_pool("") is None
    assert A._parse_kv_pool("mean") == "mean" and A._parse_kv_pool("nearest") == "nearest"
    for bad in ("1", "avg", "Mean"):
        with pytest.raises(ValueError, match="0 .off., mean or nearest"):
            A._parse_kv_pool(bad)
    # ... and at import, where the environment is read
    env = dict(os.environ, VCX_SATTN_KV_POOL="max")
    r = subprocess.run([sys.executable, "-c", "import viewcrafter_amd.lvdm.modules.attention"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "VCX_SATTN_KV_POOL='max'" in r.stderr and "mean or nearest" in r.stderr


# ------------------------------------------------------------------------------------------------------------------ host graph
class _PoolRecorder(_Recorder):
    """tests/test_mxfp8_sattn_cpu._Recorder plus the pooled operand; the attention and the transposed projection also record their pitches."""

    NAMES = _Recorder.NAMES + ("layer_norm_pool2x2",)

    def layer_norm_pool2x2(self, x, gamma, beta, eps, n, H, W, mode):
        assert gamma.dtype == beta.dtype == torch.float32 and isinstance(eps, float)
        self.calls.append(("layer_norm_pool2x2", tuple(x.shape), n, H, W, mode))
        return torch.zeros((n * (H // 2) * (W // 2), x.shape[1]), dtype=torch.float16)

    def gemm(self, a, w, *, M, N, **kw):
        self.calls.append(("gemm", (M, N), kw["K"], kw["lda"], tuple(a.shape), tuple(w.shape)))
        return torch.zeros((M, N), dtype=torch.float16)

    def linear(self, x, w, bias=None, **kw):
        out = super().linear(x, w, bias, **kw)
        self.calls[-1] = self.calls[-1] + (kw.get("alpha", 1.0), bias is not None)
        return out

    def flash_attn(self, q, k, vt, out, **kw):
        self.calls.append(("flash_attn", kw["nq"], kw["nk"], kw["log2_logits"], kw["n_groups"], kw["heads"], kw["kv_rows"], kw["kv_div"], kw["ldq"], kw["ldk"],
                           kw["ldvt"], kw["ldo"], tuple(q.shape), tuple(k.shape), tuple(vt.shape)))
        return out


def _pool_packs(st):
    return [blk.attn1._pk["kv_pool"] for blk in st.transformer_blocks if blk.attn1._pk is not None and "kv_pool" in blk.attn1._pk]


# What the commit before the switch existed records for _transformer(1) on _x(8, 8, 12) with an image context (tests/test_mxfp8_sattn_cpu._Recorder):
# norm, proj_in, [statistics, q|k, V^T, attention, to_out], [statistics, q, dual attention, to_out], LayerNorm + GEGLU, [ff.2 | proj_out] ...
TODAY_8x12 = [("group_norm", (8, 96, 64)), ("linear", (768, 64, 64), False, False, False), ("row_stats",), ("linear", (768, 128, 64), False, False, True),
              ("gemm", (64, 768)), ("flash_attn", 96, 96, True), ("linear", (768, 64, 64), True, False, False), ("row_stats",),
              ("linear", (768, 64, 64), False, False, True), ("flash_attn_dual", 96, 77, 16), ("linear", (768, 64, 64), True, False, False),
              ("layer_norm", (768, 64)), ("linear", (768, 512, 64), False, False, False), ("linear", (768, 64, 256), True, False, False),
              ("linear", (768, 64, 64), True, False, False)]


def test_switch_off_makes_the_calls_it_makes_today_and_builds_no_pooled_pack(monkeypatch):
    A, st = _transformer()
    assert A.SATTN_KV_POOL is None
    with monkeypatch.context() as mp:
        rec = _Recorder(mp)
        with torch.no_grad():
            y, _ = st(_x(2 * FPV, 8, 12), context_kv=_context(A, st, 2), frames_per_video=FPV)
    assert rec.calls == TODAY_8x12
    assert _pool_packs(st) == [] and "layer_norm_pool2x2" not in rec.names(skip=()) and y.shape == (2 * FPV, 8, 12, C)
    # MIN_TOKENS alone switches nothing on
    monkeypatch.setattr(A, "SATTN_KV_POOL_MIN_TOKENS", 1)
    assert _fp16_run(monkeypatch, st, _context(A, st, 2), _x(2 * FPV, 8, 12)) == [c[0] for c in TODAY_8x12] and _pool_packs(st) == []


def _self_attention_calls(A, ops, st, frames, H, W, have_rs=False):
    """The calls section 2 of the issue lists for the pooled self-attention of one block, as _PoolRecorder records them."""
    tokens, N, Np = frames * H * W, H * W, (H // 2) * (W // 2)
    alpha = (st.transformer_blocks[0].attn1.scale * ops.LOG2E) ** 0.5
    folded = ops.lnfold_ok(tokens, C, C, lda=C)          # C = 64: the packs are folded; the library says whether the kernel takes the rows
    q = ([] if have_rs else [("row_stats",)]) + [("linear", (tokens, C, C), False, False, True, alpha, True)] if folded else \
        [("layer_norm", (tokens, C)), ("linear", (tokens, C, C), False, False, False, alpha, False)]
    return q + [("layer_norm_pool2x2", (tokens, C), frames, H, W, A._KV_POOL_MODES[A.SATTN_KV_POOL]),
                ("linear", (frames * Np, C, C), False, False, False, alpha, False),
                ("gemm", (C, frames * Np), C, C, (C, C), (frames * Np, C)),
                ("flash_attn", N, Np, True, frames, 1, Np, 1, C, C, frames * Np, C, (tokens, C), (frames * Np, C), (C, frames * Np))]


@pytest.mark.parametrize("mode", ["mean", "nearest"])
@pytest.mark.parametrize("depth", [1, 2])
def test_switch_on_runs_the_listed_calls_per_block(monkeypatch, depth, mode):
    from viewcrafter_amd import ops
    A, st = _transformer(depth)
    kv, x = _context(A, st, 2), _x(2 * FPV, 8, 12)
    with monkeypatch.context() as mp:
        rec0 = _PoolRecorder(mp)
        with torch.no_grad():
            st(x, context_kv=kv, frames_per_video=FPV)
    today = rec0.calls
    _on(monkeypatch, A, mode)
    rec = _PoolRecorder(monkeypatch)
    with torch.no_grad():
        y, cs = st(x, context_kv=kv, frames_per_video=FPV)
    calls = rec.calls
    assert calls[:2] == today[:2] and [c[0] for c in calls[:2]] == ["group_norm", "linear"], "norm and proj_in are today's"
    want = _self_attention_calls(A, ops, st, 2 * FPV, 8, 12)
    i = j = 2
    for b in range(depth):
        assert calls[i:i + len(want)] == want, f"block {b}: {calls[i:i + len(want)]}"
        i += len(want)
        j += [c[0] for c in today[j:]].index("flash_attn") + 1
        # to_out, the cross-attention, the feed-forward (between blocks) run exactly as today: up to the next block's self-attention
        nxt = [c[0] for c in today[j:]].index("flash_attn") - 3 if b + 1 < depth else len(today) - j
        assert calls[i:i + nxt] == today[j:j + nxt], f"block {b}: behind the self-attention"
        i, j = i + nxt, j + nxt
    assert i == len(calls) and j == len(today)
    assert y.shape == (2 * FPV, 8, 12, C) and cs is None
    # the packs: Q folded as today's Q|K pack is, carrying the same factor; plain K and V weights; built once, dropped with the pack
    packs = _pool_packs(st)
    assert len(packs) == depth
    a1 = st.transformer_blocks[0].attn1
    qk, pq = a1._pk["qk"], packs[0]["q"]
    assert pq["colsum"] is not None and torch.equal(pq["w"], qk["w"][:C]) and torch.equal(pq["colsum"], qk["colsum"][:C]) and torch.equal(pq["bias"], qk["bias"][:C])
    assert torch.equal(packs[0]["wk"], a1.to_k.weight.detach().half()) and torch.equal(packs[0]["wv"], a1.to_v.weight.detach().half())
    assert packs[0]["wk"].dtype == packs[0]["wv"].dtype == torch.float16
    with torch.no_grad():
        st(x, context_kv=kv, frames_per_video=FPV)
    assert all(a is b for a, b in zip(_pool_packs(st), packs))
    st.load_state_dict(st.state_dict())
    assert _pool_packs(st) == [], "loading a state dict drops the pooled packs with the fp16 packs"


def test_cfg_repeat_and_text_only_context(monkeypatch):
    from viewcrafter_amd import ops
    A, st = _transformer(2)
    _on(monkeypatch, A)
    rec = _PoolRecorder(monkeypatch)
    # the shared CFG prefix: block 0's pooled self-attention runs once on the FPV shared frames, the replication stays in front of the
    # cross-attention, block 1 runs on the replicated rows
    with torch.no_grad():
        y, _ = st(_x(FPV, 16, 32), context_kv=_context(A, st, 2), frames_per_video=FPV, cfg_repeat=2)
    names = rec.names()
    want0, want1 = _self_attention_calls(A, ops, st, FPV, 16, 32), _self_attention_calls(A, ops, st, 2 * FPV, 16, 32)
    assert rec.calls[2:2 + len(want0)] == want0
    r = names.index("repeat_rows")
    assert names[r:r + 4] == ["repeat_rows"] * 3 + ["flash_attn_dual"] and names.count("repeat_rows") == 3
    second = [i for i, c in enumerate(rec.calls) if c[0] == "layer_norm_pool2x2"][1]
    k = second - [c[0] for c in want1].index("layer_norm_pool2x2")
    assert rec.calls[k:k + len(want1)] == want1 and k > r
    assert y.shape == (2 * FPV, 16, 32, C)
    assert [c[1:3] for c in rec.calls if c[0] == "flash_attn"] == [(512, 128), (512, 128)]
    # no image context: the cross-attention is the single-set entry, keys shared by the frames of a video, untouched by the switch
    rec.calls.clear()
    with torch.no_grad():
        st(_x(2 * FPV, 8, 12), context_kv=_context(A, st, 2, image=False), frames_per_video=FPV)
    fa = [c for c in rec.calls if c[0] == "flash_attn"]
    assert [(c[1], c[2], c[6], c[7]) for c in fa] == [(96, 24, 24, 1), (96, 77, 80, FPV)] * 2
    assert "flash_attn_dual" not in rec.names()


@pytest.mark.parametrize("why,H,W", [("pooled count 12", 6, 8), ("padded tokens", 6, 10), ("below the threshold", 8, 12), ("predicate", 8, 12)])
def test_a_refused_geometry_keeps_todays_calls_and_builds_no_pack(monkeypatch, why, H, W):
    from viewcrafter_amd import ops
    A, st = _transformer()
    kv, x = _context(A, st, 2), _x(2 * FPV, H, W)
    today = _fp16_run(monkeypatch, st, kv, x)
    _on(monkeypatch, A, min_tokens=97 if why == "below the threshold" else 1)
    if why == "predicate":
        monkeypatch.setattr(ops, "layer_norm_pool2x2_ok", lambda *a: False)
    rec = _PoolRecorder(monkeypatch)
    with torch.no_grad():
        y, _ = st(x, context_kv=kv, frames_per_video=FPV)
    assert rec.names(skip=()) == today, "a refusal keeps today's calls, all of them"
    assert _pool_packs(st) == [] and y.shape == x.shape


def test_with_sattn_mxfp8_the_eligible_call_pools_and_the_others_keep_mx(monkeypatch):
    A, st = _transformer()
    kv = _context(A, st, 2)
    monkeypatch.setattr(A, "SATTN_MXFP8", True)
    monkeypatch.setattr(A, "SATTN_MXFP8_SKIP_DIMS", frozenset())
    _on(monkeypatch, A, min_tokens=96)
    today = [c[0] for c in TODAY_8x12]
    rec = _PoolRecorder(monkeypatch)
    with torch.no_grad():
        st(_x(2 * FPV, 8, 12), context_kv=kv, frames_per_video=FPV)           # 96 tokens: pools
    names = rec.names(skip=())
    assert not any("mxfp8" in n for n in names), "neither an MX op nor an MX predicate: a pooled call asks none"
    plan = st._plan(_x(2 * FPV, 8, 12), kv, FPV, 1)
    assert plan.engine == "pool" and plan.pool == (4, 6)
    assert names[2:8] == ["row_stats", "linear", "layer_norm_pool2x2", "linear", "gemm", "flash_attn"] and names[8:] == today[6:]
    rec.calls.clear()
    with torch.no_grad():
        st(_x(2 * FPV, 6, 8), context_kv=kv, frames_per_video=FPV)            # 48 tokens: below the threshold, the MX route as without the switch
    assert rec.names()[2:11] == _block_mx() and "layer_norm_pool2x2" not in rec.names()
    assert [blk.attn1._pk.get("mx") is not None for blk in st.transformer_blocks] == [True]


# ------------------------------------------------------------------------------------------------------------------ numerics on the stand-ins
CDIM = 128


@pytest.fixture(scope="module")
def synth_transformer():
    from viewcrafter_amd.lvdm.modules import attention as A
    st = A.SpatialTransformer(C, 1, 64, depth=1, context_dim=CDIM, use_checkpoint=False, use_linear=True, image_cross_attention=True).eval()
    sd = {"st." + k: v for k, v in load_synth(st).items()}
    return A, st, sd


def transformer_inputs(H, W, fpv=2, videos=2, width=C):
    """(x fp16 [n, H, W, C] channels-last, the module's context dict, the oracle's x [n, C, H, W] and per-frame context) from one draw"""
    n = fpv * videos
    x16 = synth_input(f"kvpool_x_{H}x{W}", (n, width, H, W)).permute(0, 2, 3, 1).contiguous().half()
    ctx = synth_input(f"kvpool_ctx_{H}x{W}", (videos, 77 + N_IMG, CDIM))
    txt = torch.zeros((videos, 80, CDIM), dtype=torch.float16)
    txt[:, :77] = ctx[:, :77].half()
    img = ctx[:, 77:].half().reshape(videos * N_IMG, CDIM).contiguous()
    ctx_o = torch.cat([txt[:, :77].float(), img.view(videos, N_IMG, CDIM).float()], 1).repeat_interleave(fpv, 0)
    return x16, dict(txt=txt.view(-1, CDIM), img=img, n_img=N_IMG, per_frame=False), x16.float().permute(0, 3, 1, 2), ctx_o


@pytest.mark.parametrize("mode", ["mean", "nearest"])
@pytest.mark.parametrize("H,W", [(16, 32), (8, 12)])
def test_module_on_the_stand_ins_against_the_pooled_reference(monkeypatch, synth_transformer, H, W, mode):
    A, st, sd = synth_transformer
    CKP.install(monkeypatch)
    x16, ctx, xo, ctx_o = transformer_inputs(H, W)
    plain = O.spatial_transformer(sd, "st", xo, ctx_o, 1)
    _on(monkeypatch, A, mode)
    ref = REF.spatial_transformer(sd, "st", xo, ctx_o, 1)
    with torch.no_grad():
        y, _ = st(x16, context_kv=st.project_context(ctx), frames_per_video=2)
    e, apart = rel_l2(y.float().permute(0, 3, 1, 2), ref), rel_l2(ref, plain)
    print(f"\n[kv-pool] SpatialTransformer({C}, {H}x{W}, {mode}) on the CPU stand-ins: rel-L2 vs the pooled reference = {e:.3e}; the pooled and the "
          f"un-pooled reference are {apart:.3e} apart")
    assert apart >= 10 * UNET_TOL, "the two references must be far enough apart for the comparison to show which one the module computes"
    assert e <= UNET_TOL


# ------------------------------------------------------------------------------------------------------------------ the stand-in, the launcher
def test_the_stand_in_is_the_composition_of_the_existing_stand_ins():
    g = torch.Generator().manual_seed(11)
    n, H, W, Cc = 3, 4, 6, 64
    x = (torch.randn((n * H * W, Cc), generator=g) * 1.5 + 0.3).half()
    gamma, beta = 1.0 + 0.2 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    a = CK.layer_norm(x, gamma, beta, 1e-5)
    mean = CKP.layer_norm_pool2x2(x, gamma, beta, 1e-5, n, H, W, CKP.POOL_MEAN)
    near = CKP.layer_norm_pool2x2(x, gamma, beta, 1e-5, n, H, W, CKP.POOL_NEAREST)
    assert mean.shape == near.shape == (n * 6, Cc) and mean.dtype == near.dtype == torch.float16 and mean.is_contiguous() and near.is_contiguous()
    assert torch.equal(mean, CK.avgpool2x2(a.view(n, H, W, Cc)).reshape(-1, Cc))
    rows = [(f * H + 2 * y) * W + 2 * xx for f in range(n) for y in range(H // 2) for xx in range(W // 2)]
    assert torch.equal(near, a[rows])
    w4 = a.view(n, H // 2, 2, W // 2, 2, Cc).float()
    assert torch.equal(mean.view(n, H // 2, W // 2, Cc), ((w4[:, :, 0, :, 0] + w4[:, :, 0, :, 1] + w4[:, :, 1, :, 0] + w4[:, :, 1, :, 1]) * 0.25).half())


def test_the_predicate_and_the_launcher_refuse_before_any_launch():
    from viewcrafter_amd import ops
    L = _lib.lib()
    assert (ops.POOL_MEAN, ops.POOL_NEAREST) == (0, 1)
    ok = lambda n=50, H=72, W=128, Cc=320, mode=0: L.vcx_layernorm_pool2x2_ok(n, H, W, Cc, mode)
    assert ok() == 1 and ok(mode=1) == 1 and ok(n=1, H=2, W=2, Cc=8) == 1 and ok(Cc=8192) == 1
    for kw, text in ((dict(H=71), b"even"), (dict(W=127), b"even"), (dict(Cc=324), b"C % 8"), (dict(Cc=8200), b"8192"), (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
                     (dict(n=0), b"> 0"), (dict(n=1 << 17, H=128, W=128), b"2^31")):
        assert ok(**kw) == 0 and text in L.vcx_last_error(), (kw, L.vcx_last_error())
    assert ok(n=(1 << 17) - 1, H=128, W=128) == 1
    assert ops.layer_norm_pool2x2_ok(50, 72, 128, 320, ops.POOL_MEAN) is True and ops.layer_norm_pool2x2_ok(50, 72, 127, 320, ops.POOL_MEAN) is False
    FAKE, EINVAL = 1 << 20, -1
    run = lambda x=FAKE, y=FAKE, g=FAKE, b=FAKE, n=2, H=4, W=6, Cc=64, mode=0: L.vcx_layernorm_pool2x2_f16(x, y, g, b, n, H, W, Cc, 1e-5, mode, None)
    for name in ("x", "y", "g", "b"):
        assert run(**{name: None}) == EINVAL and b"null" in L.vcx_last_error(), name
        assert run(**{name: FAKE + 8}) == EINVAL and b"aligned" in L.vcx_last_error(), name
    for kw in (dict(H=5), dict(W=7), dict(Cc=68), dict(Cc=8200), dict(mode=2), dict(n=1 << 17, H=128, W=128)):
        assert run(**kw) == EINVAL and b"vcx_layernorm_pool2x2_f16" in L.vcx_last_error(), kw


def test_the_extension_header_the_library_and_the_binding_agree():
    """include/vcx_pool.h is additive: its functions are exactly _lib.EXT_SYMBOLS, the library exports them with the declared argument
    counts, none of them is in include/vcx.h or _lib.SYMBOLS, and the ABI number is vcx.h's own."""
    import re
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)
    ext, base = strip("vcx_pool.h"), strip("vcx.h")
    declared = set(re.findall(r"\b(vcx_[a-z0-9_]+)\s*\(", ext))
    assert declared == set(_lib.EXT_SYMBOLS) == {"vcx_layernorm_pool2x2_f16", "vcx_layernorm_pool2x2_ok"}
    assert not declared & set(_lib.SYMBOLS) and not declared & set(re.findall(r"\b(vcx_[a-z0-9_]+)\s*\(", base))
    assert '#include "vcx.h"' in ext and "VCX_ABI_VERSION" not in ext
    L = _lib.lib()
    for name, nargs in (("vcx_layernorm_pool2x2_f16", 11), ("vcx_layernorm_pool2x2_ok", 5)):
        fn = getattr(L, name)
        decl = re.search(r"int " + name + r"\((.*?)\);", ext, re.S).group(1)
        assert len(fn.argtypes) == nargs == len(decl.split(",")) and fn.restype is ctypes.c_int
    assert int(re.search(r"#define VCX_POOL_MEAN (\d)", ext).group(1)) == 0 and int(re.search(r"#define VCX_POOL_NEAREST (\d)", ext).group(1)) == 1
    assert L.vcx_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define VCX_ABI_VERSION (\d+)", base).group(1))
