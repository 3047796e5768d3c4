"""Transformer blocks of the lvdm UNet on the gfx950 kernels.

Mirrors the classes of the reference's lvdm/modules/attention.py that the ViewCrafter graph instantiates
(CrossAttention, FeedForward/GEGLU, BasicTransformerBlock, SpatialTransformer, TemporalTransformer) with identical
constructor arguments and parameter names/shapes, so reference checkpoints load with strict=True.  The parameters are
held in stock nn.Linear / nn.LayerNorm / nn.GroupNorm containers; `forward` never calls them — it runs the packed
fp16 copies through libvcx (no PyTorch fallback).

Activations are channels-last fp16.  A spatial transformer sees tokens [(b t h w), C]; a temporal transformer sees the
SAME row order (Linear/LayerNorm are row-wise, so no '(b t) c h w <-> (b h w) t c' copies are needed — only the
temporal attention kernel itself walks frames with a stride of h*w rows).
"""
import math
import os
from collections import namedtuple

import torch
from torch import nn

from ... import ops
from ...packing import fold_layernorm, pack_ff_out_folded, pack_geglu, pack_mxfp8
from ..common import default
from .flow import GN_STATS_LEVEL, env_dims, out_kwargs


def _f16(t):
    return t.detach().to(torch.float16).contiguous()


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


# nn.LayerNorm -> nn.Linear pairs of BasicTransformerBlock run as row statistics + ONE projection of the un-normalised token rows
# (VCX_GEMM_LNFOLD, include/vcx.h): the normalised copy of the token stream is neither written nor re-read.  Needs the DMA GEMM
# kernel (channel count % 64 == 0); VCX_LN_FOLD=0 keeps the separate LayerNorm kernel (A/B runs, tools/lnfold_ab.py).
FOLD_LAYERNORM = os.environ.get("VCX_LN_FOLD", "1") != "0"
# ... in front of the GEGLU projection too, from C = 640 up (round 6): there the projection runs on the tiled engine either way and the fold
# replaces a read + write pass over the token stream by a statistics pass (same box, tools/step_ab.py lnff = 0 / 2 / 1, profiles/r06s_lnff_ab.txt:
# LayerNorm family 3.14 -> 2.67 ms at no GEMM cost, step -0.45 ms).  NOT at C = 320: the level-0 projection would leave the weight-stationary
# GEGLU kernel for the tiled engine's folded epilogue, whose two extra multiply-adds per output pair cost more than the pass they save (fold
# everywhere: GEMM +1.0 ms, step level; round 3: profiles/r03_experiments.md section 8).  VCX_LN_FOLD_FF=0: never; VCX_LN_FOLD_FF_MIN_DIM: the width.
FOLD_LAYERNORM_FF = os.environ.get("VCX_LN_FOLD_FF", "1") != "0"
FOLD_LAYERNORM_FF_MIN_DIM = int(os.environ.get("VCX_LN_FOLD_FF_MIN_DIM", "640"))
# Opt-in (VCX_FF_MXFP8=1, default off): the two linears of the GEGLU feed-forward on the block-scaled MXFP8 matrix pipe (include/vcx.h "MXFP8
# operands", csrc/gemm_mx.hip) - LayerNorm + quantiser in one pass, GEGLU projection with MXFP8 output, ff.2 with bias and residual reading
# those bytes.  The LayerNorm is APPLIED, not folded: quantising the raw stream and subtracting mean x colsum afterwards would amplify
# the quantisation error.  Accuracy with a real checkpoint is unmeasured; what was measured is in profiles/mxfp8_ff.md.  Off: no new
# launch, no new allocation, every output bit as before.
FF_MXFP8 = os.environ.get("VCX_FF_MXFP8", "0") == "1"
# Widths whose feed-forward stays on the fp16 route although the switch is on.  320 (level 0) by default: isolated, its GEGLU projection is
# slower in MXFP8 than on the weight-stationary fp16 kernel (1.08 against 0.98 ms at 460800 rows; the pair 1.49 against 1.45 ms), while
# the 640- and 1280-wide pairs are 1.25x / 1.29x faster (profiles/mxfp8_ff.md).  VCX_FF_MXFP8_SKIP_DIMS="" puts every width on MX.
FF_MXFP8_SKIP_DIMS = env_dims("VCX_FF_MXFP8_SKIP_DIMS", "320")
# Opt-in (VCX_TATTN_MXFP8=1, default off): the two self-attentions of every block of a TemporalTransformer on the MXFP8 matrix pipe -
# LayerNorm + quantiser in one pass, the q|k|v projection reading those bytes (un-folded weights, a zero bias: the reference has none),
# the temporal attention kernel writing MXFP8 bytes + scales itself (vcx_attn_temporal_d64_mxfp8: a head's 64 columns are two MX blocks
# held by one wave, so no quantiser pass), to_out with bias and residual reading them.  T <= 32, no relative position; any refusal keeps
# the fp16 calls for the whole transformer.  (The spatial transformer: SATTN_MXFP8 below.)  Accuracy with a real checkpoint is unmeasured; what was
# measured is in profiles/mxfp8_tattn.md.  Off: no new launch, no new allocation, every output bit as before.
TATTN_MXFP8 = os.environ.get("VCX_TATTN_MXFP8", "0") == "1"
# Widths whose temporal attentions stay on the fp16 route although the switch is on: those whose isolated MX layer is not faster than
# its fp16 layer by more than the fp16 layer's own spread on the same box.  320 by default: its MX layer is 0.80x of the fp16 one (Kp = 384
# pads a sixth of K, N = 320 half-fills the third column tile), 640 / 1280 are 1.05x / 1.26x against a spread of 0.5 % (profiles/mxfp8_tattn.md).
# VCX_TATTN_MXFP8_SKIP_DIMS="" puts every width on MX.
TATTN_MXFP8_SKIP_DIMS = env_dims("VCX_TATTN_MXFP8_SKIP_DIMS", "320")
# Opt-in (VCX_SATTN_MXFP8=1, default off; independent of the other four switches): the attention projections of every block of a
# SpatialTransformer on the MXFP8 matrix pipe - LayerNorm + quantiser in one pass in front of q|k, V^T (vcx_gemm_mxfp8 with its operands
# swapped: ops.linear_t_mxfp8) and the cross-attention's query projection, un-folded weights carrying the base-2 logit scale; the three
# spatial attention kernels write MXFP8 bytes + scales themselves (vcx_attn_flash_d64_mxfp8 / vcx_attn_flash_dual_d64_mxfp8: the fp16
# kernels with a quantising store tail, so no quantiser pass), and both to_out layers read them, with bias and residual.  The context
# K / V (cached per video), proj_in and the feed-forward + proj_out keep their code; no row-statistics buffers are requested.  Any
# refusal keeps the fp16 calls for the whole transformer.  Accuracy with a real checkpoint is unmeasured; what was measured is in
# profiles/mxfp8_sattn.md.  Off: no new launch, no new allocation, every output bit as before.
SATTN_MXFP8 = os.environ.get("VCX_SATTN_MXFP8", "0") == "1"
# Widths whose spatial attentions stay on the fp16 route although the switch is on, by the rule of profiles/mxfp8_tattn.md: a width stays on
# fp16 unless its isolated MX layer beats the fp16 layer by more than the fp16 layer's own spread in the same run.  320 by default: the two
# attentions of a 320-wide block are 0.94x of fp16 on MX (Kp = 384 pads a sixth of K; to_out 0.74x, q|k 0.91x), 640 / 1280 are 1.04x / 1.15x
# against a spread of 0.2 - 0.7 % (profiles/mxfp8_sattn.md).  VCX_SATTN_MXFP8_SKIP_DIMS="" puts every width on MX.
SATTN_MXFP8_SKIP_DIMS = env_dims("VCX_SATTN_MXFP8_SKIP_DIMS", "320")
# Opt-in (VCX_SATTN_KV_POOL=mean | nearest, default off): the spatial self-attention keeps every query but takes its keys and values from
# the 2x2-pooled token grid of the frame (token downsampling: "ToDo", Smith et al. 2024; the spatial-reduction attention of PVT; training-
# free) - a quarter of the key tiles, K and V^T projected from a quarter of the rows.  The pooled operand is LayerNorm + pool in one pass
# (vcx_layernorm_pool2x2_f16: the mean of the window, or its row (2y, 2x)); Q is its own folded projection, K and V^T plain projections
# of the pooled rows; the attention kernel is the fp16 flash kernel with nq = 4 nk.  Which calls pool: kv_pool_plan.  An approximation:
# accuracy with a real checkpoint is unmeasured; what was measured is in profiles/sattn_kv_pool.md.  Off: no new launch, no new
# allocation, every output bit as before.
_KV_POOL_MODES = {"mean": ops.POOL_MEAN, "nearest": ops.POOL_NEAREST}


def _parse_kv_pool(value):
    if value in ("", "0"):
        return None
    if value not in _KV_POOL_MODES:
        raise ValueError(f"VCX_SATTN_KV_POOL={value!r}: expected 0 (off), mean or nearest")
    return value


SATTN_KV_POOL = _parse_kv_pool(os.environ.get("VCX_SATTN_KV_POOL", "0"))
# Frames with fewer tokens keep the un-pooled attention.  4096: level 0 of 576x1024 (9216 tokens a frame) pools, its deeper levels (2304,
# 576, 144) and every level of 320x512 (2560 at most) do not, until this is lowered.
SATTN_KV_POOL_MIN_TOKENS = int(os.environ.get("VCX_SATTN_KV_POOL_MIN_TOKENS", "4096"))


def kv_pool_plan(H, W, C):
    """SATTN_KV_POOL: the pooled token grid (H/2, W/2) the self-attention of a SpatialTransformer over H x W tokens of C channels a frame
    takes its keys and values from, or None: the call keeps today's route.  From ONE frame's geometry only - a frame's route must not
    depend on the batch it runs in (B = 2 against two B = 1, the shared CFG prefix against the replicated batch).  Pools iff the switch is
    on, H and W are even, the frame has at least SATTN_KV_POOL_MIN_TOKENS tokens, the pooled count is a multiple of 8 (the attention
    kernels address a frame's keys at 16-byte granularity; it makes H W a multiple of 8 too: no padded rows) and the library takes it."""
    if SATTN_KV_POOL is None or H % 2 or W % 2 or H * W < SATTN_KV_POOL_MIN_TOKENS or (H // 2) * (W // 2) % 8:
        return None
    if not ops.layer_norm_pool2x2_ok(1, H, W, C, _KV_POOL_MODES[SATTN_KV_POOL]):
        return None
    return H // 2, W // 2

# A transformer's last two linear layers - ff.net[2] + block residual, then proj_out + transformer residual - have nothing between them
# and the token stream between them has no other reader (depth 1; proj_out follows the last block), so they run as ONE GEMM over
# K = 4D + D: weights [Wout W2 | Wout] combined at pack time (packing.pack_ff_out_folded), the GEGLU output g as the A operand and the
# token stream t as its K tail (include/vcx.h tail_a0; ops.linear_tail_ok).  The write and re-read of the feed-forward's output, one
# launch and one fp16 rounding disappear; the result agrees with the two-step form to fp16 rounding, not bit for bit.  On the GPU only
# (CPU / meta tensors keep the two calls), fp16 feed-forward route only.  VCX_FF_OUT_FOLD=0: two calls everywhere (A/B runs,
# tools/step_ab.py); VCX_FF_OUT_FOLD_SKIP_DIMS: widths that keep two calls.  1280 by default: isolated at the benchmark's rows the merged call
# is 13 % / 9 % faster than the pair at D = 320 / 640, but at D = 1280 (K = 6400, compute-bound either way) its 2-5 % lies inside the pair's
# own round-to-round spread, and the step is level with those twelve transformers folded or not (profiles/ff_out_fold.md).
FF_OUT_FOLD = os.environ.get("VCX_FF_OUT_FOLD", "1") != "0"
FF_OUT_FOLD_SKIP_DIMS = env_dims("VCX_FF_OUT_FOLD_SKIP_DIMS", "1280")


# TemporalTransformer.norm -> proj_in (reference attention.py:331-336,369-372) and SpatialTransformer.norm -> proj_in (:265-269,299):
# a GroupNorm without SiLU in front of a linear layer is an affine map per (statistics unit, channel), so it runs as per-unit scaled
# weights and bias of the projection (vcx_groupnorm_fold_linear_f16 + vcx_gemm_units_f16 on the UN-normalised rows) and the normalised
# copy of the tensor is neither written nor re-read.  All units of a call run under ONE tile plan wherever ops.units_one_launch_ok holds: the
# weight-stationary kernel at C = 320, the tiled engine's per-unit form at the other widths (at most two launches, tiles counted per unit;
# the same bits as the unit-by-unit loop it replaced).  Temporal norms (unit = video): wherever a video's tensor is at least
# GN_FOLD_MIN_BYTES - a per-video size floor from the time when every video was a launch of its own, kept so that the default host graph
# and its rounding stay what they were.  Spatial norms (unit = frame, 50 of them): by default only at C = 320, level 0 of the UNet (the
# weight-stationary kernel, whose blocks keep a weight set in registers anyway).  VCX_GN_FOLD_SPATIAL=2 (opt-in) folds them at every width
# where the frames of a video go through the per-unit form; the fold agrees with norm-then-linear to fp16 rounding, not bit for bit,
# which is why the default stays.  VCX_GN_FOLD=0: the separate apply pass everywhere (A/B runs, tools/step_ab.py).
GN_FOLD = os.environ.get("VCX_GN_FOLD", "1") != "0"
GN_FOLD_MIN_BYTES = int(os.environ.get("VCX_GN_FOLD_MIN_BYTES", str(16 << 20)))
GN_FOLD_SPATIAL = {"0": 0, "2": 2}.get(os.environ.get("VCX_GN_FOLD_SPATIAL", "1"), 1)      # 0: never, 1: C = 320 only, 2: every width with a one-plan route


def spatial_fold_ok(n, pixels, C, D):
    """Does vcx_gemm_units_f16 take the frames of a video, n frames of `pixels` rows, in ONE weight-stationary launch (csrc/gemm.hip)?
    Decided per VIDEO (n = frames per video, not frames per call): a frame's bits must not depend on how many videos share the call
    (B = 2 against two B = 1, the shared CFG prefix against the replicated batch), so the size thresholds look at one video and the
    kernel's own M >= 8192 follows from them for every batch.  The caller checks the 4 GiB extents of the whole call (fold_extent_ok).
    GN_FOLD_SPATIAL == 2 (opt-in): also where the tiled engine's per-unit form takes the frames of a video (ops.units_route "grouped");
    that form and the unit-by-unit loop give the same bits, so there too a frame does not depend on the batch."""
    if (GN_FOLD and GN_FOLD_SPATIAL == 2 and n > 1 and pixels % 8 == 0 and 2 * n * pixels * C >= GN_FOLD_MIN_BYTES and fold_extent_ok(n * pixels, max(C, D))
            and ops.units_route(n * pixels, D, C, pixels) == "grouped"):
        return True
    return (GN_FOLD and GN_FOLD_SPATIAL and C == 320 and D == 320 and pixels % 32 == 0 and pixels >= 1024 and n * pixels >= 8192
            and 2 * n * pixels * C >= GN_FOLD_MIN_BYTES and fold_extent_ok(n * pixels, C) and ops.tune_get("GEMM_DMA") != 0
            and ops.tune_get("GEMM_WS") != 0 and ops.tune_get("GEMM_CFG") < 0)      # (a forced tile configuration means the tiled engine: ADVICE r5)


def fold_extent_ok(rows, C):
    """32-bit byte offsets of the one-launch vcx_gemm_units_f16 over `rows` rows of C channels (output up to 256 rows past the end)."""
    return 2 * (rows + 256) * C < 0xFFFF0000


def temporal_fold_ok(rows, C, D):
    """Does the norm of a TemporalTransformer run as per-video weights / bias of proj_in (vcx_gemm_units_f16, unit = the `rows` rows of a
    video)?  From ONE video's size, like spatial_fold_ok."""
    return GN_FOLD and C % 64 == 0 and 2 * rows * C >= GN_FOLD_MIN_BYTES and 2 * rows * max(C, D) < 0xFFFF0000 and ops.tune_get("GEMM_DMA") != 0


def _folded(pj, rows, K, lda, transposed=False):
    """Does this pack run as a folded projection (and so want row statistics)?  THE rule of _ln_operands: the pack is folded AND the
    kernel takes the shape."""
    return pj["colsum"] is not None and ops.lnfold_ok(rows, pj["w"].shape[0], K, lda=lda, transposed=transposed)


def _ln_projection(w, ln, alpha=1.0, bias=None):
    """Packed form of `Linear(w, bias)(LayerNorm(.)) * alpha` (alpha scales the product, not the layer's own bias): folded
    (w', colsum, bias') when `ln` is given, plain fp16 weights otherwise (colsum None: the caller normalises first).  A folded
    pack keeps what it needs to build the plain form on demand (`_plain`: shapes the folded kernel cannot take, ops.lnfold_ok)."""
    if ln is not None:
        wf, colsum, bias_f = fold_layernorm(w, ln.weight, ln.bias, None)
        bias_f = bias_f * alpha
        if bias is not None:
            bias_f = bias_f + bias.detach().float()
        return dict(w=wf, colsum=colsum, bias=bias_f.contiguous(), eps=ln.eps, _src=(w, bias), _plain=None)
    return dict(w=_f16(w), colsum=None, bias=None if bias is None else _f32(bias), eps=None)


def _plain_of(pj):
    """The un-folded fp16 weights (+ fp32 bias) of a folded pack, built once when a call cannot use the fold."""
    if pj["_plain"] is None:
        w, bias = pj["_src"]
        with torch.no_grad():
            pj["_plain"] = (_f16(w), None if bias is None else _f32(bias))
    return pj["_plain"]


def _ln_operands(t, pj, lnp, stats=None, transposed=False, plain=_plain_of):
    """What a projection of LayerNorm(t) by the pack pj (keys w / colsum / bias) runs on -> (rows, weights, bias, fold keywords): the
    un-normalised rows, the folded weights and ln_stats / ln_colsum where _folded says so; layer_norm(t), the plain weights (a folded
    pack's: plain(pj)) and no keywords otherwise.  lnp = (gamma, beta, eps); `stats` = row statistics of t when the caller has them."""
    if _folded(pj, t.shape[0], t.shape[1], t.stride(0), transposed):
        st = stats if stats is not None else ops.row_stats(t, lnp[2])
        return t, pj["w"], pj["bias"], dict(ln_stats=st, ln_colsum=pj["colsum"])
    w, bias = (pj["w"], pj["bias"]) if pj["colsum"] is None else plain(pj)
    return ops.layer_norm(t, *lnp), w, bias, {}


def ln_linear(t, pj, lnp, alpha=1.0, stats=None, **kw):
    """Linear(LayerNorm(t)) * alpha for a pack of _ln_projection: folded or layer_norm + plain projection, by _ln_operands."""
    a, w, bias, fold = _ln_operands(t, pj, lnp, stats)
    return ops.linear(a, w, bias, alpha=alpha, **fold, **kw)


def ln_linear_t(t, pj, lnp, stats=None):
    """The transposed projection out[D, tokens] = W LayerNorm(t)^T (V^T of the spatial self-attention), same rule as ln_linear."""
    tokens, K = t.shape
    a, w, bias, fold = _ln_operands(t, pj, lnp, stats, transposed=True)
    if fold:
        fold.update(ldw=t.stride(0), ln_t=True)
    return ops.gemm(w, a, M=w.shape[0], N=tokens, K=K, lda=K, bias=bias, bias_m=bias is not None, **fold)


def _sig(tensors):
    return tuple((p.data_ptr(), p._version) for p in tensors)


class PackedModule(nn.Module):
    """Base for modules that keep kernel-layout copies of their parameters in `self._pk` (built lazily on the first
    forward, dropped whenever parameters are moved/cast or a state dict is loaded).  A pack that embeds parameters of ANOTHER
    module (the folded LayerNorm of the owning BasicTransformerBlock, `_pre_norm`) also remembers their identity and version
    counter and is rebuilt when either changes - `blk.norm1.load_state_dict(...)`, `.data` assignment or in-place edits of the
    norm no longer leave stale folded weights behind."""

    def __init__(self):
        super().__init__()
        self._pk = None
        self._pk_sig = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._drop_packed())

    def _drop_packed(self):
        self._pk = None

    def _apply(self, fn, recurse=True):
        self._pk = None
        return super()._apply(fn, recurse)

    def _foreign_params(self):
        pre = getattr(self, "_pre_norm", None)
        return [pre[0].weight, pre[0].bias] if pre else []

    def packed(self):
        foreign = self._foreign_params()
        if self._pk is not None and foreign and _sig(foreign) != self._pk_sig:
            self._pk = None
        if self._pk is None:
            with torch.no_grad():
                self._pk = self._pack()
            self._pk_sig = _sig(foreign)
        return self._pk

    def _pack(self):
        raise NotImplementedError

    def packed_with(self, key, build):
        """packed() with entries in it that only some routes need: build() -> dict of the entries to add (`key` among them), called at the
        first use of the route.  They live inside the pack: dropped and rebuilt with it."""
        pk = self.packed()
        if key not in pk:
            with torch.no_grad():
                pk.update(build(pk))
        return pk


class RelativePosition(nn.Module):
    """Reference attention.py:20-40: a table of 2 R + 1 embeddings indexed by clamp(s - t, -R, R) + R.  Parameter container: the two contractions
    with it are 64-wide GEMMs around the temporal attention kernel (TemporalTransformer.forward)."""

    def __init__(self, num_units, max_relative_position):
        super().__init__()
        self.num_units, self.max_relative_position = num_units, max_relative_position
        self.embeddings_table = nn.Parameter(torch.empty(max_relative_position * 2 + 1, num_units))
        nn.init.xavier_uniform_(self.embeddings_table)


class CrossAttention(PackedModule):
    """Reference attention.py:42-209.  Parameter container + packing; the attention itself is launched by the owning
    transformer (it needs the token geometry).  relative_position (`use_relative_position`; false in the ViewCrafter YAMLs) and the causal
    mask exist in the temporal transformer only: two table GEMMs around / a flag of the temporal attention kernel."""

    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0., relative_position=False,
                 temporal_length=None, video_length=None, image_cross_attention=False, image_cross_attention_scale=1.0,
                 image_cross_attention_scale_learnable=False, text_context_len=77):
        super().__init__()
        if relative_position and (temporal_length is None or 2 * temporal_length + 1 > 64 or context_dim is not None):
            raise NotImplementedError("relative_position: temporal self-attention with temporal_length <= 31 (2R + 1 table rows in 64 slots)")
        if image_cross_attention_scale_learnable:
            raise NotImplementedError("image_cross_attention_scale_learnable is not used by the ViewCrafter configs")
        if dim_head != 64:
            raise NotImplementedError(f"libvcx attention kernels are built for head dim 64 (got {dim_head})")
        if image_cross_attention and image_cross_attention_scale != 1.0:
            raise NotImplementedError("image_cross_attention_scale != 1.0 (the dual-softmax kernel sums the two outputs unweighted; "
                                      "the ViewCrafter configs keep the constant 1.0, attention.py:62)")
        inner_dim = dim_head * heads
        self.is_self = context_dim is None
        context_dim = default(context_dim, query_dim)
        self.scale = dim_head ** -0.5
        self.heads, self.dim_head, self.inner_dim = heads, dim_head, inner_dim
        self.to_q = nn.Linear(query_dim, inner_dim, bias=False)
        self.to_k = nn.Linear(context_dim, inner_dim, bias=False)
        self.to_v = nn.Linear(context_dim, inner_dim, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, query_dim), nn.Dropout(dropout))
        self.relative_position = bool(relative_position)
        if self.relative_position:      # (reference attention.py:59-62)
            self.relative_position_k = RelativePosition(num_units=dim_head, max_relative_position=temporal_length)
            self.relative_position_v = RelativePosition(num_units=dim_head, max_relative_position=temporal_length)
        self.video_length = video_length
        self.image_cross_attention = image_cross_attention
        self.image_cross_attention_scale = image_cross_attention_scale
        self.text_context_len = text_context_len
        if image_cross_attention:
            self.to_k_ip = nn.Linear(context_dim, inner_dim, bias=False)
            self.to_v_ip = nn.Linear(context_dim, inner_dim, bias=False)
        self.query_dim = query_dim
        self._pre_norm = None      # [LayerNorm] in front of the query-side projections (set by BasicTransformerBlock; a list so
        self.kind = None           # that it is not registered as a sub-module);  kind: "spatial" | "temporal" (owner's layout)

    def _pack(self):
        """wo / bo always; the query-side projections in the form their owner launches them - spatial self-attention: Q|K as one
        [tokens, 2D] projection carrying sqrt(scale log2 e) each + V^T; temporal: Q|K|V as one; cross-attention: Q carrying
        scale log2 e, and K / V (+ image K / V) weights for the context side - with the preceding LayerNorm folded in where possible."""
        pk = dict(wo=_f16(self.to_out[0].weight), bo=_f32(self.to_out[0].bias))
        ln = self._pre_norm[0] if (self._pre_norm and FOLD_LAYERNORM and self.query_dim % 64 == 0) else None
        wq, wk, wv = self.to_q.weight.detach(), self.to_k.weight.detach(), self.to_v.weight.detach()
        if not self.is_self:
            pk["q"] = _ln_projection(wq, ln, alpha=self.scale * ops.LOG2E)
            pk["wk"], pk["wv"] = _f16(wk), _f16(wv)
        elif self.kind == "temporal":
            pk["qkv"] = _ln_projection(torch.cat([wq, wk, wv], 0), ln)
        else:
            pk["qk"] = _ln_projection(torch.cat([wq, wk], 0), ln, alpha=math.sqrt(self.scale * ops.LOG2E))
            pk["v"] = _ln_projection(wv, ln)
        if self.image_cross_attention:
            pk["wk_ip"], pk["wv_ip"] = _f16(self.to_k_ip.weight), _f16(self.to_v_ip.weight)
        if self.relative_position:
            # Ek as the weight of  relg = q Ek^T  ([64 slots, 64 dims], rows 2R + 1 .. 63 zero) and Ev^T as the weight of  out += relp Ev  ([64 dims, 64 slots])
            ek, ev = self.relative_position_k.embeddings_table.detach(), self.relative_position_v.embeddings_table.detach()
            wk_rel = torch.zeros((64, 64), dtype=torch.float32, device=ek.device)
            wv_rel = torch.zeros((64, 64), dtype=torch.float32, device=ek.device)
            wk_rel[:ek.shape[0]] = ek.float()
            wv_rel[:, :ev.shape[0]] = ev.float().t()
            pk["rel_k"], pk["rel_v"], pk["rel_R"] = _f16(wk_rel), _f16(wv_rel), self.relative_position_k.max_relative_position
        return pk

    def mx_packed(self):
        """TATTN_MXFP8 (temporal self-attention): the MXFP8 pairs of the UN-folded cat(Wq, Wk, Wv) and of to_out's weight, a zero bias [3D]
        for the projection that has none (vcx_gemm_mxfp8 wants one) and bo.  SATTN_MXFP8 (kind "spatial"): self-attention - the pairs of
        sqrt(scale log2 e) * cat(Wq, Wk) (scaled in fp32, one fp16 rounding), of Wv and of to_out's weight, a zero bias [2D]; cross-attention -
        the pairs of scale log2 e * Wq and of to_out's weight, a zero bias [D].  Built at first use of the route (packed_with)."""
        def build(pk):
            wq, wk, wv = self.to_q.weight.detach().float(), self.to_k.weight.detach().float(), self.to_v.weight.detach().float()
            zeros = lambda n: torch.zeros(n, dtype=torch.float32, device=wq.device)
            if self.kind == "temporal":
                wqkv = _f16(torch.cat([self.to_q.weight.detach(), self.to_k.weight.detach(), self.to_v.weight.detach()], 0))
                mx = dict(wqkv=pack_mxfp8(wqkv), zero=zeros(wqkv.shape[0]))
            elif self.is_self:
                wqk = _f16(torch.cat([wq, wk], 0) * math.sqrt(self.scale * ops.LOG2E))
                mx = dict(wqk=pack_mxfp8(wqk), wv=pack_mxfp8(_f16(wv)), zero=zeros(wqk.shape[0]))
            else:
                wq2 = _f16(wq * (self.scale * ops.LOG2E))
                mx = dict(wq=pack_mxfp8(wq2), zero=zeros(wq2.shape[0]))
            return dict(mx=dict(mx, wo=pack_mxfp8(pk["wo"]), bo=pk["bo"]))
        return self.packed_with("mx", build)["mx"]

    def kv_pool_packed(self):
        """SATTN_KV_POOL (spatial self-attention): Q alone in the form today's Q|K pack has - folded where that is folded, carrying
        sqrt(scale log2 e) - and the plain fp16 weights of K and V, which project the pooled, already normalised rows.  Built at first use
        of the route (packed_with)."""
        def build(pk):
            ln, pv = self._pre_norm[0] if pk["qk"]["colsum"] is not None else None, pk["v"]
            return dict(kv_pool=dict(q=_ln_projection(self.to_q.weight.detach(), ln, alpha=math.sqrt(self.scale * ops.LOG2E)),
                                     wk=_f16(self.to_k.weight), wv=pv["w"] if pv["colsum"] is None else _plain_of(pv)[0]))
        return self.packed_with("kv_pool", build)["kv_pool"]

    def forward(self, *args, **kwargs):
        raise RuntimeError("CrossAttention is driven by SpatialTransformer/TemporalTransformer in this package")


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)


class FeedForward(PackedModule):
    """Reference attention.py:425-442 with glu=True: Linear(C, 8C) -> x * gelu(gate) -> Linear(4C, C).  The GEGLU gate
    is applied inside the first GEMM's epilogue (weights row-interleaved by pack_geglu)."""

    def __init__(self, dim, dim_out=None, mult=4, glu=False, dropout=0.):
        super().__init__()
        if not glu:
            raise NotImplementedError("only the gated (GEGLU) feed-forward is on the ViewCrafter path")
        inner_dim = int(dim * mult)
        dim_out = default(dim_out, dim)
        self.net = nn.Sequential(GEGLU(dim, inner_dim), nn.Dropout(dropout), nn.Linear(inner_dim, dim_out))
        self.dim = dim
        self._pre_norm = None      # [LayerNorm] in front of the GEGLU projection (set by BasicTransformerBlock)

    def _pack(self):
        proj = self.net[0].proj
        ln = self._pre_norm[0] if (self._pre_norm and FOLD_LAYERNORM and FOLD_LAYERNORM_FF and self.dim % 64 == 0 and self.dim >= FOLD_LAYERNORM_FF_MIN_DIM) else None
        p1 = _ln_projection(proj.weight.detach(), ln, bias=proj.bias)
        w1, b1 = pack_geglu(p1["w"], p1["bias"])
        colsum = None if p1["colsum"] is None else pack_geglu(p1["w"], p1["colsum"])[1]
        return dict(w=w1, bias=b1, colsum=colsum, w2=_f16(self.net[2].weight), b2=_f32(self.net[2].bias))      # (w / colsum / bias: a pack _ln_operands takes)

    def _mx_ok(self, t):
        """FF_MXFP8: does vcx_gemm_mxfp8 take BOTH linears at this row count (its own predicate)?  Either side refusing keeps the fp16 route."""
        proj, out = self.net[0].proj, self.net[2]
        rows = t.shape[0]
        return (self.dim not in FF_MXFP8_SKIP_DIMS and t.is_contiguous() and proj.bias is not None and out.bias is not None
                and ops.linear_mxfp8_ok(rows, proj.out_features, self.dim, geglu=True, mx_out=True)
                and ops.linear_mxfp8_ok(rows, out.out_features, out.in_features, residual=True))

    def _plain_glu(self):
        return pack_geglu(_f16(self.net[0].proj.weight), _f32(self.net[0].proj.bias))

    def glu(self, t, ln_params):
        """x * gelu(gate) of the GEGLU projection of LayerNorm(t), [rows, 4 dim]: the operand of net[2].  The fp16 route (FF_MXFP8 off, or _mx_ok refusing)."""
        def plain(pk):      # folded pack, shape the folded kernel cannot take: the un-folded (w1, b1), built at first use
            return self.packed_with("plain", lambda _: dict(plain=self._plain_glu()))["plain"]
        a, w1, b1, fold = _ln_operands(t, self.packed(), ln_params, plain=plain)
        return ops.linear(a, w1, b1, geglu=True, **fold)

    def run(self, t, ln_params, mx=None):
        """t + FF(LayerNorm(t)); ln_params = (gamma, beta, eps) of the LayerNorm in front (used when it is not folded into w1).  mx: the
        answer of FF_MXFP8 and _mx_ok(t) where the caller has asked already (ff_proj_out)."""
        pk = self.packed()
        if (FF_MXFP8 and self._mx_ok(t)) if mx is None else mx:
            def build(pk):          # beside the fp16 packs, from the un-folded weights
                w1, b1 = self._plain_glu()
                return dict(mx=dict(w1=pack_mxfp8(w1), b1=b1, w2=pack_mxfp8(pk["w2"])))
            pm = self.packed_with("mx", build)["mx"]
            a = ops.layer_norm_mxfp8(t, *ln_params)
            g = ops.linear_mxfp8(a, pm["w1"], pm["b1"], K=self.dim, geglu=True, mx_out=True)
            return ops.linear_mxfp8(g, pm["w2"], pk["b2"], K=pk["w2"].shape[1], residual=t)
        return ops.linear(self.glu(t, ln_params), pk["w2"], pk["b2"], residual=t)


class BasicTransformerBlock(PackedModule):
    """Reference attention.py:212-246 (attn1 self, attn2 cross or - in temporal blocks - self again, GEGLU FF)."""

    def __init__(self, dim, n_heads, d_head, dropout=0., context_dim=None, gated_ff=True, checkpoint=True,
                 disable_self_attn=False, attention_cls=None, video_length=None, image_cross_attention=False,
                 image_cross_attention_scale=1.0, image_cross_attention_scale_learnable=False, text_context_len=77):
        super().__init__()
        if disable_self_attn:
            raise NotImplementedError("disable_self_attn is not used by the ViewCrafter configs")
        attn_cls = CrossAttention if attention_cls is None else attention_cls
        self.attn1 = attn_cls(query_dim=dim, heads=n_heads, dim_head=d_head, dropout=dropout, context_dim=None)
        self.ff = FeedForward(dim, dropout=dropout, glu=gated_ff)
        self.attn2 = attn_cls(query_dim=dim, context_dim=context_dim, heads=n_heads, dim_head=d_head, dropout=dropout,
                              video_length=video_length, image_cross_attention=image_cross_attention,
                              image_cross_attention_scale=image_cross_attention_scale,
                              image_cross_attention_scale_learnable=image_cross_attention_scale_learnable,
                              text_context_len=text_context_len)
        self.image_cross_attention = image_cross_attention
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.norm3 = nn.LayerNorm(dim)
        self.checkpoint = checkpoint
        self.attn1._pre_norm, self.attn2._pre_norm, self.ff._pre_norm = [self.norm1], [self.norm2], [self.norm3]

    def set_kind(self, kind):
        self.attn1.kind = self.attn2.kind = kind

    def _drop_packed(self):
        super()._drop_packed()
        for m in (self.attn1, self.attn2, self.ff):      # their packs hold this block's LayerNorm parameters
            m._drop_packed()

    def _pack(self):
        return [(_f32(n.weight), _f32(n.bias), n.eps) for n in (self.norm1, self.norm2, self.norm3)]

    def ln_params(self):
        return self.packed()


def ff_proj_out(tr, t, ln_params, xin, kw, video_rows):
    """proj_out(t + FF(LayerNorm(t))) + xin behind the last block of transformer `tr` (Spatial / Temporal), kw = out_kwargs' keywords
    of the proj_out call.  One GEMM over [g ; t] where FF_OUT_FOLD applies (see there), ff.run + proj_out otherwise.  The two forms
    differ in the last bits, so which one runs must not depend on the batch: the dispatcher is asked about the rows of ONE video and
    about the call itself (only the 4 GiB extents then depend on the whole call), like ops.rowstats_ok."""
    pk, ff = tr.packed(), tr.transformer_blocks[-1].ff
    tokens, D = t.shape
    C = pk["wout"].shape[0]
    mx = FF_MXFP8 and ff._mx_ok(t)      # the feed-forward's engine, asked once: for the fold and for ff.run
    fold = (FF_OUT_FOLD and t.is_cuda and D not in FF_OUT_FOLD_SKIP_DIMS and ff.net[2].bias is not None and not mx
            and all(ops.linear_tail_ok(m, C, ff.net[2].in_features, [D], ldc=kw.get("ldc"), residual=True, colstats="colstats" in kw)
                    for m in sorted({video_rows, tokens})))
    if not fold:
        return ops.linear(ff.run(t, ln_params, mx), pk["wout"], pk["bout"], residual=xin, **kw)
    pk = tr.packed_with("wcat", lambda pk: dict(zip(("wcat", "bcat"), pack_ff_out_folded(ff.net[2].weight, ff.net[2].bias, pk["wout"], pk["bout"]))))
    return ops.linear(ff.glu(t, ln_params), pk["wcat"], pk["bcat"], tail=[t], residual=xin, **kw)


class _Transformer(PackedModule):
    """What SpatialTransformer and TemporalTransformer pack alike: the norm, proj_in and proj_out (a linear layer, or its 1x1 / k = 1
    convolution form: the same matmul on a channels-last row, the weight reshaped)."""

    def _foreign_params(self):
        ff2 = self.transformer_blocks[-1].ff.net[2]
        return [ff2.weight] + ([] if ff2.bias is None else [ff2.bias])

    def _pack(self):
        """+ wcat / bcat, built on first use by ff_proj_out: [Wout W2 | Wout] and Wout b2 + bout, DERIVED FROM transformer_blocks[-1].ff.net[2]
        (a child's parameters: _foreign_params rebuilds the pack when they change, _drop_packed discards it with the rest)."""
        win = self.proj_in.weight.detach().reshape(self.proj_in.weight.shape[0], -1)
        wout = self.proj_out.weight.detach().reshape(self.proj_out.weight.shape[0], -1)
        return dict(gn_w=_f32(self.norm.weight), gn_b=_f32(self.norm.bias), win=_f16(win), win32=_f32(win), bin=_f32(self.proj_in.bias),
                    wout=_f16(wout), bout=_f32(self.proj_out.bias))


class ContextKV:
    """Projected cross-attention keys/values of one SpatialTransformer block for one conditioning tensor.  They depend
    only on the context, i.e. they are constant over all DDIM steps and are cached by UNetModel."""
    __slots__ = ("k_txt", "vt_txt", "k_img", "vt_img", "n_txt_rows", "n_txt", "n_img", "img_per_frame")


def project_context(attn2, ctx):
    """ctx: dict(txt=[B*80, D] fp16 (rows 77..79 zero), img=[G*Li, D] fp16 or None, n_img=Li, per_frame=bool)."""
    pk = attn2.packed()
    kv = ContextKV()
    txt = ctx["txt"]
    D = txt.shape[1]
    C = attn2.inner_dim
    kv.k_txt = ops.linear(txt, pk["wk"])                                        # [B*80, C]
    kv.vt_txt = ops.gemm(pk["wv"], txt, M=C, N=txt.shape[0], K=D, lda=D)        # [C, B*80]  (V^T for the flash kernel)
    kv.n_txt_rows = txt.shape[0]
    kv.n_txt = int(ctx.get("n_txt", attn2.text_context_len))      # real text tokens (a context shorter than 77 is zero-padded to 80 rows)
    kv.k_img = kv.vt_img = None
    kv.n_img, kv.img_per_frame = ctx.get("n_img", 0), ctx.get("per_frame", False)
    if attn2.image_cross_attention and ctx.get("img") is not None:
        img = ctx["img"]
        kv.k_img = ops.linear(img, pk["wk_ip"])
        kv.vt_img = ops.gemm(pk["wv_ip"], img, M=C, N=img.shape[0], K=D, lda=D)
    return kv


def _norm_proj_in(tr, x, unit_rows, stats, fold, rowstats, pad=None):
    """GroupNorm -> proj_in of transformer `tr` over x [..., C], `unit_rows` rows a statistics unit (Spatial: a frame, Temporal: a video);
    stats: the units' statistics where the caller has them.  fold: the norm as per-unit weights / bias of the projection, which reads the
    un-normalised rows; else the norm is applied.  rowstats: the projection writes the row statistics of its output (VCX_GEMM_ROWSTATS).
    pad (never with fold): rows -> rows with every frame padded.  -> (token stream, its row statistics or None, the rows of x, padded)"""
    pk, C = tr.packed(), x.shape[-1]
    xin = x.reshape(-1, C)
    units = xin.shape[0] // unit_rows
    if fold:
        if stats is None:
            stats = ops.group_norm_stats(x.view(units, unit_rows, C))
        wn, bn = ops.group_norm_fold_linear(pk["win32"], pk["bin"], pk["gn_w"], pk["gn_b"], stats, tr.norm.eps)
    else:
        a = ops.group_norm(x.view(units, unit_rows, C), pk["gn_w"], pk["gn_b"], tr.norm.eps, False, stats=stats).view(-1, C)
        if pad is not None:
            xin, a = pad(xin), pad(a)
    rs = ops.rowstats_buffer(xin.shape[0], x.device) if rowstats else None
    rs_eps = tr.transformer_blocks[0].norm1.eps
    if fold:
        return ops.gemm_units(xin, wn, bn, unit_rows=unit_rows, rowstats=rs, rowstats_eps=rs_eps), rs, xin
    return ops.linear(a, pk["win"], pk["bin"], rowstats=rs, rowstats_eps=rs_eps), rs, xin


def _to_out(o, ap, t, mx, **kw):
    """to_out of an attention with the residual t; ap: the attention's pack of its engine (packed() / mx_packed(): wo, bo), o: the fp16
    attention output / its MXFP8 pair.  kw: further keywords of the fp16 layer (row statistics: the MX route requests none)."""
    if mx:
        return ops.linear_mxfp8(o, ap["wo"], ap["bo"], K=t.shape[1], residual=t)
    return ops.linear(o, ap["wo"], ap["bo"], residual=t, **kw)


# ---- the attention calls of a SpatialTransformer: one geometry function per call - the keywords the MX predicate, the fp16 launcher (+ ldo,
# log2_logits) and the MX launcher all take - and one function per engine.  scale * log2(e) rides in the projections (sqrt of it on Q and on K
# of the self-attention: one fp16 rounding each, as without it), so the kernels get base-2 logits and the running max can live in the MFMA
# accumulator (VCX_ATTN_LOG2_LOGITS).
def _self_attn_geometry(frames, heads, N, N_img, D, pool=None):
    """Self-attention over `frames` frames of N rows, the first N_img of them tokens (keys; the pad rows' results are dropped): q|k one
    [tokens, 2D] projection, V^T [D, tokens].  pool (kv_pool_plan): Q alone [tokens, D], keys and values the rows of the pooled grid."""
    kv_rows, nk, ld = (N, N_img, 2 * D) if pool is None else (pool[0] * pool[1], pool[0] * pool[1], D)
    return dict(n_groups=frames, heads=heads, nq=N, nk=nk, kv_rows=kv_rows, kv_div=1, ldq=ld, ldk=ld, ldvt=frames * kv_rows)


def _cross_attn_geometry(kv, frames, heads, N, D, frames_per_video):
    """Cross-attention of `frames` frames of N rows to the context kv (ContextKV): text keys (80 rows a video) shared by the frames of a
    video, and - kv.k_img: the dual kernels, text (+) image in one pass over q and o - image keys per video or per frame."""
    ldvt = kv.n_txt_rows // 80 * 80
    if kv.k_img is None:
        return dict(n_groups=frames, heads=heads, nq=N, nk=kv.n_txt, kv_rows=80, kv_div=frames_per_video, ldq=D, ldk=D, ldvt=ldvt)
    return dict(n_groups=frames, heads=heads, nq=N, nk1=kv.n_txt, kv_rows1=80, kv_div1=frames_per_video, ldk1=D, ldvt1=ldvt, nk2=kv.n_img,
                kv_rows2=kv.n_img, kv_div2=1 if kv.img_per_frame else frames_per_video, ldk2=D, ldvt2=kv.vt_img.shape[1], ldq=D)


def _attend(q, kvt, geo, scale, mx):
    """One attention call of a SpatialTransformer: kvt = (k, V^T) with the keywords of _self_attn_geometry, or the context's (k_txt, vt_txt
    [, k_img, vt_img]) with those of _cross_attn_geometry; mx: the quantising kernel.  -> [tokens, D] fp16, or its MXFP8 pair"""
    dual, D = len(kvt) == 4, 64 * geo["heads"]
    if mx:
        return (ops.flash_attn_dual_mxfp8 if dual else ops.flash_attn_mxfp8)(q, *kvt, **geo, scale=scale)
    o = torch.empty((q.shape[0], D), dtype=torch.float16, device=q.device)
    return (ops.flash_attn_dual if dual else ops.flash_attn)(q, *kvt, o, **geo, ldo=D, scale=scale, log2_logits=True)


def _sattn_fp16(blk, lnp, t, geo, stats, grid):
    """The self-attention of one SpatialTransformer block up to its output projection, fp16 engine -> [tokens, D].  lnp = (gamma, beta, eps)
    of norm1 (folded into both projections wherever _ln_operands says so), stats = the row statistics of t where its producer wrote them."""
    a1, D = blk.attn1.packed(), t.shape[1]
    if stats is None and a1["qk"]["colsum"] is not None:
        stats = ops.row_stats(t, lnp[2])
    qk = ln_linear(t, a1["qk"], lnp, alpha=math.sqrt(blk.attn1.scale * ops.LOG2E), stats=stats)      # [tokens, 2D]
    vt = ln_linear_t(t, a1["v"], lnp, stats=stats)                                                   # [D, tokens]
    return _attend(qk, (qk[:, D:], vt), geo, blk.attn1.scale, False)


def _sattn_kv_pool(blk, lnp, t, geo, stats, grid):
    """The same on the SATTN_KV_POOL route, every query and the keys and values of the 2x2-pooled tokens: five calls (six where the folded Q
    projection has no row statistics from its producer), in this order.  t [n H W, D] (kv_pool_plan: no padded rows), grid = (H, W)."""
    pp, D, n = blk.attn1.kv_pool_packed(), t.shape[1], geo["n_groups"]
    alpha = math.sqrt(blk.attn1.scale * ops.LOG2E)
    q = ln_linear(t, pp["q"], lnp, alpha=alpha, stats=stats)                                     # [tokens, D], every query
    p = ops.layer_norm_pool2x2(t, *lnp, n, *grid, _KV_POOL_MODES[SATTN_KV_POOL])                 # [n Np, D], normalised and pooled
    k = ops.linear(p, pp["wk"], None, alpha=alpha)                                               # [n Np, D]
    vt = ops.gemm(pp["wv"], p, M=D, N=n * geo["kv_rows"], K=D, lda=D)                            # [D, n Np]
    return _attend(q, (k, vt), geo, blk.attn1.scale, False)


def _sattn_mx(blk, lnp, t, geo, stats, grid):
    """The same on the SATTN_MXFP8 route: four calls (the quantising LayerNorm computes its own statistics).  -> the MXFP8 pair [tokens, Kp(D)]"""
    m1, D = blk.attn1.mx_packed(), t.shape[1]
    an = ops.layer_norm_mxfp8(t, *lnp)
    qk = ops.linear_mxfp8(an, m1["wqk"], m1["zero"], K=D)                     # [tokens, 2D] fp16, base-2 logit scale in the weights
    vt = ops.linear_t_mxfp8(an, m1["wv"], K=D)                                # [D, tokens] fp16
    return _attend(qk, (qk[:, D:], vt), geo, blk.attn1.scale, True)


SpatialPlan = namedtuple("SpatialPlan", "N fold engine pool rowstats")
TemporalPlan = namedtuple("TemporalPlan", "fold engine rowstats")


class SpatialTransformer(_Transformer):
    """Reference attention.py:249-310 (use_linear=True, or False = 1x1 Conv2d projections): GN(eps 1e-6) -> proj_in -> [LN, self-attn, LN, text (+) image
    cross-attn, LN, GEGLU-FF] -> proj_out -> + x."""

    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0., context_dim=None, use_checkpoint=True,
                 disable_self_attn=False, use_linear=False, video_length=None, image_cross_attention=False,
                 image_cross_attention_scale_learnable=False):
        super().__init__()
        self.in_channels = in_channels
        inner_dim = n_heads * d_head
        self.n_heads = n_heads
        self.norm = nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)
        # use_linear=False (reference attention.py:266-267, 287-288; not used by the ViewCrafter YAMLs): 1x1 Conv2d projections - the same
        # matmul on a channels-last row; the parameters keep the reference's [out, in, 1, 1] shape so a checkpoint loads strictly
        self.proj_in = nn.Linear(in_channels, inner_dim) if use_linear else nn.Conv2d(in_channels, inner_dim, kernel_size=1, stride=1, padding=0)
        self.transformer_blocks = nn.ModuleList([
            BasicTransformerBlock(inner_dim, n_heads, d_head, dropout=dropout, context_dim=context_dim,
                                  disable_self_attn=disable_self_attn, checkpoint=use_checkpoint, attention_cls=None,
                                  video_length=video_length, image_cross_attention=image_cross_attention,
                                  image_cross_attention_scale_learnable=image_cross_attention_scale_learnable)
            for _ in range(depth)])
        for blk in self.transformer_blocks:
            blk.set_kind("spatial")
        self.proj_out = nn.Linear(inner_dim, in_channels) if use_linear else nn.Conv2d(inner_dim, in_channels, kernel_size=1, stride=1, padding=0)
        nn.init.zeros_(self.proj_out.weight)
        nn.init.zeros_(self.proj_out.bias)
        self.use_linear = use_linear

    def project_context(self, ctx):
        return [project_context(blk.attn2, ctx) for blk in self.transformer_blocks]

    def _mx_accepts(self, n, N, N_img, D, context_kv, frames_per_video, cfg_repeat):
        """SATTN_MXFP8: the width is not skipped and the library takes the attentions of every block - every predicate asked about the frames
        of ONE video (a row's route must not depend on the batch it runs in: B = 2 against two B = 1, the shared CFG prefix against the
        replicated batch) and about the call itself, before and behind the CFG replication (only the 32-bit extents depend on the batch)."""
        heads = self.n_heads
        if not SATTN_MXFP8 or D in SATTN_MXFP8_SKIP_DIMS or any(a.to_out[0].bias is None or a.inner_dim != D or a.query_dim != D
                                                                  for blk in self.transformer_blocks for a in (blk.attn1, blk.attn2)):
            return False
        for frames in sorted({frames_per_video, n, n * cfg_repeat}):
            tokens = frames * N
            if not (ops.linear_mxfp8_ok(tokens, 2 * D, D) and ops.linear_t_mxfp8_ok(tokens, D, D) and ops.linear_mxfp8_ok(tokens, D, D)
                    and ops.linear_mxfp8_ok(tokens, D, D, residual=True) and ops.flash_attn_mxfp8_ok(**_self_attn_geometry(frames, heads, N, N_img, D))):
                return False
            if not all((ops.flash_attn_mxfp8_ok if kv.k_img is None else ops.flash_attn_dual_mxfp8_ok)(
                    **_cross_attn_geometry(kv, frames, heads, N, D, frames_per_video)) for kv in context_kv):
                return False
        return True

    def _plan(self, x, context_kv, frames_per_video=1, cfg_repeat=1):
        """Every routing decision of a forward, made before the first launch or buffer (packs aside: built at first use) -> SpatialPlan.  N: the rows of a frame, h*w
        padded to a multiple of 8 (the attention kernels address a frame's keys / values at 16-byte granularity; e.g. 384x640: 6x10 = 60
        tokens at the deepest level).  fold: the norm as per-frame weights / bias of proj_in.  engine: "pool" (pool = the grid of
        kv_pool_plan, asked first: a call that pools asks no MX predicate), "mx" (SATTN_MXFP8: both attentions of every block) or "fp16";
        any refusal keeps the fp16 calls for the whole transformer.  rowstats: proj_in writes the row statistics norm1 of the first block
        reads (VCX_GEMM_ROWSTATS: the producer is the weight-stationary kernel, C = 320, and the consumer a folded projection; row_stats,
        one read of the tensor, otherwise; none on the MX route, whose quantising LayerNorm computes its own).  fold and rowstats change the
        last bits, so they are decided on the rows of ONE video: the shared CFG prefix must match the replicated batch bit for bit."""
        n, H, W, C = x.shape
        N_img, D = H * W, self.packed()["win"].shape[0]
        N = (N_img + 7) // 8 * 8
        pool = kv_pool_plan(H, W, D)
        engine = "pool" if pool is not None else "mx" if self._mx_accepts(n, N, N_img, D, context_kv, frames_per_video, cfg_repeat) else "fp16"
        fold = bool(N_img % 8 == 0 and spatial_fold_ok(frames_per_video, N_img, C, D) and fold_extent_ok(n * N_img, max(C, D)))
        attn1 = self.transformer_blocks[0].attn1
        p1 = attn1.kv_pool_packed()["q"] if pool is not None else attn1.packed()["qk"]      # the projection that reads norm1's statistics
        rowstats = engine != "mx" and _folded(p1, n * N, D, D) and ops.rowstats_ok(n * N, D, C, lda=C, unit_rows=N_img if fold else None,
                                                                                   video_rows=frames_per_video * N)
        return SpatialPlan(N, fold, engine, pool, rowstats)

    def forward(self, x, context_kv=None, frames_per_video=1, cfg_repeat=1, colstats=None, want_colstats=False, **kwargs):
        """x [n, H, W, C] fp16 channels-last, n = b*t frames; context_kv from project_context().
        cfg_repeat = r > 1: x holds ONE copy of a batch whose r conditionings (classifier-free guidance: cond / uncond / ...)
        share everything up to here; everything that does not depend on the context - GroupNorm, proj_in, the whole
        self-attention of the first block, LayerNorm and the Q projection of its cross-attention - is computed once and the
        token stream is replicated r times right before the first cross-attention (context_kv holds r * b videos).  The
        result [r * n, H, W, C] equals the forward of the r-fold replicated input bit for bit.
        colstats: column moments of x (no statistics pass for the norm); want_colstats: let proj_out write the moments of the
        result for the GroupNorm of the layer behind this one.  -> (result, its moments or None)"""
        n, H, W, C = x.shape
        N_img = H * W
        plan = self._plan(x, context_kv, frames_per_video, cfg_repeat)
        N, mx, self_attn = plan.N, plan.engine == "mx", {"fp16": _sattn_fp16, "pool": _sattn_kv_pool, "mx": _sattn_mx}[plan.engine]
        stats = None if colstats is None else ops.group_norm_stats_from_colstats(colstats, n, N_img, C)

        def pad_frames(src):      # zero rows up to N behind each frame for the length of this transformer: all its layers are row-wise
            dst = torch.zeros((n * N, C), dtype=torch.float16, device=x.device)      # except the attentions, which take nq = N and nk = h*w
            ops.copy2d(src, dst, n, N_img * C, N_img * C, N * C)           # one "row" per frame
            return dst
        t, rs, xin = _norm_proj_in(self, x, N_img, stats, plan.fold, plan.rowstats, pad_frames if N != N_img else None)
        tokens, video_rows, D, heads = n * N, frames_per_video * N, t.shape[1], self.n_heads
        for bi, (blk, kv) in enumerate(zip(self.transformer_blocks, context_kv)):
            ln = blk.ln_params()
            a1, a2 = [a.mx_packed() if mx else a.packed() for a in (blk.attn1, blk.attn2)]
            # ---- self-attention over the h*w tokens of each frame; its output projection writes norm2's row statistics as proj_in writes norm1's
            o = self_attn(blk, ln[0], t, _self_attn_geometry(n, heads, N, N_img, D, plan.pool), rs if bi == 0 else None, (H, W))
            st2 = ops.rowstats_buffer(tokens, x.device) if (not mx and _folded(a2["q"], tokens, D, D)
                                                            and ops.rowstats_ok(tokens, D, D, ldr=D, video_rows=video_rows)) else None
            t = _to_out(o, a1, t, mx, rowstats=st2, rowstats_eps=ln[1][2])
            # ---- cross-attention: softmax(Q K_txt) V_txt + softmax(Q K_img) V_img
            if mx:
                q2 = ops.linear_mxfp8(ops.layer_norm_mxfp8(t, *ln[1]), a2["wq"], a2["zero"], K=D)
            else:
                q2 = ln_linear(t, a2["q"], ln[1], alpha=blk.attn2.scale * ops.LOG2E, stats=st2)
            if bi == 0 and cfg_repeat > 1:      # from here on the r conditionings differ
                t, q2, xin = ops.repeat_rows(t, cfg_repeat), ops.repeat_rows(q2, cfg_repeat), ops.repeat_rows(xin, cfg_repeat)
                n, tokens = n * cfg_repeat, tokens * cfg_repeat
            ctx = (kv.k_txt, kv.vt_txt) if kv.k_img is None else (kv.k_txt, kv.vt_txt, kv.k_img, kv.vt_img)
            o2 = _attend(q2, ctx, _cross_attn_geometry(kv, n, heads, N, D, frames_per_video), blk.attn2.scale, mx)
            t = _to_out(o2, a2, t, mx)
            # ---- feed-forward (the last block's: with proj_out, below)
            if bi + 1 < len(self.transformer_blocks):
                t = blk.ff.run(t, ln[2])
        kw, cs_out = out_kwargs(None, want_colstats and N == N_img, tokens, N_img, D, C, x.device)
        out = ff_proj_out(self, t, ln[2], xin, kw, video_rows)
        if N != N_img:
            unpadded = torch.empty((n * N_img, C), dtype=torch.float16, device=x.device)
            ops.copy2d(out, unpadded, n, N_img * C, N * C, N_img * C)
            out = unpadded
        return out.view(n, H, W, C), cs_out


class TemporalTransformer(_Transformer):
    """Reference attention.py:313-412 with only_self_att=True: GN over (C/32, T, H, W) -> proj_in -> [LN, self-attn
    over T, LN, self-attn over T again (context None, :389-390), LN, GEGLU-FF] -> proj_out -> + x."""

    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0., context_dim=None, use_checkpoint=True,
                 use_linear=False, only_self_att=True, causal_attention=False, causal_block_size=1,
                 relative_position=False, temporal_length=None):
        super().__init__()
        if not only_self_att:
            raise NotImplementedError("ViewCrafter uses temporal self-attention only")
        if relative_position and temporal_length is None:
            raise AssertionError("relative_position needs temporal_length (reference attention.py:339)")
        # causal_attention (reference attention.py:343-345, 377-384: a lower-triangular mask over the frames, handed to attn1 AND attn2 of every block,
        # :241-243; `use_causal_attention`, not used by the ViewCrafter YAMLs): VCX_ATTN_CAUSAL of the temporal attention kernel
        if causal_attention and temporal_length is None:
            raise AssertionError("causal_attention needs temporal_length (reference attention.py:344)")
        self.causal_attention = bool(causal_attention)
        self.temporal_length = temporal_length
        self.only_self_att = only_self_att
        self.in_channels = in_channels
        inner_dim = n_heads * d_head
        self.n_heads = n_heads
        self.norm = nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)
        if not use_linear:   # init_attn: Conv1d k=1 (openaimodel3d.py:389-399); same matmul, weight [inner, C, 1]
            self.proj_in = nn.Conv1d(in_channels, inner_dim, kernel_size=1, stride=1, padding=0)
            self.proj_out = nn.Conv1d(inner_dim, in_channels, kernel_size=1, stride=1, padding=0)
        else:
            self.proj_in = nn.Linear(in_channels, inner_dim)
            self.proj_out = nn.Linear(inner_dim, in_channels)
        nn.init.zeros_(self.proj_out.weight)
        nn.init.zeros_(self.proj_out.bias)

        def attention_cls(**kw):
            return CrossAttention(temporal_length=temporal_length, relative_position=bool(relative_position), **kw)
        self.transformer_blocks = nn.ModuleList([
            BasicTransformerBlock(inner_dim, n_heads, d_head, dropout=dropout, context_dim=None,
                                  attention_cls=attention_cls, checkpoint=use_checkpoint) for _ in range(depth)])
        for blk in self.transformer_blocks:
            blk.set_kind("temporal")
        self.use_linear = use_linear

    def _mx_accepts(self, x, D):
        """TATTN_MXFP8: width not skipped, T <= 32, no relative position, dense rows, and the library's three predicates - asked about ONE
        video (a row's route must not depend on the batch it runs in) and about the call itself (only the 32-bit extents depend on B)."""
        B, T, P, _ = x.shape
        if not TATTN_MXFP8 or D in TATTN_MXFP8_SKIP_DIMS or T > 32 or not x.is_contiguous() or any(
                a.relative_position or a.to_out[0].bias is None or a.inner_dim != D or a.query_dim != D
                for blk in self.transformer_blocks for a in (blk.attn1, blk.attn2)):
            return False
        attn_ok = lambda g: ops.temporal_attn_mxfp8_ok(g["B"], g["T"], g["P"], g["heads"], g["ld"], causal=g["causal"])      # (no use for the offsets)
        return all(ops.linear_mxfp8_ok(b * T * P, 3 * D, D) and ops.linear_mxfp8_ok(b * T * P, D, D, residual=True)
                   and attn_ok(self._attn_geometry(b, T, P, D)) for b in sorted({1, B}))

    def _attn_geometry(self, B, T, P, D):
        """The keywords every temporal attention kernel takes: q|k|v one [tokens, 3D] projection."""
        return dict(B=B, T=T, P=P, heads=self.n_heads, ld=3 * D, k_off=D, v_off=2 * D, causal=self.causal_attention)

    def _plan(self, x):
        """Every routing decision of a forward, made before the first launch or activation buffer -> TemporalPlan.  fold: temporal_fold_ok.
        engine of all self-attentions: "mx" (TATTN_MXFP8) or "fp16"; any refusal keeps the fp16 calls for the whole transformer.  rowstats:
        proj_in writes the row statistics norm1 of the first block reads (as SpatialTransformer._plan; none on the MX route)."""
        B, T, P, C = x.shape
        D, rows, tokens = self.packed()["win"].shape[0], T * P, B * T * P
        engine = "mx" if self._mx_accepts(x, D) else "fp16"
        fold = bool(temporal_fold_ok(rows, C, D))
        rowstats = engine != "mx" and _folded(self.transformer_blocks[0].attn1.packed()["qkv"], tokens, D, D) and ops.rowstats_ok(
            tokens, D, C, lda=C, unit_rows=rows if fold else None, video_rows=rows)
        return TemporalPlan(fold, engine, rowstats)

    def forward(self, x, context=None, colstats=None, want_colstats=False, target=None):
        """x [B, T, P, C] fp16 channels-last (P = h*w).  colstats: column moments of x (the per-video norm then needs no statistics
        pass); want_colstats / target: proj_out writes the moments of the result / the result itself into a concat buffer
        (lvdm/modules/flow.py).  -> (result [B, T, P, C or ld], its moments or None)"""
        B, T, P, C = x.shape
        rows, tokens = T * P, B * T * P
        plan = self._plan(x)
        mx, self_attn = plan.engine == "mx", _tattn_mx if plan.engine == "mx" else _tattn_fp16
        stats = None if (colstats is None or GN_STATS_LEVEL < 2) else ops.group_norm_stats_from_colstats(colstats, B, rows, C)
        t, st, xin = _norm_proj_in(self, x, rows, stats, plan.fold, plan.rowstats)
        D = t.shape[1]
        geo = self._attn_geometry(B, T, P, D)
        for blk in self.transformer_blocks:
            ln = blk.ln_params()
            for ai, (attn, lnp) in enumerate(((blk.attn1, ln[0]), (blk.attn2, ln[1]))):
                o = self_attn(attn, lnp, t, geo, st)
                st = ops.rowstats_buffer(tokens, x.device) if (not mx and ai == 0 and _folded(blk.attn2.packed()["qkv"], tokens, D, D)
                                                               and ops.rowstats_ok(tokens, D, D, ldr=D, video_rows=rows)) else None
                t = _to_out(o, attn.mx_packed() if mx else attn.packed(), t, mx, rowstats=st, rowstats_eps=ln[1][2])
            if blk is not self.transformer_blocks[-1]:      # (the last block's feed-forward: with proj_out, below)
                t = blk.ff.run(t, ln[2])
        kw, cs_out = out_kwargs(target, want_colstats, tokens, P, D, C, x.device)
        out = ff_proj_out(self, t, ln[2], xin, kw, rows)
        return out.view(B, T, P, -1), cs_out


def _tattn_fp16(attn, lnp, t, geo, stats):
    """One self-attention over T of a TemporalTransformer block up to its output projection, fp16 engine -> [tokens, D].  lnp = (gamma,
    beta, eps) of the norm in front, geo = _attn_geometry, stats = the row statistics of t where its producer wrote them."""
    ap, (tokens, D), heads = attn.packed(), t.shape, geo["heads"]
    qkv = ln_linear(t, ap["qkv"], lnp, stats=stats)                         # [tokens, 3D]
    o = torch.empty((tokens, D), dtype=torch.float16, device=t.device)
    if not attn.relative_position:
        return ops.temporal_attn(qkv, o, **geo, ldo=D, scale=attn.scale)
    # logits += q Ek^T (per head: a [tokens, 64] x [64, 64] GEMM on the q columns of qkv), out += (probabilities by clipped distance) Ev
    relg = torch.empty((tokens, heads, 64), dtype=torch.float16, device=t.device)
    relp = torch.zeros((tokens, heads, 64), dtype=torch.float16, device=t.device)
    for h_ in range(heads):
        ops.gemm(qkv[:, h_ * 64:], ap["rel_k"], M=tokens, N=64, K=64, lda=3 * D, out=relg[:, h_], ldc=heads * 64)
    ops.temporal_attn_rel(qkv, o, relg, relp, R=ap["rel_R"], **geo, ldo=D, scale=attn.scale)
    for h_ in range(heads):
        ops.gemm(relp[:, h_], ap["rel_v"], M=tokens, N=64, K=64, lda=heads * 64, out=o[:, h_ * 64:], ldc=D, residual=o[:, h_ * 64:], ldr=D)
    return o


def _tattn_mx(attn, lnp, t, geo, stats):
    """The same on the TATTN_MXFP8 route (the quantising LayerNorm computes its own statistics) -> the MXFP8 pair [tokens, Kp(D)]"""
    am = attn.mx_packed()
    qkv = ops.linear_mxfp8(ops.layer_norm_mxfp8(t, *lnp), am["wqkv"], am["zero"], K=t.shape[1])           # [tokens, 3D] fp16
    return ops.temporal_attn_mxfp8(qkv, **geo, scale=attn.scale)
