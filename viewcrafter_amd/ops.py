"""Thin torch-tensor front end of the libvcx C ABI.

Tensors are only used for device memory and streams; every function below launches one (or two)
hand-written gfx950 kernels through ctypes.  Activations are fp16 channels-last, i.e. a video
latent is [B, T, H, W, C] and all token matrices are [rows, C] views of it.

Which reference call sites each entry point stands in for (nn.Linear / Conv2d / Conv3d attention.py:53-57,
openaimodel3d.py:69-186, GroupNorm basics.py:76-81, LayerNorm attention.py:226-228, memory_efficient_attention
attention.py:175,187, the DDIM update ddim.py:228-279, ...) is tabulated in INTEGRATION.md section 2 and include/vcx.h.
"""
import ctypes
import os

import torch

from ._lib import (GEMM_BIAS_M, GEMM_BIAS_N, GEMM_COLSTATS, GEMM_CONV_SLABK, GEMM_GEGLU, GEMM_LNFOLD, GEMM_LNFOLD_T, GEMM_MXFP8_OUT, GEMM_OUT_F32, GEMM_RESIDUAL, GEMM_ROWADD, GEMM_ROWSTATS, PROF_FAMILIES,
                   ROUTE_UNITS_GROUPED, ROUTE_UNITS_LOOP, ROUTE_UNITS_WS320, TUNE, GemmDesc, VcxError, check, lib)
from .packing import conv_slab_major

_f16 = torch.float16
_f32 = torch.float32
# LayerNorm statistics from the producing layer's epilogue (VCX_GEMM_ROWSTATS, round 6); 0 = a statistics pass everywhere (A/B runs)
LN_ROWSTATS = os.environ.get("VCX_LN_ROWSTATS", "1") != "0"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _dev16(*tensors):
    """The C ABI takes raw pointers: a host tensor or a wrong element type would be read as garbage, not rejected."""
    for t in tensors:
        if t is not None and (t.dtype is not _f16 or not t.is_cuda):
            raise VcxError(f"expected a GPU fp16 tensor, got {t.dtype} on {t.device}")


def _dev32(*tensors):
    for t in tensors:
        if t is not None and (t.dtype is not _f32 or not t.is_cuda):
            raise VcxError(f"expected a GPU fp32 tensor, got {t.dtype} on {t.device}")


def _out_arg(out, ldc, M, n_out, like, dtype=_f16, what=None):
    """(out, ldc) of a launcher's `out` / `ldc` keywords: a fresh dense [M, n_out] tensor on the device of `like`, or the caller's with its
    row stride where ldc is not given.  `what` (the MXFP8 convolutions): the caller's buffer must hold M rows of that pitch."""
    if out is None:
        return torch.empty((M, n_out), dtype=dtype, device=like.device), n_out
    if ldc is None:
        ldc = out.stride(0)
    if what is not None and out.numel() < (M - 1) * ldc + n_out:
        raise VcxError(f"{what}: out holds {out.numel()} elements, [{M}] rows of pitch {ldc} need {(M - 1) * ldc + n_out}")
    return out, ldc


def _colstats_arg(colstats, colstats_ld, colstats_col, M, n_out):
    """(pointer to the moments of the call's first column, ldcs) of a launcher's colstats* keywords; (None, 0) without a buffer."""
    if colstats is None:
        return None, 0
    _dev32(colstats)
    cld = n_out if colstats_ld is None else int(colstats_ld)
    if colstats.numel() != (M // 64) * cld * 2 or colstats_col < 0 or colstats_col + n_out > cld:
        raise VcxError(f"colstats must hold [M / 64, {cld}, 2] floats (M={M}, N={n_out}, first column {colstats_col}), got {tuple(colstats.shape)}")
    return colstats.data_ptr() + 8 * int(colstats_col), cld


def _rowstats_arg(rowstats, M):
    _dev32(rowstats)
    if rowstats.numel() != 2 * M or not rowstats.is_contiguous():
        raise VcxError(f"rowstats must hold [M = {M}, 2] floats, got {tuple(rowstats.shape)}")
    return rowstats.data_ptr()


def require_gpu():
    """Raise unless a gfx950 device and the built library are available (no fallback path)."""
    if not torch.cuda.is_available():
        raise VcxError("viewcrafter_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False "
                       "and there is no CPU fallback")
    lib()


# ------------------------------------------------------------------------------------------
# GEMM / convolution
# ------------------------------------------------------------------------------------------
def _gemm_desc(M, N, K, lda, ldc, *, ldw=None, ldr=0, conv=None, tail=(), flags=0, alpha=1.0):
    """The pointer-free part of a vcx_gemm_desc: shape, strides, convolution geometry (`conv`, see gemm), K tail as (k, row stride) pairs,
    flags.  gemm() / gemm_units() add their pointers to it; the *_ok predicates below send it to vcx_gemm_route as it is, so what they
    ask about is the descriptor the launcher would get."""
    ldw = K if ldw is None else ldw
    if max(M, N, K, ldw, ldc, ldr, conv["in_w"] if conv else 0) >= 1 << 31:      # ctypes would truncate them silently
        raise VcxError(f"gemm: M={M} N={N} K={K} ldw={ldw} ldc={ldc} ldr={ldr} do not fit the descriptor's 32-bit fields")
    d = GemmDesc()
    d.lda, d.M, d.N, d.K, d.ldw, d.ldc, d.ldr = lda, M, N, K, ldw, ldc, ldr
    if conv is not None:
        d.mode = 1
        d.in_h, d.in_w, d.out_h, d.out_w = conv["in_h"], conv["in_w"], conv["out_h"], conv["out_w"]
        d.cin, d.kh, d.kw = conv["cin"], conv["kh"], conv["kw"]
        d.stride, d.pad_h, d.pad_w, d.ups = conv["stride"], conv["pad_h"], conv["pad_w"], conv.get("ups", 0)
        if conv.get("slabk", conv_slab_major(conv["cin"], conv["kh"] * conv["kw"])):     # the order pack_conv() produced
            flags |= GEMM_CONV_SLABK
    for j, (k, ld) in zip("01", tail):
        setattr(d, "tail_k" + j, k)
        setattr(d, "tail_lda" + j, ld)
    d.flags, d.alpha = flags, alpha
    return d


def _takes(M, N, K, lda, ldc, unit_rows=0, **kw):
    """Does a kernel take the call _gemm_desc(...) describes - vcx_gemm_f16, or vcx_gemm_units_f16 with unit_rows > 0 - with every
    by-product its flags ask for?  The dispatcher's own answer (vcx_gemm_route): it refuses a flag that the route's kernel does not have."""
    try:
        return lib().vcx_gemm_route(ctypes.byref(_gemm_desc(M, N, K, lda, ldc, **kw)), unit_rows) > 0
    except VcxError:          # a size beyond the descriptor's fields
        return False


def gemm(a, w, *, M, N, K, lda, out=None, ldc=None, bias=None, bias_m=False, residual=None, ldr=None, rowadd=None,
         rowadd_div=0, geglu=False, out_f32=False, alpha=1.0, conv=None, ldw=None, ln_stats=None, ln_colsum=None, ln_t=False, colstats=None,
         colstats_ld=None, colstats_col=0, rowstats=None, rowstats_eps=1e-5, tail=None):
    """out[M, N] = epilogue(alpha * X W^T); see include/vcx.h.  `conv` = dict(in_h, in_w, out_h, out_w, cin, kh, kw,
    stride, pad_h, pad_w, ups) switches X to the im2col gather of a channels-last image.  `ln_stats` (from row_stats) +
    `ln_colsum` select the folded-LayerNorm epilogue (VCX_GEMM_LNFOLD; `ln_t`: the normalised rows are the W operand).
    `colstats` (fp32 [M / 64, N, 2], see colstats_buffer) makes the layer write the column moments of its output for the
    GroupNorm behind it (VCX_GEMM_COLSTATS); with `colstats_ld` / `colstats_col` the buffer is [M / 64, colstats_ld, 2] and this
    call fills the columns [colstats_col, colstats_col + N) - the moments of a tensor that is one part of a channel concat.
    `rowstats` (fp32 [M, 2], see rowstats_ok) makes the layer write LayerNorm's (mean, rstd) of its output rows (VCX_GEMM_ROWSTATS).
    `tail`: one or two fp16 tensors [M, k_j] whose rows are the last sum(k_j) K columns of the problem - K then counts them
    (include/vcx.h tail_a0 / tail_a1).  Behind a convolution's taps (see conv_tail_ok), or - without `conv` - behind the K - sum(k_j)
    columns of a: one GEMM over the row-aligned sources [a | tail...], bit for bit the linear layer on their concatenation wherever the
    tiled engine takes that (see linear_tail_ok; linear() counts K itself)."""
    n_out = N // 2 if geglu else N
    _dev16(a, w, residual)
    _dev32(bias, rowadd)
    out, ldc = _out_arg(out, ldc, M, n_out, a, _f32 if out_f32 else _f16)
    if tail and len(tail) > 2:
        raise VcxError("gemm: a K tail has one or two sources")
    for j, t in enumerate(tail or ()):
        if t.dim() != 2 or t.shape[0] != M or t.stride(1) != 1:
            raise VcxError(f"gemm: tail source {j} must be [M = {M}, k] with unit column stride, got {tuple(t.shape)}")
    d = _gemm_desc(M, N, K, lda, ldc, ldw=ldw, conv=conv, tail=[(t.shape[1], t.stride(0)) for t in tail or ()], alpha=alpha)
    d.A, d.W, d.C = a.data_ptr(), w.data_ptr(), out.data_ptr()
    flags = d.flags
    if bias is not None:
        d.bias = bias.data_ptr()
        flags |= GEMM_BIAS_M if bias_m else GEMM_BIAS_N
    if rowadd is not None:
        if rowadd.dim() != 2 or rowadd.stride(1) != 1 or rowadd.shape[1] != n_out:
            raise VcxError(f"rowadd must be [rows, N = {n_out}] fp32 with unit column stride (a column slice of a wider matrix is fine), got {tuple(rowadd.shape)}")
        d.rowadd = rowadd.data_ptr()
        d.rowadd_div = rowadd_div
        d.rowadd_ld = rowadd.stride(0) if rowadd.shape[0] > 1 else n_out
        flags |= GEMM_ROWADD
    if residual is not None:
        d.residual = residual.data_ptr()
        d.ldr = ldr if ldr is not None else residual.stride(0)
        flags |= GEMM_RESIDUAL
    if geglu:
        flags |= GEMM_GEGLU
    if out_f32:
        flags |= GEMM_OUT_F32
    if ln_stats is not None:
        _dev32(ln_stats, ln_colsum)
        d.ln_stats, d.ln_colsum = ln_stats.data_ptr(), ln_colsum.data_ptr()
        flags |= GEMM_LNFOLD_T if ln_t else GEMM_LNFOLD
    if colstats is not None:
        d.colstats, d.ldcs = _colstats_arg(colstats, colstats_ld, colstats_col, M, n_out)
        flags |= GEMM_COLSTATS
    if rowstats is not None:
        d.rowstats, d.rowstats_eps = _rowstats_arg(rowstats, M), float(rowstats_eps)
        flags |= GEMM_ROWSTATS
    if tail:
        _dev16(*tail)
        d.tail_a0 = tail[0].data_ptr()
        if len(tail) > 1:
            d.tail_a1 = tail[1].data_ptr()
    d.flags = flags
    check(lib().vcx_gemm_f16(ctypes.byref(d), _stream()), "vcx_gemm_f16")
    return out


def rowstats_ok(M, N, K, *, lda=None, ldc=None, ldr=0, unit_rows=None, video_rows=None):
    """Will the layer producing an [M, N] output - vcx_gemm_f16 (bias / residual at most), or vcx_gemm_units_f16 with `unit_rows` rows per
    weight set - write LayerNorm's row statistics of its output (VCX_GEMM_ROWSTATS)?  Only the pipelined weight-stationary kernel has
    that epilogue; whether it takes the flagged call is the dispatcher's answer (vcx_gemm_route).  Elsewhere the consumer makes its
    statistics pass (row_stats).
    The epilogue's statistics and row_stats agree to rounding, not bit for bit, so a row's route must not depend on the batch it runs
    in.  That is this function's own rule: the dispatcher is asked about ONE video alone (`video_rows` rows, default M), with per-unit
    weights also about two videos - the smallest batch, where a video may be one unit among several and other conditions hold - and
    about the call itself; all must be taken.  Only the 4 GiB extents then depend on the whole call."""
    per_video = M if video_rows is None else video_rows
    if not LN_ROWSTATS or M < per_video:
        return False
    flags = GEMM_ROWSTATS | GEMM_BIAS_N | (GEMM_RESIDUAL if ldr else 0)
    lda, ldc = K if lda is None else lda, N if ldc is None else ldc
    calls = {per_video, M} | ({2 * per_video} if unit_rows else set())
    return all(_takes(m, N, K, lda, ldc, unit_rows or 0, ldr=ldr, flags=flags) for m in sorted(calls))


def rowstats_buffer(M, device):
    return torch.empty((M, 2), dtype=_f32, device=device)


def gemm_units(a, wn, bn, *, unit_rows, out=None, rowstats=None, rowstats_eps=1e-5):
    """out[M, N] = a[M, K] Wn[u]^T + bn[u] for the rows of unit u = m // unit_rows: wn [units, N, K] fp16, bn [units, N] fp32 (the
    sets of group_norm_fold_linear).  One launch of the weight-stationary kernel at N = K = 320, one plan of the tiled engine (at most two
    launches, tiles counted per unit) wherever its DMA kernel takes the shape, else unit by unit - units_route below, include/vcx.h.
    The tiled form and the unit-by-unit loop give the same bits.  `rowstats`: as in gemm (the weight-stationary one-launch form, or a
    single unit; see rowstats_ok)."""
    M, K = a.shape
    units, N, K2 = wn.shape
    _dev16(a, wn, out)
    _dev32(bn)
    if K2 != K or M != units * unit_rows or tuple(bn.shape) != (units, N) or not wn.is_contiguous() or not bn.is_contiguous():
        raise VcxError(f"gemm_units: a {tuple(a.shape)} / wn {tuple(wn.shape)} / bn {tuple(bn.shape)} do not describe {units} units of {unit_rows} rows")
    out, ldc = _out_arg(out, None, M, N, a)
    d = _gemm_desc(M, N, K, a.stride(0), ldc, flags=GEMM_BIAS_N)
    d.A, d.W, d.C, d.bias = a.data_ptr(), wn.data_ptr(), out.data_ptr(), bn.data_ptr()
    if rowstats is not None:
        d.rowstats, d.rowstats_eps = _rowstats_arg(rowstats, M), float(rowstats_eps)
        d.flags |= GEMM_ROWSTATS
    check(lib().vcx_gemm_units_f16(ctypes.byref(d), int(unit_rows), N * K, N, _stream()), "vcx_gemm_units_f16")
    return out


def units_route(M, N, K, unit_rows, *, lda=None, ldc=None):
    """The route vcx_gemm_units_f16 takes for M rows in units of unit_rows, as its dispatcher says (vcx_gemm_route; knobs and
    VCX_GEMM_UNITS_LOOP as they are at the time of the call): "single" (one unit: vcx_gemm_f16's call), "ws320" (one launch of the
    weight-stationary kernel, N = K = 320), "grouped" (the tiled engine's per-unit form: one plan for all units) or "loop" (vcx_gemm_f16
    unit by unit)."""
    if unit_rows <= 0 or M <= 0 or M % unit_rows != 0:
        raise VcxError(f"units_route: M ({M}) must be a whole number of units of {unit_rows} rows")
    d = _gemm_desc(M, N, K, K if lda is None else lda, N if ldc is None else ldc, flags=GEMM_BIAS_N)
    route = lib().vcx_gemm_route(ctypes.byref(d), unit_rows)
    if route <= 0:
        raise VcxError("units_route: " + lib().vcx_last_error().decode("utf-8", "replace"))
    return {ROUTE_UNITS_WS320: "ws320", ROUTE_UNITS_GROUPED: "grouped", ROUTE_UNITS_LOOP: "loop"}.get(route, "single")


def units_one_launch_ok(M, N, K, unit_rows, *, lda=None, ldc=None):
    """Does vcx_gemm_units_f16 run all units of the call under ONE tile plan (the weight-stationary launch or the tiled engine's per-unit
    form) instead of once per unit?  (units_route; like lnfold_ok, callers use it to decide a fold whose cost is a launch per unit.)"""
    return units_route(M, N, K, unit_rows, lda=lda, ldc=ldc) in ("ws320", "grouped")


def lnfold_ok(rows, n_out, K, *, lda=None, ldc=None, transposed=False):
    """Will vcx_gemm_f16 take a folded-LayerNorm projection (VCX_GEMM_LNFOLD / _T) of `rows` token rows x K channels onto n_out
    outputs?  The epilogue exists in the DMA kernels only; the dispatcher says whether one of them takes the call (vcx_gemm_route).
    Where it says no - a longer clip or a larger frame than any shipped config - the caller runs layer_norm + the plain projection, as
    before the fold existed, instead of getting VCX_EINVAL from every transformer block."""
    lda = K if lda is None else lda
    if transposed:          # LNFOLD_T puts the weight rows on M, the token rows are the W operand
        return _takes(n_out, rows, K, K, rows if ldc is None else ldc, ldw=lda, flags=GEMM_LNFOLD_T | GEMM_BIAS_M)
    return _takes(rows, n_out, K, lda, n_out if ldc is None else ldc, flags=GEMM_LNFOLD | GEMM_BIAS_N)


def linear(x, w, bias=None, **kw):
    """x [rows, K] (row stride may exceed K) times w [N, K]^T.  tail=[t...]: [x | t...] times w [N, K + sum(k_j)]^T (gemm, linear_tail_ok)."""
    rows, K = x.shape
    K += sum(t.shape[1] for t in kw.get("tail") or ())
    return gemm(x, w, M=rows, N=w.shape[0], K=K, lda=x.stride(0), bias=bias, **kw)


def linear_tail_ok(M, N, K, tail_ks, lda=None, ldc=None, residual=False, colstats=False):
    """Will vcx_gemm_f16 take the linear layer [a | tail...] W^T - K main columns from a, then a K tail of widths tail_ks - with a bias,
    this residual / column-moment epilogue and these strides (tail sources dense)?  The tiled engine only: the dispatcher's answer
    (vcx_gemm_route) for the descriptor gemm(..., tail=...) would send."""
    if not 0 < len(tail_ks) <= 2 or any(k <= 0 for k in tail_ks):
        return False
    flags = GEMM_BIAS_N | (GEMM_RESIDUAL if residual else 0) | (GEMM_COLSTATS if colstats else 0)
    return _takes(M, N, K + sum(tail_ks), K if lda is None else lda, N if ldc is None else ldc, ldr=N if residual else 0, tail=[(k, k) for k in tail_ks], flags=flags)


def conv2d(x, w, bias, *, kh, kw, stride=1, pad_h=None, pad_w=None, ups=0, out_hw=None, **kwargs):
    """x [n, H, W, Cin] channels-last fp16, w [Cout, kh*kw*Cin] as packed by packing.pack_conv.  Returns [n, Ho, Wo, Cout]."""
    n, H, W, cin = x.shape
    if pad_h is None:
        pad_h = kh // 2
    if pad_w is None:
        pad_w = kw // 2
    if out_hw is None:
        He, We = H << ups, W << ups
        out_hw = ((He + 2 * pad_h - kh) // stride + 1, (We + 2 * pad_w - kw) // stride + 1)
    Ho, Wo = out_hw
    cout = w.shape[0]
    geom = dict(in_h=H, in_w=W, out_h=Ho, out_w=Wo, cin=cin, kh=kh, kw=kw, stride=stride, pad_h=pad_h, pad_w=pad_w,
                ups=ups)
    tail_k = sum(t.shape[1] for t in kwargs.get("tail") or ())
    out = gemm(x, w, M=n * Ho * Wo, N=cout, K=kh * kw * cin + tail_k, lda=x.stride(2), bias=bias, conv=geom, **kwargs)
    return out.view(n, Ho, Wo, -1)


# Upsample convolutions in their folded form (ups = 2, include/vcx.h; round 11).  VCX_UPS_FOLD=0: the nine-tap ups = 1 call everywhere (A/B runs)
UPS_FOLD = os.environ.get("VCX_UPS_FOLD", "1") != "0"


def _ups_folded_desc(n, H, W, cin, cout, lda, ldc, colstats):
    geom = dict(in_h=H, in_w=W, out_h=2 * H, out_w=2 * W, cin=cin, kh=2, kw=2, stride=1, pad_h=1, pad_w=1, ups=2)
    return dict(M=n * 4 * H * W, N=cout, K=4 * cin, lda=lda, ldc=ldc, conv=geom, flags=GEMM_BIAS_N | (GEMM_COLSTATS if colstats else 0))


def conv2d_ups_folded_ok(n, H, W, cin, cout, *, lda=None, ldc=None, colstats=False):
    """Does the library run nearest-2x + 3x3 on an [n, H, W, cin] source in its folded form (four 2x2 weight sets, conv2d_ups_folded)?
    The dispatcher's answer (vcx_gemm_route) for the descriptor that call would send; False also under VCX_UPS_FOLD=0.  Where it says
    no the caller runs conv2d(..., ups=1) on the nine-tap weights."""
    if not UPS_FOLD:
        return False
    d = _ups_folded_desc(n, H, W, cin, cout, cin if lda is None else lda, cout if ldc is None else ldc, colstats)
    return _takes(d.pop("M"), d.pop("N"), d.pop("K"), d.pop("lda"), d.pop("ldc"), **d)


def conv2d_ups_folded(x, wf, bias, *, out=None, ldc=None, colstats=None, colstats_ld=None, colstats_col=0):
    """F.interpolate(x, 2, 'nearest') + 3x3 / padding 1 as four 2x2 convolutions on the source grid: x [n, H, W, Cin] channels-last fp16,
    wf [4, Cout, 4*Cin] as packed by packing.pack_conv_ups_folded.  Returns [n, 2H, 2W, Cout]; out / ldc / colstats* as in gemm.  Shapes:
    conv2d_ups_folded_ok - a shape the folded kernel does not take is an error here, not a fall-back."""
    n, H, W, cin = x.shape
    cout = wf.shape[1]
    if wf.dim() != 3 or wf.shape[0] != 4 or wf.shape[2] != 4 * cin or not wf.is_contiguous():
        raise VcxError(f"conv2d_ups_folded: weights must be contiguous [4, Cout, 4 * {cin}], got {tuple(wf.shape)}")
    geom = _ups_folded_desc(n, H, W, cin, cout, 0, 0, False)["conv"]
    res = gemm(x, wf, M=n * 4 * H * W, N=cout, K=4 * cin, lda=x.stride(2), bias=bias, conv=geom, out=out, ldc=ldc, colstats=colstats,
               colstats_ld=colstats_ld, colstats_col=colstats_col)
    return res.view(n, 2 * H, 2 * W, -1)


def _rows_geom(M, in_rows, cin, taps):
    """Convolution geometry for a route query that knows row counts only: ONE image of in_rows pixels and M outputs, taps x 1 taps."""
    return dict(in_h=1, in_w=M if in_rows is None else in_rows, out_h=1, out_w=M, cin=cin, kh=taps, kw=1, stride=1, pad_h=0, pad_w=0)


def conv_tail_ok(M, cin, cout, taps, tail_ks, in_rows=None):
    """Will vcx_gemm_f16 take a convolution over a cin-channel image with a K tail of widths tail_ks (the 1x1 skip convolution of a
    ResBlock folded into its second convolution)?  The DMA kernel only: the dispatcher's answer (vcx_gemm_route)."""
    return (0 < len(tail_ks) <= 2 and all(k > 0 for k in tail_ks)
            and _takes(M, cout, taps * cin + sum(tail_ks), cin, cout, conv=_rows_geom(M, in_rows, cin, taps), tail=[(k, k) for k in tail_ks]))


def temporal_conv3(x, w, bias, **kwargs):
    """x [B, T, P, C]; (3,1,1) convolution along T with zero padding; w [Cout, 3*Cin] as packed by packing.pack_conv."""
    B, T, P, C = x.shape
    geom = dict(in_h=T, in_w=P, out_h=T, out_w=P, cin=C, kh=3, kw=1, stride=1, pad_h=1, pad_w=0, ups=0)
    out = gemm(x, w, M=B * T * P, N=w.shape[0], K=3 * C, lda=x.stride(2), bias=bias, conv=geom, **kwargs)
    return out.view(B, T, P, -1)


# ------------------------------------------------------------------------------------------
# normalisation
# ------------------------------------------------------------------------------------------
def colstats_ok(M, pixels, cin, cout, in_rows=None):
    """Can the layer producing an [M, cout] output - a convolution over a cin-channel image of in_rows pixels, or a linear layer with
    K = cin - write column moments for a GroupNorm whose statistics span `pixels` consecutive output rows?  (VCX_GEMM_COLSTATS.)
    Whole 64-row strips per statistics unit are the host graph's rule; whether a kernel with that epilogue takes the call is the
    dispatcher's answer (vcx_gemm_route).  A convolution is asked about with one tap: its taps multiply the weight's extent only."""
    return (pixels % 64 == 0 and M % 64 == 0
            and _takes(M, cout, cin, cin, cout, conv=None if in_rows is None else _rows_geom(M, in_rows, cin, 1), flags=GEMM_COLSTATS))


def colstats_buffer(M, cout, device):
    return torch.empty((M // 64, cout, 2), dtype=_f32, device=device)


def group_norm_stats_from_colstats(colstats, n_outer, pixels, C, groups=32):
    """(mean, variance) per (n, group) from the column moments a colstats= convolution wrote: what group_norm(stats=) takes."""
    _dev32(colstats)
    # the moments travel across module boundaries (flow.py, concat targets): a buffer that does not hold exactly the strips of this
    # tensor would be read out of bounds or give silently wrong statistics
    if pixels % 64 != 0 or colstats.numel() != (n_outer * pixels // 64) * C * 2:
        raise VcxError(f"colstats must hold [{n_outer} x {pixels} / 64, {C}, 2] floats with pixels % 64 == 0, got {tuple(colstats.shape)}")
    stats = torch.empty((n_outer, groups, 2), dtype=_f32, device=colstats.device)
    L = lib()
    ws = torch.empty((L.vcx_groupnorm_ws_bytes(n_outer, pixels, groups),), dtype=torch.uint8, device=colstats.device)
    check(L.vcx_groupnorm_stats_from_colstats_f32(colstats.data_ptr(), stats.data_ptr(), ws.data_ptr(), n_outer, pixels, C, groups, _stream()),
          "groupnorm_stats_from_colstats")
    return stats


def group_norm_stats(x, groups=32):
    """(mean, variance) per (n, group) of x [n_outer, pixels, C] fp16: the statistics pass of group_norm on its own."""
    n_outer, pixels, C = x.shape
    _dev16(x)
    L = lib()
    stats = torch.empty((n_outer, groups, 2), dtype=_f32, device=x.device)
    ws = torch.empty((L.vcx_groupnorm_ws_bytes(n_outer, pixels, groups),), dtype=torch.uint8, device=x.device)
    check(L.vcx_groupnorm_stats_f16(x.data_ptr(), stats.data_ptr(), ws.data_ptr(), n_outer, pixels, C, groups, _stream()), "groupnorm_stats")
    return stats


def group_norm_fold_linear(w32, bias, gamma, beta, stats, eps, groups=32):
    """GroupNorm (no SiLU) folded into the linear layer behind it: w32 [N, C] fp32 master weights, stats [n, groups, 2] ->
    (Wn [n, N, C] fp16, bn [n, N] fp32) with Linear(GroupNorm(x_n)) = x_n Wn[n]^T + bn[n] (include/vcx.h)."""
    _dev32(w32, bias, gamma, beta, stats)
    N, C = w32.shape
    n = stats.shape[0]
    if not w32.is_contiguous() or tuple(stats.shape) != (n, groups, 2):
        raise VcxError(f"group_norm_fold_linear: contiguous [N, C] weights and [n, {groups}, 2] statistics expected, got {tuple(w32.shape)} / {tuple(stats.shape)}")
    wn = torch.empty((n, N, C), dtype=_f16, device=w32.device)
    bn = torch.empty((n, N), dtype=_f32, device=w32.device)
    check(lib().vcx_groupnorm_fold_linear_f16(w32.data_ptr(), _ptr(bias), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(), wn.data_ptr(),
                                              bn.data_ptr(), n, N, C, groups, eps, _stream()), "groupnorm_fold_linear")
    return wn, bn


def _group_norm_arg(what, x, x2, gamma, beta, stats, groups, quant, out=None):
    """What group_norm, group_norm_mxfp8 and group_norm_mxfp8_raw (`what`) share: the checks of x [n_outer, pixels, c1] and of the optional
    second half x2 of a channel concat (`quant`: the quantising forms' own - a dense x, whole MX blocks over the concat), the type of a
    caller's `out`, and the statistics pass where `stats` is not handed in.  -> (n_outer, pixels, c1, C, stats)"""
    n_outer, pixels, c1 = x.shape
    C = c1 + (0 if x2 is None else x2.shape[2])
    _dev16(x, x2, out)
    _dev32(gamma, beta, stats)
    if quant and not x.is_contiguous():
        raise VcxError(f"{what}: a contiguous [n_outer, pixels, C] tensor needed")
    if x2 is not None and (stats is None or tuple(x2.shape[:2]) != (n_outer, pixels) or c1 % 8 != 0 or (quant and C % 32 != 0) or not x.is_contiguous()
                           or not x2.is_contiguous()):
        raise VcxError(f"{what} over a split concat needs statistics, contiguous halves{', c1 % 8 == 0 and C % 32 == 0' if quant else ' and c1 % 8 == 0'} "
                       f"(x1 {tuple(x.shape)}, x2 {tuple(x2.shape)})")
    return n_outer, pixels, c1, C, group_norm_stats(x, groups) if stats is None else stats


def group_norm(x, gamma, beta, eps, silu, groups=32, out=None, stats=None, x2=None):
    """x [n_outer, pixels, C] fp16 (contiguous).  Statistics over (pixels, C/groups) - computed here, or handed in (`stats`
    [n_outer, groups, 2] = (mean, variance), from group_norm_stats_from_colstats).  x2 [n_outer, pixels, C2]: the norm runs over the
    channel concat [x | x2] without materialising it (vcx_groupnorm_apply2_f16; `stats` required)."""
    n_outer, pixels, c1, C, stats = _group_norm_arg("group_norm", x, x2, gamma, beta, stats, groups, False, out)
    rest = (stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), n_outer, pixels, C, groups, eps, 1 if silu else 0, _stream())
    if x2 is None:
        out = torch.empty_like(x) if out is None else out
        check(lib().vcx_groupnorm_apply_f16(x.data_ptr(), out.data_ptr(), *rest), "groupnorm_apply")
    else:
        out = torch.empty((n_outer, pixels, C), dtype=_f16, device=x.device) if out is None else out
        check(lib().vcx_groupnorm_apply2_f16(x.data_ptr(), c1, x2.data_ptr(), out.data_ptr(), *rest), "groupnorm_apply2")
    return out


def row_stats(x, eps=1e-5):
    """(mean, rstd) of every row of x [rows, C] fp16 -> [rows, 2] fp32: LayerNorm's statistics for a VCX_GEMM_LNFOLD projection."""
    rows, C = x.shape
    _dev16(x)
    stats = torch.empty((rows, 2), dtype=_f32, device=x.device)
    check(lib().vcx_rowstats_f16(x.data_ptr(), stats.data_ptr(), rows, C, eps, _stream()), "rowstats")
    return stats


def layer_norm(x, gamma, beta, eps=1e-5):
    rows, C = x.shape
    _dev16(x)
    _dev32(gamma, beta)
    out = torch.empty_like(x)
    check(lib().vcx_layernorm_f16(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rows, C, eps,
                                  _stream()), "layernorm")
    return out


POOL_MEAN, POOL_NEAREST = 0, 1      # include/vcx_pool.h VCX_POOL_*


def layer_norm_pool2x2_ok(n, H, W, C, mode):
    """Does vcx_layernorm_pool2x2_f16 take n frames of H x W tokens with C channels in this mode?  The library's answer (no device needed)."""
    return lib().vcx_layernorm_pool2x2_ok(n, H, W, C, mode) == 1


def layer_norm_pool2x2(x, gamma, beta, eps, n, H, W, mode):
    """x [n H W, C] dense token rows, row-major over (frame, y, x) -> [n (H/2) (W/2), C]: avgpool2x2(layer_norm(x) viewed [n, H, W, C]) for
    POOL_MEAN, the rows (2y, 2x) of layer_norm(x) for POOL_NEAREST - byte for byte, in one pass; the normalised rows are never written."""
    rows, C = x.shape
    _dev16(x)
    _dev32(gamma, beta)
    if rows != n * H * W or not x.is_contiguous():
        raise VcxError(f"layer_norm_pool2x2: dense rows [n H W, C] needed (rows={rows} n={n} H={H} W={W})")
    out = torch.empty((n * (H // 2) * (W // 2), C), dtype=_f16, device=x.device)
    check(lib().vcx_layernorm_pool2x2_f16(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), n, H, W, C, eps, mode, _stream()),
          "layernorm_pool2x2")
    return out


# ------------------------------------------------------------------------------------------
# MXFP8 operands (include/vcx.h "MXFP8 operands"; opt-in: the GEGLU feed-forward under VCX_FF_MXFP8=1, the TemporalConvBlock convolutions
# under VCX_TCONV_MXFP8=1, the ResBlock 3x3 convolutions under VCX_RESCONV_MXFP8=1)
# ------------------------------------------------------------------------------------------
_u8 = torch.uint8


def mx_kp(K):
    """K extent of an MXFP8 buffer: K rounded up to a multiple of 128."""
    return (K + 127) // 128 * 128


def _mx_buffers(rows, K, device):
    kp = mx_kp(K)
    return torch.empty((rows, kp), dtype=_u8, device=device), torch.empty((rows, kp // 32), dtype=_u8, device=device)


def _mx_weight_arg(pair, rows, k_bytes, what):
    """An MXFP8 pair with rows of k_bytes element bytes (a convolution's weight rows: its taps, each padded on its own, and its tail)."""
    for t, shape in zip(pair, ((rows, k_bytes), (rows, k_bytes // 32))):
        if t.dtype is not _u8 or not t.is_cuda or tuple(t.shape) != shape or not t.is_contiguous():
            raise VcxError(f"{what}: expected contiguous GPU uint8 {shape}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def _dev_mx(pair, rows, K, what):
    _mx_weight_arg(pair, rows, mx_kp(K), what)


def _mx_bias_residual_arg(bias, residual, ldr, M, n_out, what, bias_n=None):
    """The bias every MXFP8 GEMM entry point requires (bias_n entries where that is not n_out: packed GEGLU columns) and its optional
    residual [M, n_out]; -> ldr (the residual's row stride where not given, 0 without a residual or a value)."""
    bias_n = n_out if bias_n is None else bias_n
    _dev32(bias)
    _dev16(residual)
    if bias is None or bias.numel() != bias_n or not bias.is_contiguous():
        raise VcxError(f"{what}: a contiguous fp32 bias [N = {bias_n}] is required")
    if residual is None:
        return ldr or 0
    if tuple(residual.shape) != (M, n_out) or residual.stride(1) != 1:
        raise VcxError(f"{what}: residual must be [{M}, {n_out}] with unit column stride, got {tuple(residual.shape)}")
    return residual.stride(0) if ldr is None else ldr


def quant_mxfp8(x):
    """x [rows, K] fp16 (row stride may exceed K) -> (element bytes [rows, Kp], scale bytes [rows, Kp / 32])."""
    rows, K = x.shape
    _dev16(x)
    if x.stride(1) != 1:
        raise VcxError("quant_mxfp8: unit column stride needed")
    q, s = _mx_buffers(rows, K, x.device)
    check(lib().vcx_quant_mxfp8_f16(x.data_ptr(), x.stride(0), q.data_ptr(), s.data_ptr(), rows, K, _stream()), "quant_mxfp8")
    return q, s


def layer_norm_mxfp8(x, gamma, beta, eps=1e-5):
    """quant_mxfp8(layer_norm(x, gamma, beta, eps)), bit for bit, in one pass: the normalised fp16 rows are never written."""
    rows, C = x.shape
    _dev16(x)
    _dev32(gamma, beta)
    if not x.is_contiguous():
        raise VcxError("layer_norm_mxfp8: dense rows needed")
    q, s = _mx_buffers(rows, C, x.device)
    check(lib().vcx_layernorm_mxfp8_f16(x.data_ptr(), q.data_ptr(), s.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rows, C, eps, _stream()),
          "layernorm_mxfp8")
    return q, s


def _mx_flags(residual=False, geglu=False, mx_out=False):
    return GEMM_BIAS_N | (GEMM_RESIDUAL if residual else 0) | (GEMM_GEGLU if geglu else 0) | (GEMM_MXFP8_OUT if mx_out else 0)


def linear_mxfp8_ok(rows, N, K, *, residual=False, geglu=False, mx_out=False):
    """Does vcx_gemm_mxfp8 take `rows` rows x K onto N (packed, for GEGLU) weight rows with this epilogue?  The library's answer."""
    return lib().vcx_gemm_mxfp8_ok(rows, N, K, _mx_flags(residual, geglu, mx_out)) == 1


def gemm_mxfp8_cfg(N, flags=GEMM_BIAS_N, gather_mode=0):
    """The tile configuration the MXFP8 GEMM kernel runs N output columns with this flag word on: 0 = 128 x 128, 1 = 128 x 160 (N = 160 j).
    gather_mode 0 = linear_mxfp8, 1 = temporal_conv3_mxfp8, 2 = conv3x3_mxfp8.  The launchers' own answer (vcx_gemm_mxfp8_cfg: N, flags and
    the environment variable VCX_GEMM_MX_CFG, no device); both configurations compute the same bytes."""
    cfg = lib().vcx_gemm_mxfp8_cfg(N, flags, gather_mode)
    check(min(cfg, 0), "gemm_mxfp8_cfg")
    return cfg


def linear_mxfp8(a, w, bias, *, K, residual=None, geglu=False, mx_out=False):
    """a, w: (element bytes, scale bytes) pairs of [rows, K] and [N, K] matrices (quant_mxfp8 / layer_norm_mxfp8 / a mx_out=True
    layer; packing.pack_mxfp8).  Returns fp16 [rows, N] = a w^T + bias (+ residual), or with geglu=True (w and bias packed by
    packing.pack_geglu) fp16 [rows, N / 2] = x * gelu(gate) - with mx_out=True that result as an MXFP8 pair, the next layer's operand."""
    rows, N = a[0].shape[0], w[0].shape[0]
    _dev_mx(a, rows, K, "linear_mxfp8 a")
    _dev_mx(w, N, K, "linear_mxfp8 w")
    n_out = N // 2 if geglu else N
    ldr = _mx_bias_residual_arg(bias, residual, None, rows, n_out, "linear_mxfp8", bias_n=N)
    if mx_out and not geglu:
        raise VcxError("linear_mxfp8: mx_out goes with geglu")
    if mx_out:
        out = _mx_buffers(rows, n_out, a[0].device)
        c, cs = out[0].data_ptr(), out[1].data_ptr()
    else:
        out = torch.empty((rows, n_out), dtype=_f16, device=a[0].device)
        c, cs = out.data_ptr(), None
    check(lib().vcx_gemm_mxfp8(a[0].data_ptr(), a[1].data_ptr(), w[0].data_ptr(), w[1].data_ptr(), c, cs, bias.data_ptr(), _ptr(residual), rows, N, K,
                               n_out, ldr, _mx_flags(residual is not None, geglu, mx_out), _stream()),
          "gemm_mxfp8")
    return out


_ZERO_BIAS = {}      # (entries, device) -> fp32 zeros: the bias vcx_gemm_mxfp8 wants where the layer has none (linear_t_mxfp8)


def _zero_bias(n, device):
    key = (n, str(device))
    if key not in _ZERO_BIAS:
        _ZERO_BIAS[key] = torch.zeros(n, dtype=torch.float32, device=device)
    return _ZERO_BIAS[key]


def linear_t_mxfp8_ok(tokens, D, K):
    """Does linear_t_mxfp8 take `tokens` activation rows x K onto D weight rows?  vcx_gemm_mxfp8 with the operands swapped: the library's
    answer for M = D, N = tokens, plus the tile overreach of the token side, which the library guards for its M side only - the column
    tiles reach up to 127 rows past `tokens`, and those 32-bit offsets must not wrap back into the buffer."""
    return tokens % 8 == 0 and (tokens + 127) * mx_kp(K) < (1 << 32) and lib().vcx_gemm_mxfp8_ok(D, tokens, K, _mx_flags()) == 1


def linear_t_mxfp8(x, w, *, K):
    """The transposed projection fp16 [D, tokens] = w x^T (V^T of the spatial self-attention) of MXFP8 pairs x [tokens, K], w [D, K]:
    linear_mxfp8(x, w, 0) transposed, bit for bit.  vcx_gemm_mxfp8 is symmetric in its operands, so this is that call with the weight
    pair as `a` and a cached zero bias of `tokens` entries (the bias is per output column); no kernel of its own."""
    tokens = x[0].shape[0]
    return linear_mxfp8(w, x, _zero_bias(tokens, x[0].device), K=K)


def group_norm_mxfp8(x, gamma, beta, eps, silu, groups=32, stats=None, x2=None):
    """quant_mxfp8(group_norm(x, ...).view(rows, C)), byte for byte, in one pass: the normalised fp16 tensor is never written.
    x [n_outer, pixels, C] fp16 (contiguous, C % 32 == 0); statistics computed here or handed in, as for group_norm.  x2
    [n_outer, pixels, C2]: the norm runs over the channel concat [x | x2] without materialising it (vcx_groupnorm_apply2_mxfp8_f16;
    `stats` required, as for group_norm).
    -> (element bytes [n_outer * pixels, Kp], scale bytes [n_outer * pixels, Kp / 32])."""
    n_outer, pixels, c1, C, stats = _group_norm_arg("group_norm_mxfp8", x, x2, gamma, beta, stats, groups, quant=True)
    q, sc = _mx_buffers(n_outer * pixels, C, x.device)
    rest = (q.data_ptr(), sc.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), n_outer, pixels, C, groups, eps, 1 if silu else 0, _stream())
    if x2 is None:
        check(lib().vcx_groupnorm_apply_mxfp8_f16(x.data_ptr(), *rest), "groupnorm_apply_mxfp8")
    else:
        check(lib().vcx_groupnorm_apply2_mxfp8_f16(x.data_ptr(), c1, x2.data_ptr(), *rest), "groupnorm_apply2_mxfp8")
    return q, sc


def group_norm_mxfp8_raw(x, gamma, beta, eps, silu, groups=32, stats=None, x2=None):
    """group_norm_mxfp8 with a second, raw output from the same pass: -> ((q, scales), (rq, rscales)), the first pair byte for byte
    group_norm_mxfp8's, the second byte for byte quant_mxfp8 of the input rows themselves - with x2 of the channel concat [x | x2], which is
    never materialised (vcx_groupnorm_apply_mxfp8_raw_f16 / vcx_groupnorm_apply2_mxfp8_raw_f16).  The raw pair is the tail operand of
    conv3x3_tail_mxfp8.  Arguments as group_norm_mxfp8 (`stats` required with x2)."""
    n_outer, pixels, c1, C, stats = _group_norm_arg("group_norm_mxfp8_raw", x, x2, gamma, beta, stats, groups, quant=True)
    q, sc = _mx_buffers(n_outer * pixels, C, x.device)
    rq, rsc = _mx_buffers(n_outer * pixels, C, x.device)
    rest = (q.data_ptr(), sc.data_ptr(), rq.data_ptr(), rsc.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), n_outer, pixels, C, groups, eps,
            1 if silu else 0, _stream())
    if x2 is None:
        check(lib().vcx_groupnorm_apply_mxfp8_raw_f16(x.data_ptr(), *rest), "groupnorm_apply_mxfp8_raw")
    else:
        check(lib().vcx_groupnorm_apply2_mxfp8_raw_f16(x.data_ptr(), c1, x2.data_ptr(), *rest), "groupnorm_apply2_mxfp8_raw")
    return (q, sc), (rq, rsc)


def _mx_conv_flags(rowadd, residual, colstats):
    return GEMM_BIAS_N | (GEMM_ROWADD if rowadd else 0) | (GEMM_RESIDUAL if residual else 0) | (GEMM_COLSTATS if colstats else 0)


def _mx_conv_pitches(cout, ldc, residual, ldr, colstats, colstats_ld, colstats_col):
    """(ldc, ldr, ldcs, first moments column) as an MXFP8 convolution's *_ok predicate sends them: the launcher's defaults, 0 for what a call
    without a residual / without moments does not have."""
    return (cout if ldc is None else ldc, (cout if ldr is None else ldr) if residual else 0,
            (cout if colstats_ld is None else colstats_ld) if colstats else 0, colstats_col if colstats else 0)


def _mx_conv_args(what, a, w, bias, M, cin, k_bytes, residual, ldr, out, ldc, colstats, colstats_ld, colstats_col):
    """The checks and defaults the MXFP8 convolution launchers (`what`) share: activation pair [M, cin], weight pair with rows of k_bytes,
    bias, residual, out / ldc, colstats*.  -> (cout, ldr, out, ldc, moments pointer, ldcs)"""
    cout = w[0].shape[0]
    _dev_mx(a, M, cin, what + " a")
    _mx_weight_arg(w, cout, k_bytes, what + " w")
    ldr = _mx_bias_residual_arg(bias, residual, ldr, M, cout, what)
    _dev16(out)
    out, ldc = _out_arg(out, ldc, M, cout, a[0], what=what)
    return (cout, ldr, out, ldc) + _colstats_arg(colstats, colstats_ld, colstats_col, M, cout)


def temporal_conv3_mxfp8_ok(B, T, P, cin, cout, *, residual=False, ldc=None, ldr=None, colstats=False, colstats_ld=None, colstats_col=0):
    """Does vcx_conv_t3_mxfp8 take a (3,1,1) convolution of B videos x T frames x P pixels x cin channels onto cout channels with these
    keywords (those of temporal_conv3_mxfp8: `residual` / `colstats` as booleans, pitches as that call would pass them)?  The library's
    answer - shape, flags, alignment, 32-bit extents; the reason of a refusal is in vcx_last_error()."""
    return lib().vcx_conv_t3_mxfp8_ok(B, T, P, cin, cout, *_mx_conv_pitches(cout, ldc, residual, ldr, colstats, colstats_ld, colstats_col),
                                      _mx_conv_flags(False, residual, colstats)) == 1


def temporal_conv3_mxfp8(a, w, bias, *, B, T, P, cin, residual=None, ldr=None, out=None, ldc=None, colstats=None, colstats_ld=None, colstats_col=0):
    """(3,1,1) convolution along T with zero padding on MXFP8 operands: a = (element bytes, scale bytes) of the activation
    [B * T * P, cin] (group_norm_mxfp8 / quant_mxfp8), w = the pair packing.pack_conv_t3_mxfp8 made of the Conv3d weight.  Returns fp16
    [B, T, P, cout] (or [.., ldc] when written into `out`); residual / out / ldc / colstats* as in gemm.  Shapes: temporal_conv3_mxfp8_ok -
    a call the kernel does not take is an error here, not a fall-back."""
    cout, ldr, out, ldc, cs_ptr, cld = _mx_conv_args("temporal_conv3_mxfp8", a, w, bias, B * T * P, cin, 3 * mx_kp(cin), residual, ldr, out, ldc, colstats,
                                                     colstats_ld, colstats_col)
    check(lib().vcx_conv_t3_mxfp8(a[0].data_ptr(), a[1].data_ptr(), w[0].data_ptr(), w[1].data_ptr(), out.data_ptr(), bias.data_ptr(), _ptr(residual), cs_ptr,
                                  B, T, P, cin, cout, ldc, ldr, cld, _mx_conv_flags(False, residual is not None, colstats is not None), _stream()), "conv_t3_mxfp8")
    return out.view(B, T, P, -1)


def conv3x3_mxfp8_ok(n, H, W, cin, cout, *, rowadd=False, rowadd_div=0, residual=False, ldc=None, ldr=None, colstats=False, colstats_ld=None,
                     colstats_col=0):
    """Does vcx_conv3x3_mxfp8 take a 3x3 / padding-1 convolution of n frames x H x W pixels x cin channels onto cout channels with these
    keywords (those of conv3x3_mxfp8: `rowadd` / `residual` / `colstats` as booleans, pitches as that call would pass them)?  The
    library's answer - shape, flags, alignment, 32-bit extents; the reason of a refusal is in vcx_last_error()."""
    return lib().vcx_conv3x3_mxfp8_ok(n, H, W, cin, cout, *_mx_conv_pitches(cout, ldc, residual, ldr, colstats, colstats_ld, colstats_col),
                                      rowadd_div if rowadd else 0, _mx_conv_flags(rowadd, residual, colstats)) == 1


def conv3x3_mxfp8(a, w, bias, *, n, H, W, cin, rowadd=None, rowadd_div=0, residual=None, ldr=None, out=None, ldc=None, colstats=None,
                  colstats_ld=None, colstats_col=0):
    """3x3 convolution with zero padding 1 on MXFP8 operands: a = (element bytes, scale bytes) of the channels-last activation
    [n * H * W, cin] (group_norm_mxfp8 / quant_mxfp8), w = the pair packing.pack_conv3x3_mxfp8 made of the Conv2d weight.  Returns fp16
    [n, H, W, cout] (or [.., ldc] when written into `out`); rowadd / rowadd_div / residual / out / ldc / colstats* as in gemm.  Shapes:
    conv3x3_mxfp8_ok - a call the kernel does not take is an error here, not a fall-back."""
    M = n * H * W
    cout, ldr, out, ldc, cs_ptr, cld = _mx_conv_args("conv3x3_mxfp8", a, w, bias, M, cin, 9 * mx_kp(cin), residual, ldr, out, ldc, colstats, colstats_ld,
                                                     colstats_col)
    rld = 0
    if rowadd is not None:
        _dev32(rowadd)
        if rowadd.dim() != 2 or rowadd.stride(1) != 1 or rowadd.shape[1] != cout or rowadd_div <= 0 or rowadd.shape[0] * rowadd_div < M:
            raise VcxError(f"conv3x3_mxfp8: rowadd must be [>= M / rowadd_div rows, N = {cout}] fp32 with unit column stride and rowadd_div > 0, "
                           f"got {tuple(rowadd.shape)}, rowadd_div={rowadd_div}, M={M}")
        rld = rowadd.stride(0) if rowadd.shape[0] > 1 else cout
    check(lib().vcx_conv3x3_mxfp8(a[0].data_ptr(), a[1].data_ptr(), w[0].data_ptr(), w[1].data_ptr(), out.data_ptr(), bias.data_ptr(), _ptr(rowadd),
                                  _ptr(residual), cs_ptr, n, H, W, cin, cout, ldc, ldr, cld, rld, rowadd_div if rowadd is not None else 0,
                                  _mx_conv_flags(rowadd is not None, residual is not None, colstats is not None), _stream()), "conv3x3_mxfp8")
    return out.view(n, H, W, -1)


def conv3x3_tail_mxfp8_ok(n, H, W, cin, ct, cout, *, rowadd=False, residual=False, bias=True, ldc=None, colstats=False, colstats_ld=None, colstats_col=0):
    """Does vcx_conv3x3_tail_mxfp8 take a 3x3 / padding-1 convolution of n frames x H x W pixels x cin channels plus a 1x1 convolution of
    a ct-channel tail onto cout channels with these keywords (those of conv3x3_tail_mxfp8, `colstats` as a boolean)?  `rowadd` / `residual`
    / `bias` exist to be asked about: the tailed form refuses a row addend, a residual and a missing bias.  The library's answer - shape,
    flags, alignment, 32-bit extents; the reason of a refusal is in vcx_last_error()."""
    ldc, _, ldcs, col = _mx_conv_pitches(cout, ldc, False, None, colstats, colstats_ld, colstats_col)
    flags = _mx_conv_flags(rowadd, residual, colstats) & ~(0 if bias else GEMM_BIAS_N)
    return lib().vcx_conv3x3_tail_mxfp8_ok(n, H, W, cin, ct, cout, ldc, ldcs, col, flags) == 1


def conv3x3_tail_mxfp8(a, tail, w, bias, *, n, H, W, cin, ct, out=None, ldc=None, colstats=None, colstats_ld=None, colstats_col=0):
    """conv3x3_mxfp8 with a 1x1 convolution of a second MXFP8 source as a linear K tail - a ResBlock's second convolution and its skip
    convolution in one accumulation: a = the pair of the activation [n * H * W, cin], tail = the pair of the block input [n * H * W, ct]
    (group_norm_mxfp8_raw's second output), w = the pair packing.pack_conv3x3_tail_mxfp8 made of the two weights, bias = the two biases
    summed.  Returns fp16 [n, H, W, cout] (or [.., ldc] when written into `out`); out / ldc / colstats* as in conv3x3_mxfp8; no rowadd, no
    residual.  Shapes: conv3x3_tail_mxfp8_ok - a call the kernel does not take is an error here, not a fall-back."""
    _dev_mx(tail, n * H * W, ct, "conv3x3_tail_mxfp8 tail")
    cout, _, out, ldc, cs_ptr, cld = _mx_conv_args("conv3x3_tail_mxfp8", a, w, bias, n * H * W, cin, 9 * mx_kp(cin) + mx_kp(ct), None, None, out, ldc, colstats,
                                                   colstats_ld, colstats_col)
    check(lib().vcx_conv3x3_tail_mxfp8(a[0].data_ptr(), a[1].data_ptr(), tail[0].data_ptr(), tail[1].data_ptr(), w[0].data_ptr(), w[1].data_ptr(),
                                       out.data_ptr(), bias.data_ptr(), cs_ptr, n, H, W, cin, ct, cout, ldc, cld,
                                       _mx_conv_flags(False, False, colstats is not None), _stream()), "conv3x3_tail_mxfp8")
    return out.view(n, H, W, -1)


# ------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------
ATTN_ACCUMULATE, ATTN_LOG2_LOGITS, ATTN_CAUSAL = 1, 2, 4
LOG2E = 1.4426950408889634


def flash_attn(q, k, vt, out, *, n_groups, heads, nq, nk, kv_rows, kv_div, ldq, ldk, ldvt, ldo, scale, accumulate=False,
               log2_logits=False):
    """softmax(scale Q K^T) V per (group, head); `log2_logits`: Q K^T already is the base-2 logit (scale * log2 e was folded
    into the projections, e.g. as the GEMM alpha) and `scale` is ignored."""
    flags = (ATTN_ACCUMULATE if accumulate else 0) | (ATTN_LOG2_LOGITS if log2_logits else 0)
    _dev16(q, k, vt, out)
    check(lib().vcx_attn_flash_d64_f16(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), n_groups, heads, nq,
                                       nk, kv_rows, kv_div, ldq, ldk, ldvt, ldo, scale, flags,
                                       _stream()), "attn_flash_d64")
    return out


def flash_attn_d512(q, k, vt, out, *, n_groups, nq, nk, kv_rows, ldq, ldk, ldvt, ldo, scale):
    """softmax(scale Q K^T) V per group with ONE head of dim 512 (VAE AttnBlock); K rows / V^T columns of group g start at g * kv_rows."""
    _dev16(q, k, vt, out)
    check(lib().vcx_attn_flash_d512_f16(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), n_groups, nq, nk, kv_rows, ldq, ldk, ldvt, ldo,
                                        scale, _stream()), "attn_flash_d512")
    return out


def flash_attn_dual(q, k1, vt1, k2, vt2, out, *, n_groups, heads, nq, nk1, kv_rows1, kv_div1, ldk1, ldvt1, nk2, kv_rows2, kv_div2,
                    ldk2, ldvt2, ldq, ldo, scale, log2_logits=False):
    """softmax(scale Q K1^T) V1 + softmax(scale Q K2^T) V2 in one pass over Q and O (text (+) image cross-attention)."""
    _dev16(q, k1, vt1, k2, vt2, out)
    check(lib().vcx_attn_flash_dual_d64_f16(q.data_ptr(), k1.data_ptr(), vt1.data_ptr(), k2.data_ptr(), vt2.data_ptr(),
                                            out.data_ptr(), n_groups, heads, nq, nk1, kv_rows1, kv_div1, ldk1, ldvt1, nk2,
                                            kv_rows2, kv_div2, ldk2, ldvt2, ldq, ldo, scale,
                                            ATTN_LOG2_LOGITS if log2_logits else 0, _stream()), "attn_flash_dual_d64")
    return out


def flash_attn_mxfp8_ok(*, n_groups, heads, nq, nk, kv_rows, kv_div, ldq, ldk, ldvt, log2_logits=True, accumulate=False):
    """Does vcx_attn_flash_d64_mxfp8 take this geometry, these pitches and flags?  The library's answer (no device needed)."""
    flags = (ATTN_ACCUMULATE if accumulate else 0) | (ATTN_LOG2_LOGITS if log2_logits else 0)
    return lib().vcx_attn_flash_d64_mxfp8_ok(n_groups, heads, nq, nk, kv_rows, kv_div, ldq, ldk, ldvt, flags) == 1


def flash_attn_mxfp8(q, k, vt, *, n_groups, heads, nq, nk, kv_rows, kv_div, ldq, ldk, ldvt, scale=1.0, log2_logits=True):
    """quant_mxfp8(flash_attn(q, k, vt, ...) with ldo = 64 heads), byte for byte, in one pass: the fp16 attention output is never written.
    Returns (element bytes [n_groups * nq, Kp(64 heads)], scale bytes [n_groups * nq, Kp / 32]), the a operand of linear_mxfp8.  Base-2
    logits only (include/vcx.h)."""
    _dev16(q, k, vt)
    oq, os_ = _mx_buffers(n_groups * nq, 64 * heads, q.device)
    check(lib().vcx_attn_flash_d64_mxfp8(q.data_ptr(), k.data_ptr(), vt.data_ptr(), oq.data_ptr(), os_.data_ptr(), n_groups, heads, nq, nk, kv_rows,
                                         kv_div, ldq, ldk, ldvt, scale, ATTN_LOG2_LOGITS if log2_logits else 0, _stream()), "attn_flash_d64_mxfp8")
    return oq, os_


def flash_attn_dual_mxfp8_ok(*, n_groups, heads, nq, nk1, kv_rows1, kv_div1, ldk1, ldvt1, nk2, kv_rows2, kv_div2, ldk2, ldvt2, ldq,
                             log2_logits=True):
    """Does vcx_attn_flash_dual_d64_mxfp8 take the call (it has no first-form resident kernel: knob XATTN_RESIDENT = 2)?  The library's answer."""
    return lib().vcx_attn_flash_dual_d64_mxfp8_ok(n_groups, heads, nq, nk1, kv_rows1, kv_div1, ldk1, ldvt1, nk2, kv_rows2, kv_div2, ldk2, ldvt2, ldq,
                                                  ATTN_LOG2_LOGITS if log2_logits else 0) == 1


def flash_attn_dual_mxfp8(q, k1, vt1, k2, vt2, *, n_groups, heads, nq, nk1, kv_rows1, kv_div1, ldk1, ldvt1, nk2, kv_rows2, kv_div2, ldk2, ldvt2,
                          ldq, scale=1.0, log2_logits=True):
    """quant_mxfp8(flash_attn_dual(...) with ldo = 64 heads), byte for byte, in one pass; returns the MXFP8 pair as flash_attn_mxfp8."""
    _dev16(q, k1, vt1, k2, vt2)
    oq, os_ = _mx_buffers(n_groups * nq, 64 * heads, q.device)
    check(lib().vcx_attn_flash_dual_d64_mxfp8(q.data_ptr(), k1.data_ptr(), vt1.data_ptr(), k2.data_ptr(), vt2.data_ptr(), oq.data_ptr(), os_.data_ptr(),
                                              n_groups, heads, nq, nk1, kv_rows1, kv_div1, ldk1, ldvt1, nk2, kv_rows2, kv_div2, ldk2, ldvt2, ldq, scale,
                                              ATTN_LOG2_LOGITS if log2_logits else 0, _stream()), "attn_flash_dual_d64_mxfp8")
    return oq, os_


def temporal_attn(qkv, out, *, B, T, P, heads, ld, k_off, v_off, ldo, scale, causal=False):
    """causal: frame t attends to frames <= t (TemporalTransformer(causal_attention=True), reference attention.py:343-345, 377-384)."""
    _dev16(qkv, out)
    if causal:
        check(lib().vcx_attn_temporal_d64_masked_f16(qkv.data_ptr(), out.data_ptr(), B, T, P, heads, ld, k_off, v_off, ldo, scale, ATTN_CAUSAL,
                                                     _stream()), "attn_temporal_d64(causal)")
    else:
        check(lib().vcx_attn_temporal_d64_f16(qkv.data_ptr(), out.data_ptr(), B, T, P, heads, ld, k_off, v_off, ldo, scale,
                                              _stream()), "attn_temporal_d64")
    return out


def temporal_attn_mxfp8_ok(B, T, P, heads, ld, causal=False):
    """Does vcx_attn_temporal_d64_mxfp8 take B videos x T frames x P pixels x heads with qkv row pitch ld?  The library's answer."""
    return lib().vcx_attn_temporal_d64_mxfp8_ok(B, T, P, heads, ld, ATTN_CAUSAL if causal else 0) == 1


def temporal_attn_mxfp8(qkv, *, B, T, P, heads, ld, k_off, v_off, scale, causal=False):
    """quant_mxfp8(temporal_attn(qkv, ...) with ldo = 64 heads), byte for byte, in one pass: the fp16 attention output is never written.
    Returns (element bytes [B * T * P, Kp(64 heads)], scale bytes [B * T * P, Kp / 32]), the a operand of linear_mxfp8.  T <= 32, no
    relative position (include/vcx.h)."""
    _dev16(qkv)
    q, s = _mx_buffers(B * T * P, 64 * heads, qkv.device)
    check(lib().vcx_attn_temporal_d64_mxfp8(qkv.data_ptr(), q.data_ptr(), s.data_ptr(), B, T, P, heads, ld, k_off, v_off, scale,
                                            ATTN_CAUSAL if causal else 0, _stream()), "attn_temporal_d64_mxfp8")
    return q, s


def temporal_attn_rel(qkv, out, relg, relp, *, R, B, T, P, heads, ld, k_off, v_off, ldo, scale, causal=False):
    """Temporal attention with relative position (reference attention.py:104-108, 120-123): relg [tokens, heads, 64] = q Ek^T is added to the
    logits, relp [tokens, heads, 64] (zeroed by the caller) receives the probabilities by clipped distance; see include/vcx.h."""
    _dev16(qkv, out, relg, relp)
    check(lib().vcx_attn_temporal_d64_rel_f16(qkv.data_ptr(), out.data_ptr(), relg.data_ptr(), relp.data_ptr(), int(R), B, T, P, heads, ld, k_off, v_off,
                                              ldo, scale, ATTN_CAUSAL if causal else 0, _stream()), "attn_temporal_d64(rel)")
    return out


def softmax_rows_(x, n=None):
    rows = x.shape[0]
    check(lib().vcx_softmax_rows_f16(x.data_ptr(), rows, n if n is not None else x.shape[1], x.stride(0), _stream()),
          "softmax_rows")
    return x


# ------------------------------------------------------------------------------------------
# element-wise / layout
# ------------------------------------------------------------------------------------------
def silu_f32(x):
    out = torch.empty_like(x)
    check(lib().vcx_silu_f32(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "silu")
    return out


def gelu_(x):
    """exact-erf GELU in place on a contiguous fp16 tensor (nn.GELU)."""
    check(lib().vcx_gelu_f16(x.data_ptr(), x.data_ptr(), x.numel(), _stream()), "gelu")
    return x


def clip_preprocess(x, size, antialias, mean, std):
    """x fp32 [B, C, H, W] in [-1, 1] -> fp32 [B, C, size, size]: kornia-style anti-aliased bicubic resize, (x + 1) / 2, CLIP
    mean / std (reference condition.py:322-329) in one kernel."""
    x = x.contiguous()
    _dev32(x)
    B, C, H, W = x.shape
    out = torch.empty((B, C, size, size), dtype=_f32, device=x.device)
    m = (ctypes.c_float * C)(*[float(v) for v in mean])
    s = (ctypes.c_float * C)(*[float(v) for v in std])
    check(lib().vcx_clip_preprocess_f32(x.data_ptr(), out.data_ptr(), B, C, H, W, int(size), 1 if antialias else 0, m, s, _stream()),
          "clip_preprocess")
    return out


def timestep_embedding(t, dim, max_period=10000.0):
    t = t.to(torch.int64).contiguous()
    out = torch.empty((t.shape[0], dim), dtype=_f32, device=t.device)
    check(lib().vcx_timestep_embedding_f32(t.data_ptr(), out.data_ptr(), t.shape[0], dim, max_period, _stream()),
          "timestep_embedding")
    return out


def to_f16(x):
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=_f16, device=x.device)
    check(lib().vcx_cast_f32_to_f16(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "cast_f32_to_f16")
    return out


def to_f32(x):
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=_f32, device=x.device)
    check(lib().vcx_cast_f16_to_f32(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "cast_f16_to_f32")
    return out


def copy2d(src, dst, rows, cols, lds, ldd):
    check(lib().vcx_copy2d_f16(src.data_ptr(), dst.data_ptr(), rows, cols, lds, ldd, _stream()), "copy2d")


def avgpool2x2(x):
    """[n, H, W, C] fp16 channels-last -> [n, H // 2, W // 2, C]: AvgPool2d(2, 2) (reference Downsample(use_conv=False), openaimodel3d.py:70-72)."""
    n, H, W, C = x.shape
    x = x.contiguous()
    out = torch.empty((n, H // 2, W // 2, C), dtype=_f16, device=x.device)
    check(lib().vcx_avgpool2x2_f16(x.data_ptr(), out.data_ptr(), n, H, W, C, _stream()), "avgpool2x2")
    return out


def upsample2x(x):
    """[n, H, W, C] fp16 channels-last -> [n, 2H, 2W, C]: F.interpolate(scale_factor=2, mode='nearest') (reference Upsample, openaimodel3d.py:98-103)."""
    n, H, W, C = x.shape
    x = x.contiguous()
    out = torch.empty((n, 2 * H, 2 * W, C), dtype=_f16, device=x.device)
    check(lib().vcx_upsample2x_f16(x.data_ptr(), out.data_ptr(), n, H, W, C, _stream()), "upsample2x")
    return out


def repeat_rows(x, r):
    """[rows, C] (row stride may exceed C) -> [r * rows, C]: r copies stacked (the batch axis of a channels-last activation)."""
    rows, C = x.shape
    out = torch.empty((r * rows, C), dtype=x.dtype, device=x.device)
    assert x.dtype == _f16
    for i in range(r):
        copy2d(x, out[i * rows:], rows, C, x.stride(0), C)
    return out


def concat_channels(a, b):
    """[rows, Ca] ++ [rows, Cb] -> [rows, Ca+Cb] (torch.cat(dim=1) of the reference's NCHW tensors)."""
    rows, ca = a.shape
    cb = b.shape[1]
    out = torch.empty((rows, ca + cb), dtype=_f16, device=a.device)
    copy2d(a, out, rows, ca, a.stride(0), ca + cb)
    copy2d(b, out[:, ca:], rows, cb, b.stride(0), ca + cb)
    return out


def add_nchw_(h, feat):
    """h [n, H, W, C] fp16 channels-last += feat [n, C, H, W] (any float dtype): adapter features (openaimodel3d.py:582-585)."""
    n, H, W, C = h.shape
    feat = feat.float().contiguous()
    if tuple(feat.shape) != (n, C, H, W):
        raise VcxError(f"adapter feature {tuple(feat.shape)} does not match the activation [{n}, {C}, {H}, {W}]")
    _dev16(h)
    _dev32(feat)
    check(lib().vcx_add_nchw_f32_to_nhwc_f16(feat.data_ptr(), h.data_ptr(), n, C, H * W, _stream()), "add_nchw")
    return h


def ncthw_to_nthwc(src, dst, c_off=0, scale=1.0):
    """src fp32 [B, C, T, H, W] -> dst fp16 [B, T, H, W, ldc][..., c_off:c_off+C]."""
    B, C, T, H, W = src.shape
    src = src.contiguous()
    check(lib().vcx_ncthw_f32_to_nthwc_f16(src.data_ptr(), dst.data_ptr(), B, C, T, H * W, dst.shape[-1], c_off, scale,
                                           _stream()), "ncthw_to_nthwc")
    return dst


def nthwc_to_ncthw(src, C=None):
    """src [B, T, H, W, ldc] (fp16 or fp32) -> fp32 [B, C, T, H, W]."""
    B, T, H, W, ldc = src.shape
    C = ldc if C is None else C
    out = torch.empty((B, C, T, H, W), dtype=_f32, device=src.device)
    check(lib().vcx_nthwc_to_ncthw_f32(src.data_ptr(), out.data_ptr(), B, C, T, H * W, ldc,
                                       1 if src.dtype == _f32 else 0, _stream()), "nthwc_to_ncthw")
    return out


def ddim_step(x, v_cond, v_uncond, noise, coef, ws=None, v_img=None, cfg_img=0.0):
    """One DDIM update on fp32 [B, ...] tensors; coef = 8 host floats (see include/vcx.h); v_img/cfg_img select the
    multi-condition guidance of vcx_ddim_step3_f32."""
    B = x.shape[0]
    n = x.numel() // B
    x_prev = torch.empty_like(x)
    pred_x0 = torch.empty_like(x)
    if ws is None:
        ws = torch.empty((lib().vcx_ddim_ws_bytes(B, n) // 8,), dtype=torch.float64, device=x.device)
    c = (ctypes.c_float * 9)(*([float(v) for v in coef[:8]] + [float(cfg_img)]))
    check(lib().vcx_ddim_step3_f32(x.data_ptr(), v_cond.data_ptr(), _ptr(v_uncond), _ptr(v_img), _ptr(noise),
                                   x_prev.data_ptr(), pred_x0.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), B, n, c,
                                   _stream()), "ddim_step")
    return x_prev, pred_x0


def dpmpp2m_step(x, v_cond, v_uncond, d_last, coef, inv_s, c_h, ws=None, v_img=None, cfg_img=0.0, d_out=None):
    """One DPM-Solver++(2M) update on fp32 [B, ...] tensors (include/vcx.h vcx_dpmpp2m_step_f32): coef = the 8 host floats of ddim_step
    with coef[3] (sigma_t) = 0, inv_s = 1 / s of this step, c_h = the second-order coefficient (0: a first-order step, d_last may be None).
    Returns (x_prev, pred_x0, d) - d = x0 / s is the history the next step passes as d_last; d_out: a buffer to write it into."""
    _dev32(x, v_cond, v_uncond, v_img, d_last, d_out)
    B = x.shape[0]
    n = x.numel() // B
    for t in (v_cond, v_uncond, v_img, d_last, d_out):
        if t is not None and (t.numel() != x.numel() or not t.is_contiguous()):
            raise VcxError(f"dpmpp2m_step: every tensor must be contiguous with x's {x.numel()} elements, got {tuple(t.shape)}")
    x_prev = torch.empty_like(x)
    pred_x0 = torch.empty_like(x)
    if d_out is None:
        d_out = torch.empty_like(x)
    if ws is None:
        ws = torch.empty((lib().vcx_ddim_ws_bytes(B, n) // 8,), dtype=torch.float64, device=x.device)
    c = (ctypes.c_float * 11)(*([float(v) for v in coef[:8]] + [float(cfg_img), float(inv_s), float(c_h)]))
    check(lib().vcx_dpmpp2m_step_f32(x.data_ptr(), v_cond.data_ptr(), _ptr(v_uncond), _ptr(v_img), _ptr(d_last), x_prev.data_ptr(),
                                     pred_x0.data_ptr(), d_out.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), B, n, c,
                                     _stream()), "dpmpp2m_step")
    return x_prev, pred_x0, d_out


# ------------------------------------------------------------------------------------------
# experiment knobs (include/vcx.h VCX_TUNE_*): A/B tooling only, the defaults are the product
# ------------------------------------------------------------------------------------------
def tune_set(name, value):
    """Set knob `name` (a key of _lib.TUNE), return its previous value."""
    return lib().vcx_tune_set(TUNE[name][0], int(value))


def tune_get(name):
    return lib().vcx_tune_get(TUNE[name][0])


def tune_report():
    """Knobs that are NOT at their default (bench.py prints this next to its numbers): {} in production."""
    return {k: tune_get(k) for k, (_, d) in TUNE.items() if tune_get(k) != d}


# ------------------------------------------------------------------------------------------
# profiling
# ------------------------------------------------------------------------------------------
def profile_begin(max_records=1 << 16):
    check(lib().vcx_profile_begin(max_records), "profile_begin")


def profile_end():
    buf = (ctypes.c_double * (4 * len(PROF_FAMILIES)))()
    check(lib().vcx_profile_end(buf), "profile_end")
    out = {}
    for i, name in enumerate(PROF_FAMILIES):
        out[name] = dict(launches=int(buf[4 * i]), ms=buf[4 * i + 1], flops=buf[4 * i + 2], bytes=buf[4 * i + 3])
    return out
