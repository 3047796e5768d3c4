/*
 * vcx_pool.h — an additive extension of the C ABI of libvcx.so (include/vcx.h, whose conventions hold here): LayerNorm and a 2x2 pool of
 * the token grid in one pass, the pooled key / value operand of the opt-in spatial self-attention over 2x2-pooled tokens.
 *
 * These entry points are exported by the same library and change no signature, descriptor or number of vcx.h: VCX_ABI_VERSION stays 18
 * and vcx.h's own list of entry points is unchanged.  A binding that wants them includes this header (ctypes: viewcrafter_amd/_lib.py
 * EXT_SYMBOLS) and finds them by name; a library built before them does not export the names.
 */
#ifndef VCX_POOL_H
#define VCX_POOL_H

#include "vcx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x fp16 [n H W][C]: dense token rows, row-major over (frame, y, x); y fp16 [n (H/2) (W/2)][C].  A byte identity, the fp16 normalised
 * image is never written:
 *   VCX_POOL_MEAN     y == vcx_avgpool2x2_f16(vcx_layernorm_f16(x) viewed [n][H][W][C]): every normalised value rounded to fp16 exactly as
 *                     vcx_layernorm_f16 stores it (its statistics, in its summation order), the four values of a window then summed in
 *                     fp32 in vcx_avgpool2x2_f16's order - (2y, 2x), (2y, 2x+1), (2y+1, 2x), (2y+1, 2x+1) - times 0.25, rounded once.
 *   VCX_POOL_NEAREST  y holds the rows (2y, 2x) of vcx_layernorm_f16(x); the other three rows of a window are never read.
 * VCX_EINVAL, nothing written: H or W odd, C % 8 != 0 or C > 8192, a pointer not 16-byte aligned, n H W >= 2^31, another mode.
 * vcx_layernorm_pool2x2_ok: 1 where the geometry and mode are taken, else 0 with the reason in vcx_last_error(); no device needed. */
#define VCX_POOL_MEAN 0
#define VCX_POOL_NEAREST 1
int vcx_layernorm_pool2x2_f16(const void* x, void* y, const float* gamma, const float* beta, int n, int H, int W, int C, float eps, int mode,
                              void* stream);
int vcx_layernorm_pool2x2_ok(int n, int H, int W, int C, int mode);

#ifdef __cplusplus
}
#endif

#endif /* VCX_POOL_H */
