// The MXFP8 format of include/vcx.h ("MXFP8 operands") as device code: ONE definition for the quantiser, the LayerNorm-quantiser and the
// quantising GEGLU epilogue (quant_mx.hip, norm.hip, gemm_mx.hip), so that all three write the same bytes for the same fp16 values.
// tests/mx_emulation.py is the same definition in torch.
#pragma once
#include "vcx_common.h"

namespace vcxmx {

constexpr int MX_BLOCK = 32;        // K-elements per scale byte
constexpr int MX_KPAD = 128;        // K extents of fp8 buffers are padded to a multiple of this (one K-step of the matrix instruction)
constexpr unsigned MX_SCALE_ONE = 127u, MX_SCALE_NAN = 255u;

__host__ __device__ inline int64_t mx_kp(int64_t K) { return (K + MX_KPAD - 1) / MX_KPAD * MX_KPAD; }

// largest |x| of 8 fp16 values as its 15 magnitude bits (an exact maximum: fp16 magnitudes order like their bit patterns; inf / NaN >= 0x7C00)
__device__ __forceinline__ unsigned mx_absmax_bits(const h8& v) {
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    const u4v w = __builtin_bit_cast(u4v, v);
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m = max(m, w[i] & 0x7FFFu);
        m = max(m, (w[i] >> 16) & 0x7FFFu);
    }
    return m;
}

// Scale byte of a block whose largest magnitude has the bits `hmax`, and the exact power of two 2^(8 - E) its elements are multiplied by.
// E = floor(log2 amax) from the exponent field (fp16 subnormals: from the leading bit of the mantissa); no logarithm, no division.
__device__ __forceinline__ unsigned mx_scale_byte(unsigned hmax, float& mul) {
    mul = 1.0f;
    if (hmax >= 0x7C00u) return MX_SCALE_NAN;      // a non-finite value in the block
    if (hmax == 0u) return 0u;
    const int e = (int)(hmax >> 10);
    const int E = e ? e - 15 : (31 - __builtin_clz(hmax)) - 24;
    mul = __builtin_bit_cast(float, (unsigned)(8 - E + 127) << 23);
    return (unsigned)(E - 8 + 127);
}

// four e4m3fn bytes (element 0 in the low byte) of clamp(v * mul, -448, 448), round-to-nearest-even
__device__ __forceinline__ unsigned mx_cvt4(float a, float b, float c, float d, float mul) {
    auto cl = [&](float x) { return __builtin_fminf(__builtin_fmaxf(x * mul, -448.0f), 448.0f); };
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(a), cl(b), w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(c), cl(d), w, true);
    return (unsigned)w;
}

// 8 fp16 values of one block -> 8 element bytes.  `sbyte` / `mul` from mx_scale_byte of the BLOCK's maximum.  A block that holds a
// non-finite value is all 0x7F (NaN) under the NaN scale.
__device__ __forceinline__ uint2 mx_quant8(const h8& v, unsigned sbyte, float mul) {
    if (sbyte == MX_SCALE_NAN) return make_uint2(0x7F7F7F7Fu, 0x7F7F7F7Fu);
    return make_uint2(mx_cvt4((float)v[0], (float)v[1], (float)v[2], (float)v[3], mul),
                      mx_cvt4((float)v[4], (float)v[5], (float)v[6], (float)v[7], mul));
}

// maximum over the four neighbouring lanes 4q .. 4q + 3 (the lanes that hold the four 8-element chunks of one block): DPP quad permutes
__device__ __forceinline__ unsigned mx_quad_max(unsigned m) {
    m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xf, 0xf, true));      // quad_perm [1,0,3,2]
    m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xf, 0xf, true));      // quad_perm [2,3,0,1]
    return m;
}

}  // namespace vcxmx
