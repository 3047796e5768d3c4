// MXFP8 store tail of the temporal attention kernel (attention.hip tattn_d64_kernel<CAUSAL, false, MXQ = true>; include/vcx.h
// vcx_attn_temporal_d64_mxfp8, ABI 15): the output values, each rounded to fp16 as the fp16 kernel stores it, leave as MXFP8 element bytes
// + block scales (mx_format.h) for the to_out GEMM.  One wave holds a (pixel, head): a head's 64 columns are two MX blocks, so the wave
// quantises its own rows - half the bytes written and no quantiser pass.  quant(the fp16 kernel's o with ldo = D) byte for byte, the K
// padding of a row included.  Everything up to the packed fp16 words `pk` is the fp16 kernel's code.
#pragma once
#include "mx_format.h"

namespace vcxmx {

// element bytes [(b t p)][ldq], scale bytes [(b t p)][ldq / 32], ldq = Kp(64 heads)
struct TAttnMxOut {
    uint8_t* q;
    uint8_t* s;
    int64_t ldq;
};

// pk[4 db + gq] = the packed fp16 words of columns 8 (4 db + gq) + 4 hi .. + 3 of output row (frame) lq, lane = 32 hi + lq - what the fp16
// store tail starts from.  `row` = (b T + lq) P + pix; rvalid = lq < T (all 64 lanes take part in the exchanges, only valid rows store).
template <class U2>
__device__ __forceinline__ void tattn_mx_store(const U2 (&pk)[8], const TAttnMxOut& o, int64_t row, int h, int heads, int hi, bool rvalid) {
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    // The fp16 tail's swap: v_permlane32_swap on the words of groups k and k + 1 leaves this lane with chunk j = k / 2 = columns
    // 16 j + 8 hi .. + 7.  MX block blk = chunks 2 blk and 2 blk + 1 of both lane halves.
    h8 ch[4];
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const unsigned a0 = pk[k][0], a1 = pk[k][1], b0 = pk[k + 1][0], b1 = pk[k + 1][1];
        const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        ch[k >> 1] = __builtin_bit_cast(h8, u4v{s0[0], s1[0], s0[1], s1[1]});
    }
    uint8_t* qrow = o.q + row * o.ldq + h * 64;
    uint8_t* srow = o.s + row * (o.ldq >> 5) + h * 2;
    unsigned sb[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        unsigned m = max(mx_absmax_bits(ch[2 * blk]), mx_absmax_bits(ch[2 * blk + 1]));      // this lane's 16 values of the block,
        m = max(m, (unsigned)__shfl_xor((int)m, 32));                                          // then the other half of the row
        float mul;
        sb[blk] = mx_scale_byte(m, mul);
        const uint2 e0 = mx_quant8(ch[2 * blk], sb[blk], mul);          // columns 32 blk + 8 hi .. + 7
        const uint2 e1 = mx_quant8(ch[2 * blk + 1], sb[blk], mul);      // columns 32 blk + 16 + 8 hi .. + 7
        // a second swap, on the byte words: lanes 0-31 get columns 32 blk .. + 15, lanes 32-63 columns 32 blk + 16 .. + 31 - one 16-byte store
        const auto t0 = __builtin_amdgcn_permlane32_swap(e0.x, e1.x, false, false);
        const auto t1 = __builtin_amdgcn_permlane32_swap(e0.y, e1.y, false, false);
        if (rvalid) *reinterpret_cast<u4v*>(qrow + 32 * blk + 16 * hi) = u4v{t0[0], t1[0], t0[1], t1[1]};
    }
    if (rvalid && hi == 0) *reinterpret_cast<unsigned short*>(srow) = (unsigned short)(sb[0] | (sb[1] << 8));
    // odd head count (D % 128 == 64): the last head's wave also writes the row's K padding - 64 zero bytes under scale 1
    if ((heads & 1) && h == heads - 1 && rvalid) {
        *reinterpret_cast<u4v*>(qrow + 64 + 16 * hi) = u4v{0u, 0u, 0u, 0u};
        *reinterpret_cast<u4v*>(qrow + 96 + 16 * hi) = u4v{0u, 0u, 0u, 0u};
        if (hi == 0) *reinterpret_cast<unsigned short*>(srow + 2) = (unsigned short)(MX_SCALE_ONE | (MX_SCALE_ONE << 8));
    }
}

}  // namespace vcxmx
