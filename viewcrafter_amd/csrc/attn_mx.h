// MXFP8 store tail of the attention kernels whose output feeds a to_out GEMM on the block-scaled matrix pipe: tattn_d64_kernel<CAUSAL, false,
// MXQ = true> (vcx_attn_temporal_d64_mxfp8, ABI 15) and the MXQ instantiations of flash_d64_kernel, xattn_resident2_d64_kernel (attention.hip)
// and flash2_d64_kernel (attention_v2.hip) behind vcx_attn_flash_d64_mxfp8 / vcx_attn_flash_dual_d64_mxfp8 (ABI 17).  The output values, each
// rounded to fp16 as the fp16 kernel stores it, leave as MXFP8 element bytes + block scales (mx_format.h).  In all four kernels a lane pair
// (l, l ^ 32) holds the 64 columns of one (row, head) - two MX blocks - so the wave quantises its own rows: half the bytes written and no
// quantiser pass.  quant(the fp16 kernel's o with ldo = D) byte for byte, the K padding of a row included.  Everything up to the packed fp16
// words `pk` is the fp16 kernel's code.
#pragma once
#include "mx_format.h"

namespace vcxmx {

// element bytes [rows][ldq], scale bytes [rows][ldq / 32], ldq = Kp(64 heads)
struct AttnMxOut {
    uint8_t* q;
    uint8_t* s;
    int64_t ldq;
};

// pk[4 db + gq] = the packed fp16 words of columns 8 (4 db + gq) + 4 hi .. + 3 of head h of the lane's output row, lane = 32 hi + lq - what
// the fp16 store tails start from (the MFMA 32x32 accumulator layout of O^T).  `row` = the row's index in the output; rvalid = the row
// exists (all 64 lanes take part in the exchanges, only valid rows store).
template <class U2>
__device__ __forceinline__ void attn_mx_store(const U2 (&pk)[8], const AttnMxOut& o, int64_t row, int h, int heads, int hi, bool rvalid) {
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
    // odd head count (D % 128 == 64): the last head's lanes also write the row's K padding - 64 zero bytes under scale 1
    if ((heads & 1) && h == heads - 1 && rvalid) {
        *reinterpret_cast<u4v*>(qrow + 64 + 16 * hi) = u4v{0u, 0u, 0u, 0u};
        *reinterpret_cast<u4v*>(qrow + 96 + 16 * hi) = u4v{0u, 0u, 0u, 0u};
        if (hi == 0) *reinterpret_cast<unsigned short*>(srow + 2) = (unsigned short)(MX_SCALE_ONE | (MX_SCALE_ONE << 8));
    }
}

}  // namespace vcxmx
