// vcx_quant_mxfp8_f16: fp16 rows -> MXFP8 element bytes + e8m0 block scales (include/vcx.h "MXFP8 operands"; arithmetic in mx_format.h).
// One thread per 8-element chunk of the PADDED row: the four chunks of a 32-element block sit in four neighbouring lanes, the block maximum
// is a DPP quad exchange.  HBM-bound: one 16-byte read and one 8-byte write per thread, one scale byte per four threads.
// (The LayerNorm-quantiser, vcx_layernorm_mxfp8_f16, is in norm.hip beside the LayerNorm kernel whose arithmetic it repeats.)
#include "mx_format.h"

using namespace vcxmx;

namespace {

__global__ void __launch_bounds__(256) quant_mx_kernel(const half_t* __restrict__ x, int64_t ldx, unsigned char* __restrict__ q, int64_t ldq,
                                                       unsigned char* __restrict__ sc, int64_t lds, int64_t rows, int K) {
    const int cpr = (int)(ldq >> 3);                                  // chunks per padded row (a multiple of 16)
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = id / cpr;
    const int c = (int)(id - row * cpr);
    const bool valid = row < rows;
    h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool real = valid && c * 8 < K;                             // K % 32 == 0: a block is real or padding as a whole
    if (real) v = *reinterpret_cast<const h8*>(x + row * ldx + c * 8);
    const unsigned hmax = mx_quad_max(mx_absmax_bits(v));
    float mul;
    const unsigned sb = real ? mx_scale_byte(hmax, mul) : MX_SCALE_ONE;
    if (!real) mul = 1.0f;
    if (!valid) return;
    *reinterpret_cast<uint2*>(q + row * ldq + c * 8) = mx_quant8(v, sb, mul);
    if ((c & 3) == 0) sc[row * lds + (c >> 2)] = (unsigned char)sb;
}

}  // namespace

extern "C" int vcx_quant_mxfp8_f16(const void* x, int64_t ldx, void* q, void* scales, int64_t rows, int K, void* stream) {
    VCX_REQUIRE(x && q && scales, "vcx_quant_mxfp8_f16: null pointer");
    VCX_REQUIRE(rows > 0 && K > 0 && K % MX_BLOCK == 0, "vcx_quant_mxfp8_f16: need K %% 32 == 0 (K=%d)", K);
    VCX_REQUIRE(ldx >= K && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)scales & 3) == 0,
                "vcx_quant_mxfp8_f16: x and q must be 16-byte aligned (ldx %% 8 == 0), scales 4-byte aligned");
    const int64_t kp = mx_kp(K);
    VCX_REQUIRE(rows < (1ll << 31) && rows * (kp / 8) < (1ll << 39), "vcx_quant_mxfp8_f16: too many rows");
    hipStream_t s = (hipStream_t)stream;
    VcxProfScope prof(VCX_FAM_ELT, s, 0.0, (double)rows * (2.0 * K + kp + kp / 32.0));
    const int64_t threads = rows * (kp / 8);
    hipLaunchKernelGGL(quant_mx_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, (const half_t*)x, ldx, (unsigned char*)q, kp,
                       (unsigned char*)scales, kp / MX_BLOCK, rows, K);
    return vcx_check_launch("vcx_quant_mxfp8_f16");
}
