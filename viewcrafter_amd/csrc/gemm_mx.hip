// vcx_gemm_mxfp8: out[m, n] = sum_k A[m, k] W[n, k] with both operands in MXFP8 (include/vcx.h "MXFP8 operands": e4m3fn element bytes,
// one e8m0 scale byte per 32 K-elements) on the block-scaled matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulation.
//
// The structure is gemm_dma.hip's: operand tiles go HBM -> LDS with `buffer_load_dwordx4 ... lds` through descriptors whose range check
// zero-fills rows beyond M / N, the 128-byte LDS row (there 64 fp16, here one 128-element K-step) carries the same XOR swizzle, the walk
// over tiles is persistent and XCD-aware (tile_coords), loads run one K-step ahead in a second LDS buffer.  The scale bytes of a K-step
// - one dword per tile row - come through LDS by the same DMA (`buffer_load_dword ... lds`), never by a VGPR load inside the K loop.
//
// Operand roles as in the fp16 engine: weight = A operand of the instruction, activation = B operand, so a lane's four accumulator
// registers are four consecutive output columns of one row (gemm_epilogue.h).
//
// Operand map of the instruction with fp8 operands, measured with one-hot operands and coded scales (tools/ubench_mfma_scale_map.hip) - NOT
// 32 consecutive K-elements per lane: lane l = (row l & 15, group g = l >> 4) supplies K-elements 16 g .. 16 g + 15 in its registers 0-3
// and 64 + 16 g .. 64 + 16 g + 15 in its registers 4-7 - the 16-byte chunks g and 4 + g of the 128-byte row, the same two chunks the fp16
// engine's lane reads - while its scale byte is the one of K-block g (elements 32 g .. 32 g + 31) of its row: a lane's scale applies to
// elements held by its neighbours (groups 2 (g >> 1) and 2 (g >> 1) + 1 hold block g's elements).  tests/test_mxfp8_gpu.py checks the
// whole path with exact data and per-(row, block) scales: a lane that fed 32 consecutive elements was an exact mismatch.
//
// TWO tile shapes - 128 x 128 (Cfg128: 2 x 2 waves, 64 x 64 per wave) and 128 x 160 (Cfg160: 64 x 80 per wave, for N = 160 j: 320 columns
// are two whole tiles of 160, not two and a half of 128) - and ONE K order: the tile shape does not enter a row's arithmetic (same K-steps,
// same instruction, same epilogue statements), so a row's result does not depend on M, on the tile it falls into, on the configuration or
// on the grid, and both configurations give the same bytes.  vcx_gemm_mxfp8_cfg (below) chooses from N alone.  A wave's 64 packed GEGLU
// columns are 32 output columns - one MX block of the next layer's K axis - so the quantising epilogue takes a block's maximum inside the
// wave, across the four lane groups, with two lane swaps: the GEGLU epilogues exist on Cfg128 only.  No atomics.
//
// vcx_conv_t3_mxfp8 (T3 = true): the (3,1,1) temporal convolution as a GATHERED mode of the same kernel.  K is three taps of Kp(Cin) each
// (weights [N][3][Kp], tap-major, every tap padded on its own: no MX block and no K-step straddles two taps); K-step kt belongs to tap
// kt / (Kp / 128), and the activation DMA and the scale-dword DMA of that step read row m + (tap - 1) P of the activation [B T P][Kp].
// Whether that row exists is decided per row from t = (m / P) % T when a tile's offsets are set up (three bits per row in one register;
// the offsets of a tap are one add and one select per DMA instruction, recomputed at issue: no second and third set of row offsets): where
// frame t + tap - 1 of the row's OWN video does not exist the offset is forced out of range, the descriptor zero-fills element and scale
// bytes and the products are 0 - a row at t = 0 of video b > 0 never reads video b - 1, and m - P < 0 never wraps.  The weight side stays
// linear in K.
//
// vcx_conv3x3_mxfp8 (GM = 2): the 3x3 / padding-1 convolution of a ResBlock, the second gathered mode.  The activation is [n][H][W][Kp], row
// m = (f H + y) W + x; K is SLAB-major, for the reason packing.conv_slab_major gives for the fp16 engine: K-step kt belongs to the
// 128-channel slab kt / 9 and to tap kt % 9 = 3 ky + kx (weights [N][Kp / 128][9][128], every tap quantised and padded on its own), so the
// nine re-reads of a tile's input rows are consecutive K-steps.  Tap (ky, kx) reads row m + (ky - 1) W + (kx - 1), which exists iff
// 0 <= y + ky - 1 < H and 0 <= x + kx - 1 < W inside the row's OWN frame: six bits per DMA row (three for ky, three for kx, from
// (m / W) % H and m % W when a tile's offsets are set up; 5 rows x 6 bits in the register T3 uses 15 bits of), a tap is valid iff both of
// its bits are set, and its offset is one add and one select at issue.  A missing source row gets an out-of-range offset: no read of the
// neighbouring frame, no wrap to the previous image row at x = 0 or the next one at x = W - 1, no negative offset at m < W + 1.
//
// vcx_conv3x3_tail_mxfp8 (GM = 2, TAIL): the second convolution of a ResBlock with its 1x1 skip convolution as a LINEAR K TAIL.  After the
// 9 Kp(Cin) / 128 gathered K-steps of a tile, Kp(Ct) / 128 further K-steps read row m ITSELF of a second MXFP8 source t [M][Kp(Ct)] (the
// quantised block input, written by the raw quantising GroupNorm apply) through descriptors of its own: no tap, no validity bits beyond
// m < M (a tail row exists for every row, wherever it sits in its frame), rows beyond M out of range.  The weight rows are
// [9 Kp(Cin) main | Kp(Ct) tail] (packing.pack_conv3x3_tail_mxfp8), linear in K like every weight side: main and tail are quantised and
// padded on their own, no MX block and no K-step straddles them.  One K order - main steps, then tail steps ascending - in both tile shapes.
#include "gemm_epilogue.h"
#include "mx_format.h"

using namespace vcxgemm;
using namespace vcxmx;

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef int i8v __attribute__((ext_vector_type(8)));
typedef int i4v __attribute__((ext_vector_type(4)));
constexpr unsigned OOB = 0xFFFFFFFFu;
constexpr int KSTEP = 128;            // K-elements (= bytes) per LDS row and per matrix instruction

struct MxArgs {
    const unsigned char* A;           // [M][kp] element bytes
    const unsigned char* As;          // [M][kp / 32] scale bytes
    const unsigned char* W;           // [N][kp]
    const unsigned char* Ws;          // [N][kp / 32]
    void* C;                          // fp16 [M][ldc], or element bytes [M][kpo] (VCX_GEMM_MXFP8_OUT)
    unsigned char* Cs;                // scale bytes [M][kpo / 32] (VCX_GEMM_MXFP8_OUT)
    const float* bias;
    const half_t* R;
    int M, N, kp, kpo;
    int ldc, ldr, flags;
    int tiles_m, tiles_n;
    unsigned a_bytes, as_bytes, w_bytes, ws_bytes, c_bytes, cs_bytes, r_bytes;
    // vcx_conv_t3_mxfp8: frames per video, pixels per frame (kp = one tap's K extent, the activation's row pitch; the weight's is 3 kp)
    int T, P;
    // vcx_conv3x3_mxfp8: the frame's grid (the weight's row pitch is 9 kp) and the row-indexed addend of VCX_GEMM_ROWADD (gemm_epilogue.h)
    int GH, GW;
    const float* rowadd;
    int rowadd_ld, rowadd_div;
    // vcx_conv3x3_tail_mxfp8: the linear tail source [M][kpt] / [M][kpt / 32] (the weight's row pitch is 9 kp + kpt)
    const unsigned char* Tl;
    const unsigned char* Tls;
    int kpt;
    unsigned t_bytes, ts_bytes;
    float* colstats;                  // VCX_GEMM_COLSTATS: (mean, M2) per 64-row strip and output column (gemm_epilogue.h, LNF = 3)
    int64_t ldcs;
};

template <int TBM_, int TBN_, int NWM_, int NWN_>
struct MxCfg {
    static constexpr int TBM = TBM_, TBN = TBN_, NWM = NWM_, NWN = NWN_;
    static constexpr int THREADS = 64 * NWM * NWN;
    static constexpr int MF = TBM / NWM / 16, NF = TBN / NWN / 16;
    static constexpr int XROWS = TBM * 8 / THREADS, WROWS = TBN * 8 / THREADS, RSTEP = THREADS / 8;
    static constexpr size_t TILE = (size_t)(TBM + TBN) * KSTEP;             // element bytes of one stage
    // scale dwords of one stage: [TBM] activation rows, then the weight rows rounded up to whole waves - every scale DMA instruction is
    // issued by all 64 lanes of a wave (a lane beyond TBN weight rows has an out-of-range offset and writes a zero into the padding)
    static constexpr int SROWS = TBM + (TBN + 63) / 64 * 64;
    static constexpr int SPASS = (SROWS + THREADS - 1) / THREADS;           // scale-DMA passes: one dword per thread and pass
    static constexpr size_t SCALES = (size_t)SROWS * 4;
    static constexpr size_t STAGES = 2 * (TILE + SCALES);
    static constexpr size_t STRIP = (size_t)TBN * NWM * sizeof(float);      // gemm_epilogue's strip of column addends per wave
    static constexpr size_t SMEM = STAGES + STRIP;
    // pass 0 covers the activation rows and the first THREADS - TBM weight rows, a second pass (Cfg160: wave 0, weight rows 128 .. 159) the rest
    static_assert(TBM % 64 == 0 && TBM < THREADS && SPASS <= 2, "scale DMA: one dword per thread and pass, a wave's 64 rows on one operand");
    static_assert(XROWS * THREADS == TBM * 8 && WROWS * THREADS == TBN * 8, "tile DMA: whole rows of 8 threads");
};

__device__ __forceinline__ int mx_lds_off(int row, int chunk) {      // byte offset of a 16-byte chunk of a [rows][128] byte tile (lds_off's swizzle)
    return row * KSTEP + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// GEGLU epilogue (bias + x * gelu_erf(gate)), fp16 or MXFP8 output from the SAME statements: the gated value is rounded to fp16 exactly once,
// QOUT then quantises the 32-column blocks of those fp16 values - quant(the fp16-out result) bit for bit.
// Packed weight columns come in 64-column blocks [32 value | 32 gate] (packing.pack_geglu); a wave owns one block: fragments 0, 1 are
// values, 2, 3 their gates, output column = block * 32 + a * 16 + lg * 4 + r.
template <class Cfg, bool QOUT>
__device__ __forceinline__ void mx_geglu_epilogue(const MxArgs& p, f4 (&acc)[Cfg::NF][Cfg::MF], int tile_m, int tile_n, int wm, int wn, int lane) {
    static_assert(Cfg::NF == 4, "one 64-column packed block per wave");
    constexpr int WM = Cfg::TBM / Cfg::NWM, WN = Cfg::TBN / Cfg::NWN;
    typedef unsigned u2v __attribute__((ext_vector_type(2)));
    const int lr = lane & 15, lg = lane >> 4;
    const int nb = tile_n * Cfg::TBN + wn * WN;          // first packed column of the wave's block
    const bool col_ok = nb + 64 <= p.N;                  // (QOUT: blocks beyond N are the output's K padding)
    const int jout = nb >> 1;
    f4 bx[2], bg[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const bool hb = col_ok && (p.flags & VCX_GEMM_BIAS_N);
        bx[a] = hb ? *reinterpret_cast<const f4*>(p.bias + nb + a * 16 + lg * 4) : f4{0.f, 0.f, 0.f, 0.f};
        bg[a] = hb ? *reinterpret_cast<const f4*>(p.bias + nb + 32 + a * 16 + lg * 4) : f4{0.f, 0.f, 0.f, 0.f};
    }
    const __amdgpu_buffer_rsrc_t srd_c = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, (int)p.c_bytes, 0x00020000);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t srd_s = __builtin_amdgcn_make_buffer_rsrc(QOUT ? (void*)p.Cs : p.C, 0, QOUT ? (int)p.cs_bytes : 0, 0x00020000);
#pragma unroll
    for (int b = 0; b < Cfg::MF; ++b) {
        const int m = tile_m * Cfg::TBM + wm * WM + b * 16 + lr;
        h4 o[2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float xv = acc[a][b][r] + bx[a][r];
                const float gv = acc[a + 2][b][r] + bg[a][r];
                o[a][r] = (half_t)(xv * gelu_erf(gv));
            }
        if constexpr (!QOUT) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const unsigned voff = (col_ok && m < p.M) ? ((unsigned)m * (unsigned)p.ldc + (unsigned)(jout + a * 16 + lg * 4)) * 2u : OOB;
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, o[a]), srd_c, voff, 0, 0);
            }
        } else {
            // the block's maximum: 8 values in the lane, then across the four lane groups that share the row (lanes lr + 16 lg)
            const h8 o8 = {o[0][0], o[0][1], o[0][2], o[0][3], o[1][0], o[1][1], o[1][2], o[1][3]};
            unsigned hmax = mx_absmax_bits(o8);
            const auto s16 = __builtin_amdgcn_permlane16_swap(hmax, hmax, false, false);
            hmax = max(s16[0], s16[1]);
            const auto s32 = __builtin_amdgcn_permlane32_swap(hmax, hmax, false, false);
            hmax = max(s32[0], s32[1]);
            float mul;
            unsigned sb = mx_scale_byte(hmax, mul);
            uint2 qb = mx_quant8(o8, sb, mul);
            if (!col_ok) {
                sb = MX_SCALE_ONE;
                qb = make_uint2(0u, 0u);
            }
            const unsigned ok = m < p.M;
            const unsigned qoff = (unsigned)m * (unsigned)p.kpo + (unsigned)(jout + lg * 4);
            __builtin_amdgcn_raw_buffer_store_b32(qb.x, srd_c, ok ? qoff : OOB, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(qb.y, srd_c, ok ? qoff + 16u : OOB, 0, 0);
            const unsigned soff = (unsigned)m * (unsigned)(p.kpo >> 5) + (unsigned)(jout >> 5);
            __builtin_amdgcn_raw_buffer_store_b8((unsigned char)sb, srd_s, (ok && lg == 0) ? soff : OOB, 0, 0);
        }
    }
}

// EPI: 0 = bias / residual, fp16 out (gemm_epilogue.h, the fp16 engine's epilogue); 1 = GEGLU, fp16 out; 2 = GEGLU, MXFP8 out;
// 3 = EPI 0 + column moments of the output (VCX_GEMM_COLSTATS).  GM, the gather mode of the activation operand: 0 = linear, 1 = the temporal
// 3-tap convolution, 2 = the spatial 3x3 convolution (file header).  TAIL (GM = 2 only): linear K-steps of a second source behind the gathered ones.
template <class Cfg, int EPI, int GM = 0, bool TAIL = false>
__global__ void __launch_bounds__(Cfg::THREADS, 2) gemm_mx_kernel(MxArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr bool T3 = GM == 1, C9 = GM == 2, GATHER = GM != 0;
    static_assert(!TAIL || (C9 && (EPI == 0 || EPI == 3)), "the K tail belongs to the 3x3 gather, plain and column-moment epilogues");
    constexpr int VB = C9 ? 6 : 3;      // validity bits per DMA row
    constexpr int TBM = Cfg::TBM, TBN = Cfg::TBN, NFRAG = Cfg::NF, MFRAG = Cfg::MF;
    constexpr int XROWS = Cfg::XROWS, WROWS = Cfg::WROWS, RSTEP = Cfg::RSTEP;
    constexpr int WM = TBM / Cfg::NWM, WN = TBN / Cfg::NWN;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];      // ALL of the kernel's LDS: [2] tiles, [2] scale dwords, strips
    unsigned char* sT = smem_raw;                                     // stage b: X tile [TBM][128], then W tile [TBN][128]
    unsigned* sS = reinterpret_cast<unsigned*>(smem_raw + 2 * Cfg::TILE);      // stage b: [TBM] activation-row dwords, then the weight-row dwords (Cfg::SROWS in all)
    constexpr int SROWS = Cfg::SROWS;

    const __amdgpu_buffer_rsrc_t srd_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.A), 0, (int)p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t srd_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.W), 0, (int)p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t srd_as = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.As), 0, (int)p.as_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t srd_ws = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.Ws), 0, (int)p.ws_bytes, 0x00020000);

    [[maybe_unused]] const __amdgpu_buffer_rsrc_t srd_t =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(TAIL ? p.Tl : p.A), 0, TAIL ? (int)p.t_bytes : 0, 0x00020000);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t srd_ts =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(TAIL ? p.Tls : p.As), 0, TAIL ? (int)p.ts_bytes : 0, 0x00020000);

    const int ntiles = p.tiles_m * p.tiles_n;
    const int G = gridDim.x;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int chunk = tid & 7;   // LDS chunk position inside the 128-byte row
    const int r0 = tid >> 3;     // tile row of this thread's first DMA instruction
    const bool scale_is_a = wave < TBM / 64;      // wave-uniform: this wave's scale dwords belong to activation rows
    // wave-uniform: this wave also issues a second scale pass, for the weight rows THREADS - TBM + 64 wave ... that pass 0 does not reach
    [[maybe_unused]] const bool scale2 = Cfg::SPASS > 1 && Cfg::THREADS + wave * 64 < SROWS;
    [[maybe_unused]] unsigned soff_w2 = OOB;

    unsigned xoff[XROWS], woff[WROWS], soff_v;
    // T3: bit 3 i + tap = the source row of tap `tap` exists for this thread's DMA row i (i = XROWS: its scale row); xoff / soff_v then hold
    // the offsets of the centre tap whether or not the row is below M.  C9: bits 6 i + ky and 6 i + 3 + kx, tap (ky, kx) exists iff both are set
    [[maybe_unused]] unsigned vbits = 0;
    [[maybe_unused]] const unsigned tap_step = T3 ? (unsigned)p.P * (unsigned)p.kp : 0u;      // bytes between a row and the same pixel one frame on
    [[maybe_unused]] const int nk_tap = p.kp / KSTEP;      // K-steps of a tap (T3) = channel slabs (C9)
    [[maybe_unused]] auto tap_bits = [&](int m) -> unsigned {
        if (m >= p.M) return 0u;
        if constexpr (C9) {
            const unsigned q = (unsigned)m / (unsigned)p.GW;
            const unsigned x = (unsigned)m - q * (unsigned)p.GW, y = q % (unsigned)p.GH;
            return 2u | (y > 0u ? 1u : 0u) | (y + 1u < (unsigned)p.GH ? 4u : 0u) | 16u | (x > 0u ? 8u : 0u) | (x + 1u < (unsigned)p.GW ? 32u : 0u);
        } else {
            const unsigned t = ((unsigned)m / (unsigned)p.P) % (unsigned)p.T;
            return 2u | (t > 0u ? 1u : 0u) | (t + 1u < (unsigned)p.T ? 4u : 0u);
        }
    };
    const unsigned wpitch = (unsigned)(C9 ? 9 * p.kp + (TAIL ? p.kpt : 0) : T3 ? 3 * p.kp : p.kp);      // bytes of a weight row
    // TAIL: first row of the load tile.  The tail offsets of a DMA row are recomputed from it at issue (one multiply per row and tail step,
    // no second set of row offsets); whether the row is below M is the centre bit of its tap bits.
    [[maybe_unused]] int lrow0 = 0;
    auto init_load = [&](int t) {
        int tile_m, tile_n;
        tile_coords(t, ntiles, p.tiles_n, tile_m, tile_n);
        if constexpr (TAIL) lrow0 = tile_m * TBM;
#pragma unroll
        for (int i = 0; i < XROWS; ++i) {
            const int r = r0 + RSTEP * i;
            const int m = tile_m * TBM + r;
            const unsigned csrc = (unsigned)(chunk ^ ((r >> 1) & 7)) * 16u;   // source chunk that lands at position `chunk`
            if constexpr (GATHER) {
                xoff[i] = (unsigned)m * (unsigned)p.kp + csrc;
                vbits = i == 0 ? tap_bits(m) : vbits | (tap_bits(m) << (VB * i));
            } else {
                xoff[i] = m < p.M ? (unsigned)m * (unsigned)p.kp + csrc : OOB;
            }
        }
#pragma unroll
        for (int i = 0; i < WROWS; ++i) {
            const int r = r0 + RSTEP * i;
            const int n = tile_n * TBN + r;
            const unsigned csrc = (unsigned)(chunk ^ ((r >> 1) & 7)) * 16u;
            woff[i] = n < p.N ? (unsigned)n * wpitch + csrc : OOB;
        }
        const unsigned spitch = (unsigned)(p.kp >> 5);
        if (scale_is_a) {
            const int m = tile_m * TBM + tid;
            if constexpr (GATHER) {
                soff_v = (unsigned)m * spitch;
                vbits |= tap_bits(m) << (VB * XROWS);
            } else {
                soff_v = m < p.M ? (unsigned)m * spitch : OOB;
            }
        } else {
            const int n = tile_n * TBN + (tid - TBM);
            soff_v = n < p.N ? (unsigned)n * (wpitch >> 5) : OOB;
        }
        if constexpr (Cfg::SPASS > 1) {
            const int r = Cfg::THREADS - TBM + tid;      // weight row of the second pass
            const int n = tile_n * TBN + r;
            soff_w2 = (r < TBN && n < p.N) ? (unsigned)n * (wpitch >> 5) : OOB;
        }
    };
    // issue the DMA of K-step kt of the load tile into LDS stage `buf` (T3: kt is K-step kk of tap `tap`, kt = tap nk_tap + kk; C9: kt is
    // tap `tap` of slab kk, kt = 9 kk + tap)
    auto load_tile = [&](int kt, int buf, [[maybe_unused]] int tap = 0, [[maybe_unused]] int kk = 0) {
        unsigned char* dx = sT + buf * Cfg::TILE + wave * 8 * KSTEP;
        unsigned char* dw = sT + buf * Cfg::TILE + TBM * KSTEP + wave * 8 * KSTEP;
        const unsigned soff = (unsigned)kt * KSTEP;
        const unsigned soff_x = GATHER ? (unsigned)kk * KSTEP : soff;
        // the tap's distance in rows, times kp bytes (kp / 32 scale bytes), modulo 2^32: exact for every row that exists
        [[maybe_unused]] const int ky = C9 ? tap / 3 : 0, kx = C9 ? tap - 3 * ky : 0;
        [[maybe_unused]] const unsigned drow = C9 ? (unsigned)((ky - 1) * p.GW + (kx - 1)) : 0u;
        [[maybe_unused]] const unsigned shift = C9 ? drow * (unsigned)p.kp : (unsigned)(tap - 1) * tap_step;
        [[maybe_unused]] const unsigned sshift = C9 ? drow * (unsigned)(p.kp >> 5) : (unsigned)(tap - 1) * (tap_step >> 5);
        [[maybe_unused]] auto valid = [&](int i) -> bool {      // the source row of this tap exists for DMA row i
            if constexpr (C9) return ((vbits >> (VB * i + ky)) & (vbits >> (VB * i + 3 + kx)) & 1u) != 0u;
            else return ((vbits >> (VB * i + tap)) & 1u) != 0u;
        };
        [[maybe_unused]] const int jt = kt - 9 * nk_tap;      // TAIL: K-step of the tail once the nine taps of every slab are through (uniform)
        if (TAIL && jt >= 0) {
#pragma unroll
            for (int i = 0; i < XROWS; ++i) {
                const int r = r0 + RSTEP * i;
                const unsigned csrc = (unsigned)(chunk ^ ((r >> 1) & 7)) * 16u;
                const unsigned vo = ((vbits >> (VB * i + 1)) & 1u) ? (unsigned)(lrow0 + r) * (unsigned)p.kpt + csrc : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_t, (lds_ptr_t)(dx + RSTEP * i * KSTEP), 16, vo, (unsigned)jt * KSTEP, 0, 0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < XROWS; ++i) {
                unsigned vo = xoff[i];
                if constexpr (GATHER) vo = valid(i) ? vo + shift : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_a, (lds_ptr_t)(dx + RSTEP * i * KSTEP), 16, vo, soff_x, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < WROWS; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_w, (lds_ptr_t)(dw + RSTEP * i * KSTEP), 16, woff[i], soff, 0, 0);
        // the K-step's four scale bytes of every tile row: one dword per thread, lane-linear behind the wave's base
        unsigned* ds = sS + buf * SROWS + wave * 64;
        if constexpr (GATHER) {
            if (scale_is_a && TAIL && jt >= 0) {
                const unsigned vo = ((vbits >> (VB * XROWS + 1)) & 1u) ? (unsigned)(lrow0 + tid) * (unsigned)(p.kpt >> 5) : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_ts, (lds_ptr_t)ds, 4, vo, (unsigned)jt * 4u, 0, 0);
            } else if (scale_is_a) {
                const unsigned vo = valid(XROWS) ? soff_v + sshift : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_as, (lds_ptr_t)ds, 4, vo, (unsigned)kk * 4u, 0, 0);
            } else {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_ws, (lds_ptr_t)ds, 4, soff_v, (unsigned)kt * 4u, 0, 0);
            }
        } else {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(scale_is_a ? srd_as : srd_ws, (lds_ptr_t)ds, 4, soff_v, (unsigned)kt * 4u, 0, 0);
        }
        if constexpr (Cfg::SPASS > 1) {      // the weight side is linear in K in every gather mode
            if (scale2) __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_ws, (lds_ptr_t)(ds + Cfg::THREADS), 4, soff_w2, (unsigned)kt * 4u, 0, 0);
        }
    };

    const int wm = wave % Cfg::NWM, wn = wave / Cfg::NWM;
    const int lr = lane & 15, lg = lane >> 4;

    f4 acc[NFRAG][MFRAG];
#pragma unroll
    for (int a = 0; a < NFRAG; ++a)
#pragma unroll
        for (int b = 0; b < MFRAG; ++b) acc[a][b] = f4{0.f, 0.f, 0.f, 0.f};

    const int nk = C9 ? 9 * nk_tap + (TAIL ? p.kpt / KSTEP : 0) : T3 ? 3 * nk_tap : p.kp / KSTEP;
    [[maybe_unused]] int ltap = 0, lkk = 0;      // T3: tap and K-step inside the tap of the load side's lkt; C9: tap and slab
    int ltile = blockIdx.x, lkt = 0;
    int ctile = blockIdx.x, ckt = 0;
    int tile_m, tile_n;
    tile_coords(ctile, ntiles, p.tiles_n, tile_m, tile_n);
    init_load(ltile);
    load_tile(0, 0, 0, 0);
    __builtin_amdgcn_s_waitcnt(0x0f70 | 0);   // vmcnt(0): first K-step landed in LDS
    __syncthreads();
    int cur = 0;
    for (;;) {
        if (++lkt == nk) {
            lkt = 0;
            ltile += G;
            if (ltile < ntiles) init_load(ltile);
            if constexpr (GATHER) ltap = lkk = 0;
        } else if constexpr (T3) {
            if (++lkk == nk_tap) {
                lkk = 0;
                ++ltap;
            }
        } else if constexpr (C9) {      // (TAIL: past the slabs tap and slab go on counting unused - a tail step is lkt - 9 nk_tap)
            if (++ltap == 9) {
                ltap = 0;
                ++lkk;
            }
        }
        const bool more = ltile < ntiles;
        if (more) load_tile(lkt, cur ^ 1, ltap, lkk);        // async: lands in the other stage while this one is consumed
        const unsigned char* cx = sT + cur * Cfg::TILE;
        const unsigned char* cw = cx + TBM * KSTEP;
        const unsigned* csx = sS + cur * SROWS;
        const unsigned* csw = csx + TBM;
        auto frag = [&](const unsigned char* base, int row) {      // the lane's 32 K-elements of `row`: 16-byte chunks lg and 4 + lg (see the file header)
            const i4v lo = *reinterpret_cast<const i4v*>(base + mx_lds_off(row, lg));
            const i4v hi = *reinterpret_cast<const i4v*>(base + mx_lds_off(row, 4 + lg));
            return i8v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        };
        {
            i8v xf[MFRAG];
            int xs[MFRAG];
#pragma unroll
            for (int b = 0; b < MFRAG; ++b) {
                xf[b] = frag(cx, wm * WM + b * 16 + lr);
                xs[b] = (int)(csx[wm * WM + b * 16 + lr] >> (8 * lg));      // byte 0 = the scale of the lane's own block
            }
            i8v wcur = frag(cw, wn * WN + lr);
            int wscur = (int)(csw[wn * WN + lr] >> (8 * lg));
#pragma unroll
            for (int a = 0; a < NFRAG; ++a) {
                i8v wnext = wcur;
                int wsnext = wscur;
                if (a + 1 < NFRAG) {      // the next weight fragment is requested ahead of the MFMAs that use the current one
                    wnext = frag(cw, wn * WN + (a + 1) * 16 + lr);
                    wsnext = (int)(csw[wn * WN + (a + 1) * 16 + lr] >> (8 * lg));
                }
#pragma unroll
                for (int b = 0; b < MFRAG; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wcur, xf[b], acc[a][b], 0, 0, 0, wscur, 0, xs[b]);
                wcur = wnext;
                wscur = wsnext;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (ckt == nk - 1) {
            if constexpr (EPI == 0 || EPI == 3) {
                GemmArgs q{};
                q.C = p.C;
                q.bias = p.bias;
                q.R = p.R;
                q.M = p.M;
                q.N = p.N;
                q.ldc = p.ldc;
                q.ldr = p.ldr;
                q.flags = p.flags;
                q.alpha = 1.0f;
                q.rowadd_div = 1;
                if constexpr (C9) {
                    q.rowadd = p.rowadd;
                    q.rowadd_ld = p.rowadd_ld;
                    q.rowadd_div = p.rowadd_div;
                }
                q.c_bytes = p.c_bytes;
                q.r_bytes = p.r_bytes;
                q.colstats = p.colstats;
                q.ldcs = p.ldcs;
                float* sB = reinterpret_cast<float*>(smem_raw + Cfg::STAGES) + wave * WN;   // the wave's private strip of column addends
                gemm_epilogue<Cfg, false, false, EPI == 3 ? 3 : 0>(q, acc, tile_m, tile_n, wm, wn, lane, sB);
            } else {
                mx_geglu_epilogue<Cfg, EPI == 2>(p, acc, tile_m, tile_n, wm, wn, lane);
            }
#pragma unroll
            for (int a = 0; a < NFRAG; ++a)
#pragma unroll
                for (int b = 0; b < MFRAG; ++b) acc[a][b] = f4{0.f, 0.f, 0.f, 0.f};
        }
        // the DMA of the next K-step must have landed, and every wave must be done reading `cur`, before the roles swap
        __builtin_amdgcn_s_waitcnt(0x0f70 | 0);
        __syncthreads();
        cur ^= 1;
        if (++ckt == nk) {
            ckt = 0;
            ctile += G;
            if (ctile >= ntiles) break;
            tile_coords(ctile, ntiles, p.tiles_n, tile_m, tile_n);
        }
    }
#endif
}

template <class Cfg, int EPI, int GM = 0, bool TAIL = false>
int launch_mx(const MxArgs& a, hipStream_t s) {
    static VcxLdsAttr lds;
    auto kern = gemm_mx_kernel<Cfg, EPI, GM, TAIL>;
    const char* name = TAIL ? "vcx_conv3x3_tail_mxfp8" : GM == 2 ? "vcx_conv3x3_mxfp8" : GM == 1 ? "vcx_conv_t3_mxfp8" : "vcx_gemm_mxfp8";
    if (!lds.ensure(reinterpret_cast<const void*>(kern), (int)Cfg::SMEM, name)) return VCX_ELAUNCH;
    const int nb = persistent_grid(a.tiles_m * a.tiles_n, 2);
    hipLaunchKernelGGL(kern, dim3(nb), dim3(Cfg::THREADS), Cfg::SMEM, s, a);
    return vcx_check_launch(name);
}

using Cfg128 = MxCfg<128, 128, 2, 2>;
using Cfg160 = MxCfg<128, 160, 2, 2>;      // 64 x 80 per wave (MF 4, NF 5); plain and column-moment epilogues, every gather mode
static_assert(Cfg160::TBM == Cfg128::TBM, "the shape predicates' row reach (127 rows past M) holds for both configurations");
constexpr unsigned long long LIM = 0xFFFF0000ull;      // 32-bit buffer offsets, as in the fp16 DMA engine

// the epilogue a flag word selects: 0 / 1 / 2 as gemm_mx_kernel's EPI, -1 = a combination this entry point does not have
int epi_of(int flags) {
    if (flags == VCX_GEMM_BIAS_N || flags == (VCX_GEMM_BIAS_N | VCX_GEMM_RESIDUAL)) return 0;
    if (flags == (VCX_GEMM_BIAS_N | VCX_GEMM_GEGLU)) return 1;
    if (flags == (VCX_GEMM_BIAS_N | VCX_GEMM_GEGLU | VCX_GEMM_MXFP8_OUT)) return 2;
    return -1;
}

// What the four entry points differ in, host side only: one value per call, read by the shape predicate and by the launcher.
struct MxCall {
    int gm;                            // gather mode (gemm_mx_kernel's GM)
    bool tail;                         // the linear K tail behind the gathered K-steps (GM = 2)
    int taps;                          // 1, 3 or 9: a weight row is taps x Kp(Cin) (+ Kp(Ct)) bytes
    int may;                           // flags a gathered form permits beside BIAS_N
    const char *dims, *rows;           // the factors of M as the messages name them ("B, T, P" / "B T P")
    const char* reach_name;            // ... and the reach ("P", "W + 1")
    const char* flag_rule;             // the reason of a refused flag word
    int64_t outer, in1, in2;           // M = outer x in1 x in2: (B, T, P), (n, H, W) or (M, 1, 1)
    unsigned long long reach;          // rows the farthest tap reads past a row: 0, P or W + 1
    int64_t Cin, Ct, N;
    int flags;
    int64_t ldc, ldr, ldcs, cs_col;    // cs_col: first column of the moments inside their [strips][ldcs] buffer (a launcher's pointer already
                                       // points there and shows its parity in its alignment: the launchers pass 0)
    int64_t rowadd_ld, rowadd_div;
    int64_t M() const { return outer * in1 * in2; }      // (after the predicate's 2^31 product checks)
    int epi() const { return gm == 0 ? epi_of(flags) : (flags & VCX_GEMM_COLSTATS) ? 3 : 0; }
};

MxCall mx_linear(int64_t M, int64_t N, int64_t K, int64_t ldc, int64_t ldr, int flags) {
    return {0, false, 1, 0, "M", "M", "", "", M, 1, 1, 0, K, 0, N, flags, ldc, ldr, 0, 0, 0, 0};
}

MxCall mx_t3(int64_t B, int64_t T, int64_t P, int64_t Cin, int64_t N, int64_t ldc, int64_t ldr, int64_t ldcs, int64_t cs_col, int flags) {
    return {1, false, 3, VCX_GEMM_RESIDUAL | VCX_GEMM_COLSTATS, "B, T, P", "B T P", "P", "flags: BIAS_N, optionally with RESIDUAL and / or COLSTATS",
            B, T, P, (unsigned long long)P, Cin, 0, N, flags, ldc, ldr, ldcs, cs_col, 0, 0};
}

// the 3x3 form, and with `tail` its K-tailed form: bias required, COLSTATS optional; a residual or a row addend is refused there (the second
// convolution of a skip-convolution block has neither)
MxCall mx_c9(int64_t n, int64_t H, int64_t W, int64_t Cin, bool tail, int64_t Ct, int64_t N, int64_t ldc, int64_t ldr, int64_t ldcs, int64_t cs_col,
             int64_t rowadd_ld, int64_t rowadd_div, int flags) {
    return {2, tail, 9, tail ? VCX_GEMM_COLSTATS : VCX_GEMM_ROWADD | VCX_GEMM_RESIDUAL | VCX_GEMM_COLSTATS, "n, H, W", "n H W", "W + 1",
            tail ? "flags: BIAS_N, optionally with COLSTATS (no RESIDUAL, no ROWADD on the tailed form)"
                 : "flags: BIAS_N, optionally with ROWADD, RESIDUAL and / or COLSTATS",
            n, H, W, (unsigned long long)W + 1, Cin, Ct, N, flags, ldc, ldr, ldcs, cs_col, rowadd_ld, rowadd_div};
}

typedef char MxWhy[256];      // the reason of a refusal
#define MX_NEED(cond, ...)                             \
    do {                                               \
        if (!(cond)) {                                 \
            snprintf(why, sizeof(MxWhy), __VA_ARGS__); \
            return false;                              \
        }                                              \
    } while (0)

// 32-bit buffer offsets of fp16 rows of pitch ld (output, residual): the tile grid reaches up to 127 rows past M, and those rows' offsets must
// not wrap back into the buffer
unsigned long long mx_mt(unsigned long long M) { return (M + 127) / 128 * 128; }
bool mx_f16_fits(unsigned long long M, int64_t ld) { return mx_mt(M) * (unsigned long long)ld * 2 < LIM; }

// vcx_gemm_mxfp8: shape rules and extents of a call with the given row pitches (elements of the output / residual; their alignment is the
// entry point's business); `why` gets the reason of a refusal
bool mx_takes(const MxCall& c, MxWhy& why) {
    const int64_t M = c.outer, N = c.N, K = c.Cin;
    const int epi = c.epi();
    MX_NEED(epi >= 0, "flags: BIAS_N, BIAS_N | RESIDUAL, BIAS_N | GEGLU or BIAS_N | GEGLU | MXFP8_OUT");
    MX_NEED(M > 0 && N > 0 && K > 0 && K % MX_BLOCK == 0 && N % 8 == 0 && !(epi && N % 64 != 0) && M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31),
            "need M, N, K > 0, K %% 32 == 0, N %% 8 == 0 (GEGLU: N %% 64 == 0, whole packed blocks; MXFP8 out: N / 2 %% 32 == 0)");
    const int64_t nout = epi ? N / 2 : N;
    const unsigned long long kp = (unsigned long long)mx_kp(K), kpo = (unsigned long long)mx_kp(nout);
    bool fits = (unsigned long long)M * kp < LIM && (unsigned long long)N * kp < LIM && mx_mt(M) * kp < (1ull << 32);
    if (epi == 2) fits = fits && mx_mt(M) * kpo < LIM;
    else fits = fits && c.ldc >= nout && mx_f16_fits(M, c.ldc) && (!(c.flags & VCX_GEMM_RESIDUAL) || (c.ldr >= nout && mx_f16_fits(M, c.ldr)));
    MX_NEED(fits, "an operand, output or residual extent of 4 GiB or more (32-bit buffer offsets)");
    return true;
}

// vcx_conv_t3_mxfp8, vcx_conv3x3_mxfp8, vcx_conv3x3_tail_mxfp8: shape, flag, pitch and extent rules; the first failing rule decides the reason
bool mx_gather_takes(const MxCall& c, MxWhy& why) {
    constexpr int64_t I31 = 1ll << 31;
    const int64_t N = c.N, Cin = c.Cin;
    const bool res = c.flags & VCX_GEMM_RESIDUAL;
    MX_NEED((c.flags & VCX_GEMM_BIAS_N) && !(c.flags & ~(VCX_GEMM_BIAS_N | c.may)), "%s", c.flag_rule);
    MX_NEED(c.outer > 0 && c.in1 > 0 && c.in2 > 0 && Cin > 0 && N > 0 && Cin % MX_BLOCK == 0 && N % 8 == 0, "need %s, Cin, N > 0, Cin %% 32 == 0, N %% 8 == 0",
            c.dims);
    MX_NEED(c.outer < I31 && c.in1 < I31 && c.in2 < I31 && Cin < I31 && N < I31 && c.ldc < I31 && c.ldr < I31 && c.ldcs < I31 && c.rowadd_div < I31
                && c.outer * c.in1 < I31 && c.outer * c.in1 * c.in2 < I31,
            "a dimension of 2^31 or more");
    const unsigned long long M = (unsigned long long)c.M(), kp = (unsigned long long)mx_kp(Cin);
    MX_NEED(c.ldc >= N && c.ldc % 8 == 0 && (!res || (c.ldr >= N && c.ldr % 8 == 0)),
            "row pitches: ldc >= N, ldc %% 8 == 0; with RESIDUAL ldr >= N, ldr %% 8 == 0");
    MX_NEED(!(c.flags & VCX_GEMM_COLSTATS) || (M % 64 == 0 && c.cs_col >= 0 && c.ldcs >= c.cs_col + N && c.ldcs % 2 == 0 && c.cs_col % 2 == 0),
            "COLSTATS: %s %% 64 == 0, ldcs >= first column + N, ldcs and the first column even (16-byte aligned moment pairs)", c.rows);
    MX_NEED(!(c.flags & VCX_GEMM_ROWADD) || c.rowadd_div > 0, "ROWADD: rowadd_div > 0 (output rows per row of the addend)");
    // 32-bit buffer offsets.  The tile grid reaches up to 127 rows past M and the farthest tap `reach` rows further: (M + 127 + reach) Kp must
    // not wrap for the activation (its scale array is 1/32 of it); the weight rows are taps x Kp long and reach 127 rows past N.
    MX_NEED((M + 127 + c.reach) * kp < LIM && ((unsigned long long)N + 127) * c.taps * kp < LIM && mx_f16_fits(M, c.ldc) && (!res || mx_f16_fits(M, c.ldr)),
            "an operand, output or residual extent of 4 GiB or more (32-bit buffer offsets; activations: (M + 127 + %s) Kp)", c.reach_name);
    if (!c.tail) return true;
    MX_NEED(c.Ct > 0 && c.Ct % MX_BLOCK == 0 && c.Ct < I31, "need Ct > 0, Ct %% 32 == 0, Ct < 2^31");
    // the tail source reaches 127 rows past M, the weight rows are taps x Kp(Cin) + Kp(Ct) long and reach 127 rows past N
    const unsigned long long kpt = (unsigned long long)mx_kp(c.Ct);
    MX_NEED((M + 127) * kpt < LIM && ((unsigned long long)N + 127) * (c.taps * kp + kpt) < LIM,
            "a tail or weight extent of 4 GiB or more (32-bit buffer offsets; tail: (M + 127) Kp(Ct), weights: (N + 127) (9 Kp(Cin) + Kp(Ct)))");
    return true;
}
#undef MX_NEED

// The tile configuration of a call: 0 = Cfg128, 1 = Cfg160 (include/vcx.h vcx_gemm_mxfp8_cfg).  A function of N, the flag word and the gather
// mode - never of M: a row's configuration cannot depend on the batch.  Cfg160 has the plain and the column-moment epilogue only.
int mx_cfg_of(int64_t N, int flags, int gm) {
    bool has;
    if (gm == 0) has = epi_of(flags) == 0;
    else {
        const int may = VCX_GEMM_BIAS_N | VCX_GEMM_RESIDUAL | VCX_GEMM_COLSTATS | (gm == 2 ? VCX_GEMM_ROWADD : 0);
        has = (flags & VCX_GEMM_BIAS_N) && !(flags & ~may);
    }
    if (!has || N <= 0 || N % 8 != 0) return 0;
    const int knob = vcx_mx_cfg_knob();
    if (knob >= 0) return knob;
    return N % Cfg160::TBN == 0 && N % Cfg128::TBN != 0;
}

// the launchers' configuration: mx_cfg_of's, unless the wide tile's reach of TBN - 1 weight rows past N leaves the 32-bit offsets (row_bytes =
// taps x Kp; the shape predicates vouch for Cfg128's reach only) - such a call keeps Cfg128, which computes the same bytes
int mx_cfg_launch(int64_t N, int flags, int gm, unsigned long long row_bytes) {
    const int cfg = mx_cfg_of(N, flags, gm);
    if (cfg == 1 && ((unsigned long long)N + Cfg160::TBN - 1) * row_bytes >= LIM) return 0;
    return cfg;
}

// every kernel there is: [GM + TAIL][EPI][configuration], null where the family has none (Cfg160: plain and column-moment epilogues only; the
// GEGLU epilogues: the linear form only; column moments: the gathered forms only)
typedef int (*MxLaunch)(const MxArgs&, hipStream_t);
constexpr MxLaunch MX_KERNELS[4][4][2] = {
    {{launch_mx<Cfg128, 0>, launch_mx<Cfg160, 0>}, {launch_mx<Cfg128, 1>, nullptr}, {launch_mx<Cfg128, 2>, nullptr}, {nullptr, nullptr}},
    {{launch_mx<Cfg128, 0, 1>, launch_mx<Cfg160, 0, 1>}, {nullptr, nullptr}, {nullptr, nullptr}, {launch_mx<Cfg128, 3, 1>, launch_mx<Cfg160, 3, 1>}},
    {{launch_mx<Cfg128, 0, 2>, launch_mx<Cfg160, 0, 2>}, {nullptr, nullptr}, {nullptr, nullptr}, {launch_mx<Cfg128, 3, 2>, launch_mx<Cfg160, 3, 2>}},
    {{launch_mx<Cfg128, 0, 2, true>, launch_mx<Cfg160, 0, 2, true>}, {nullptr, nullptr}, {nullptr, nullptr},
     {launch_mx<Cfg128, 3, 2, true>, launch_mx<Cfg160, 3, 2, true>}},
};

// a call's operands, in the order the entry points name them; null where a form has none
struct MxPtrs {
    const void *a, *a_scales, *t, *t_scales, *w, *w_scales;
    void *out, *out_scales;
    const float *bias, *rowadd;
    const void* residual;
    float* colstats;
};

// fills the kernel's arguments for a call its predicate took, and launches it
int mx_launch(const MxCall& c, const MxPtrs& o, void* stream) {
    const int64_t M = c.M(), N = c.N;
    const int epi = c.epi();
    const int64_t nout = epi == 1 || epi == 2 ? N / 2 : N;
    const bool radd = c.flags & VCX_GEMM_ROWADD;
    MxArgs p{};
    p.A = (const unsigned char*)o.a;
    p.As = (const unsigned char*)o.a_scales;
    p.Tl = (const unsigned char*)o.t;
    p.Tls = (const unsigned char*)o.t_scales;
    p.W = (const unsigned char*)o.w;
    p.Ws = (const unsigned char*)o.w_scales;
    p.C = o.out;
    p.Cs = (unsigned char*)o.out_scales;
    p.bias = o.bias;
    p.R = (const half_t*)o.residual;
    p.M = (int)M;
    p.N = (int)N;
    p.kp = (int)mx_kp(c.Cin);
    p.kpt = c.tail ? (int)mx_kp(c.Ct) : 0;
    p.kpo = (int)mx_kp(nout);
    if (c.gm == 1) {
        p.T = (int)c.in1;
        p.P = (int)c.in2;
    } else if (c.gm == 2) {
        p.GH = (int)c.in1;
        p.GW = (int)c.in2;
    }
    p.rowadd = radd ? o.rowadd : nullptr;
    p.rowadd_ld = radd ? (int)c.rowadd_ld : 0;
    p.rowadd_div = radd ? (int)c.rowadd_div : 1;      // (the 3x3 epilogue divides by it with or without the flag)
    p.ldc = (int)c.ldc;
    p.ldr = (int)c.ldr;
    p.flags = c.flags;
    p.colstats = o.colstats;
    p.ldcs = c.ldcs;
    const int64_t wrow = (int64_t)c.taps * p.kp + p.kpt;      // bytes of a weight row
    const int cfg = mx_cfg_launch(N, c.flags, c.gm, (unsigned long long)wrow);
    const int tbn = cfg ? Cfg160::TBN : Cfg128::TBN;
    p.tiles_m = (int)((M + Cfg128::TBM - 1) / Cfg128::TBM);
    p.tiles_n = epi == 2 ? 2 * p.kpo / Cfg128::TBN : (int)((N + tbn - 1) / tbn);
    p.a_bytes = (unsigned)(M * p.kp);
    p.as_bytes = (unsigned)(M * (p.kp / MX_BLOCK));
    p.t_bytes = (unsigned)(M * p.kpt);
    p.ts_bytes = (unsigned)(M * (p.kpt / MX_BLOCK));
    p.w_bytes = (unsigned)(N * wrow);
    p.ws_bytes = (unsigned)(N * (wrow / MX_BLOCK));
    p.c_bytes = epi == 2 ? (unsigned)(M * p.kpo) : (unsigned)(2 * ((M - 1) * c.ldc + nout));
    p.cs_bytes = epi == 2 ? (unsigned)(M * (p.kpo / MX_BLOCK)) : 0u;
    p.r_bytes = (c.flags & VCX_GEMM_RESIDUAL) ? (unsigned)(2 * ((M - 1) * c.ldr + nout)) : 0u;
    const MxLaunch launch = MX_KERNELS[c.gm + c.tail][epi][cfg];
    VCX_REQUIRE(launch, "gemm_mx: no kernel for gather mode %d%s, epilogue %d, configuration %d", c.gm, c.tail ? " (tailed)" : "", epi, cfg);
    hipStream_t s = (hipStream_t)stream;
    VcxProfScope prof(VCX_FAM_GEMM, s, 2.0 * M * N * ((double)c.taps * c.Cin + c.Ct), (double)M * (p.kp + p.kpt) + (double)N * wrow + 2.0 * M * nout);
    return launch(p, s);
}

}  // namespace

extern "C" int vcx_gemm_mxfp8_cfg(int64_t N, int flags, int gather_mode) {
    VCX_REQUIRE(gather_mode >= 0 && gather_mode <= 2, "vcx_gemm_mxfp8_cfg: gather mode %d (0 = vcx_gemm_mxfp8, 1 = vcx_conv_t3_mxfp8, 2 = vcx_conv3x3_mxfp8)", gather_mode);
    return mx_cfg_of(N, flags, gather_mode);
}

extern "C" int vcx_conv3x3_mxfp8_ok(int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t N, int64_t ldc, int64_t ldr, int64_t ldcs, int64_t colstats_col,
                                    int64_t rowadd_div, int flags) {
    MxWhy why;
    if (mx_gather_takes(mx_c9(n, H, W, Cin, false, 0, N, ldc, ldr, ldcs, colstats_col, 0, rowadd_div, flags), why)) return 1;
    vcx_set_error("vcx_conv3x3_mxfp8_ok(n=%lld, H=%lld, W=%lld, Cin=%lld, N=%lld, ldc=%lld, ldr=%lld, ldcs=%lld, col=%lld, rowadd_div=%lld, flags=0x%x): %s",
                  (long long)n, (long long)H, (long long)W, (long long)Cin, (long long)N, (long long)ldc, (long long)ldr, (long long)ldcs, (long long)colstats_col,
                  (long long)rowadd_div, flags, why);
    return 0;
}

extern "C" int vcx_conv3x3_mxfp8(const void* a, const void* a_scales, const void* w, const void* w_scales, void* out, const float* bias, const float* rowadd,
                                 const void* residual, float* colstats, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t N, int64_t ldc, int64_t ldr,
                                 int64_t ldcs, int64_t rowadd_ld, int64_t rowadd_div, int flags, void* stream) {
    VCX_REQUIRE(a && a_scales && w && w_scales && out && bias, "vcx_conv3x3_mxfp8: null pointer");
    VCX_REQUIRE(!(flags & VCX_GEMM_ROWADD) || rowadd, "vcx_conv3x3_mxfp8: VCX_GEMM_ROWADD needs a rowadd");
    VCX_REQUIRE(!(flags & VCX_GEMM_RESIDUAL) || residual, "vcx_conv3x3_mxfp8: VCX_GEMM_RESIDUAL needs a residual");
    VCX_REQUIRE(!(flags & VCX_GEMM_COLSTATS) || colstats, "vcx_conv3x3_mxfp8: VCX_GEMM_COLSTATS needs a colstats buffer");
    const MxCall c = mx_c9(n, H, W, Cin, false, 0, N, ldc, ldr, ldcs, 0, rowadd_ld, rowadd_div, flags);
    MxWhy why;
    VCX_REQUIRE(mx_gather_takes(c, why),
                "vcx_conv3x3_mxfp8(n=%lld, H=%lld, W=%lld, Cin=%lld, N=%lld, flags=0x%x, ldc=%lld, ldr=%lld, ldcs=%lld, rowadd_div=%lld): %s", (long long)n,
                (long long)H, (long long)W, (long long)Cin, (long long)N, flags, (long long)ldc, (long long)ldr, (long long)ldcs, (long long)rowadd_div, why);
    VCX_REQUIRE(!(flags & VCX_GEMM_ROWADD) || (rowadd_ld >= N && rowadd_ld % 4 == 0 && rowadd_ld < (1ll << 31)),
                "vcx_conv3x3_mxfp8: VCX_GEMM_ROWADD needs rowadd_ld >= N, rowadd_ld %% 4 == 0 (rowadd_ld=%lld)", (long long)rowadd_ld);
    VCX_REQUIRE((((uintptr_t)a | (uintptr_t)w | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)rowadd | (uintptr_t)residual | (uintptr_t)colstats) & 15) == 0
                    && (((uintptr_t)a_scales | (uintptr_t)w_scales) & 3) == 0,
                "vcx_conv3x3_mxfp8: operands, output, bias, rowadd, residual and colstats must be 16-byte aligned, scale arrays 4-byte aligned");
    return mx_launch(c, {a, a_scales, nullptr, nullptr, w, w_scales, out, nullptr, bias, rowadd, residual, colstats}, stream);
}

extern "C" int vcx_conv3x3_tail_mxfp8_ok(int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t Ct, int64_t N, int64_t ldc, int64_t ldcs, int64_t colstats_col,
                                         int flags) {
    MxWhy why;
    if (mx_gather_takes(mx_c9(n, H, W, Cin, true, Ct, N, ldc, 0, ldcs, colstats_col, 0, 0, flags), why)) return 1;
    vcx_set_error("vcx_conv3x3_tail_mxfp8_ok(n=%lld, H=%lld, W=%lld, Cin=%lld, Ct=%lld, N=%lld, ldc=%lld, ldcs=%lld, col=%lld, flags=0x%x): %s", (long long)n,
                  (long long)H, (long long)W, (long long)Cin, (long long)Ct, (long long)N, (long long)ldc, (long long)ldcs, (long long)colstats_col, flags, why);
    return 0;
}

extern "C" int vcx_conv3x3_tail_mxfp8(const void* a, const void* a_scales, const void* t, const void* t_scales, const void* w, const void* w_scales, void* out,
                                      const float* bias, float* colstats, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t Ct, int64_t N, int64_t ldc,
                                      int64_t ldcs, int flags, void* stream) {
    VCX_REQUIRE(a && a_scales && t && t_scales && w && w_scales && out && bias, "vcx_conv3x3_tail_mxfp8: null pointer");
    VCX_REQUIRE(!(flags & VCX_GEMM_COLSTATS) || colstats, "vcx_conv3x3_tail_mxfp8: VCX_GEMM_COLSTATS needs a colstats buffer");
    const MxCall c = mx_c9(n, H, W, Cin, true, Ct, N, ldc, 0, ldcs, 0, 0, 0, flags);
    MxWhy why;
    VCX_REQUIRE(mx_gather_takes(c, why), "vcx_conv3x3_tail_mxfp8(n=%lld, H=%lld, W=%lld, Cin=%lld, Ct=%lld, N=%lld, flags=0x%x, ldc=%lld, ldcs=%lld): %s",
                (long long)n, (long long)H, (long long)W, (long long)Cin, (long long)Ct, (long long)N, flags, (long long)ldc, (long long)ldcs, why);
    VCX_REQUIRE((((uintptr_t)a | (uintptr_t)t | (uintptr_t)w | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)colstats) & 15) == 0
                    && (((uintptr_t)a_scales | (uintptr_t)t_scales | (uintptr_t)w_scales) & 3) == 0,
                "vcx_conv3x3_tail_mxfp8: operands, output, bias and colstats must be 16-byte aligned, scale arrays 4-byte aligned");
    return mx_launch(c, {a, a_scales, t, t_scales, w, w_scales, out, nullptr, bias, nullptr, nullptr, colstats}, stream);
}

extern "C" int vcx_conv_t3_mxfp8_ok(int64_t B, int64_t T, int64_t P, int64_t Cin, int64_t N, int64_t ldc, int64_t ldr, int64_t ldcs, int64_t colstats_col,
                                    int flags) {
    MxWhy why;
    if (mx_gather_takes(mx_t3(B, T, P, Cin, N, ldc, ldr, ldcs, colstats_col, flags), why)) return 1;
    vcx_set_error("vcx_conv_t3_mxfp8_ok(B=%lld, T=%lld, P=%lld, Cin=%lld, N=%lld, ldc=%lld, ldr=%lld, ldcs=%lld, col=%lld, flags=0x%x): %s", (long long)B,
                  (long long)T, (long long)P, (long long)Cin, (long long)N, (long long)ldc, (long long)ldr, (long long)ldcs, (long long)colstats_col, flags, why);
    return 0;
}

extern "C" int vcx_conv_t3_mxfp8(const void* a, const void* a_scales, const void* w, const void* w_scales, void* out, const float* bias,
                                 const void* residual, float* colstats, int64_t B, int64_t T, int64_t P, int64_t Cin, int64_t N, int64_t ldc, int64_t ldr,
                                 int64_t ldcs, int flags, void* stream) {
    VCX_REQUIRE(a && a_scales && w && w_scales && out && bias, "vcx_conv_t3_mxfp8: null pointer");
    VCX_REQUIRE(!(flags & VCX_GEMM_RESIDUAL) || residual, "vcx_conv_t3_mxfp8: VCX_GEMM_RESIDUAL needs a residual");
    VCX_REQUIRE(!(flags & VCX_GEMM_COLSTATS) || colstats, "vcx_conv_t3_mxfp8: VCX_GEMM_COLSTATS needs a colstats buffer");
    const MxCall c = mx_t3(B, T, P, Cin, N, ldc, ldr, ldcs, 0, flags);
    MxWhy why;
    VCX_REQUIRE(mx_gather_takes(c, why), "vcx_conv_t3_mxfp8(B=%lld, T=%lld, P=%lld, Cin=%lld, N=%lld, flags=0x%x, ldc=%lld, ldr=%lld, ldcs=%lld): %s",
                (long long)B, (long long)T, (long long)P, (long long)Cin, (long long)N, flags, (long long)ldc, (long long)ldr, (long long)ldcs, why);
    VCX_REQUIRE((((uintptr_t)a | (uintptr_t)w | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)colstats) & 15) == 0
                    && (((uintptr_t)a_scales | (uintptr_t)w_scales) & 3) == 0,
                "vcx_conv_t3_mxfp8: operands, output, bias, residual and colstats must be 16-byte aligned, scale arrays 4-byte aligned");
    return mx_launch(c, {a, a_scales, nullptr, nullptr, w, w_scales, out, nullptr, bias, nullptr, residual, colstats}, stream);
}

extern "C" int vcx_gemm_mxfp8_ok(int64_t M, int64_t N, int64_t K, int flags) {
    MxWhy why;
    const int64_t nout = (flags & VCX_GEMM_GEGLU) ? N / 2 : N;
    if (mx_takes(mx_linear(M, N, K, nout, nout, flags), why)) return 1;
    vcx_set_error("vcx_gemm_mxfp8_ok(M=%lld, N=%lld, K=%lld, flags=0x%x): %s", (long long)M, (long long)N, (long long)K, flags, why);
    return 0;
}

extern "C" int vcx_gemm_mxfp8(const void* a, const void* a_scales, const void* w, const void* w_scales, void* out, void* out_scales,
                              const float* bias, const void* residual, int64_t M, int64_t N, int64_t K, int64_t ldc, int64_t ldr, int flags,
                              void* stream) {
    VCX_REQUIRE(a && a_scales && w && w_scales && out && bias, "vcx_gemm_mxfp8: null pointer");
    VCX_REQUIRE(epi_of(flags) != 2 || out_scales, "vcx_gemm_mxfp8: VCX_GEMM_MXFP8_OUT needs out_scales");
    VCX_REQUIRE(!(flags & VCX_GEMM_RESIDUAL) || residual, "vcx_gemm_mxfp8: VCX_GEMM_RESIDUAL needs a residual");
    const MxCall c = mx_linear(M, N, K, ldc, ldr, flags);
    MxWhy why;
    VCX_REQUIRE(mx_takes(c, why), "vcx_gemm_mxfp8(M=%lld, N=%lld, K=%lld, flags=0x%x, ldc=%lld, ldr=%lld): %s", (long long)M, (long long)N, (long long)K, flags,
                (long long)ldc, (long long)ldr, why);
    VCX_REQUIRE((((uintptr_t)a | (uintptr_t)w | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)residual) & 15) == 0 && ldc % 8 == 0 && ldr % 8 == 0
                    && (((uintptr_t)a_scales | (uintptr_t)w_scales | (uintptr_t)out_scales) & 3) == 0,
                "vcx_gemm_mxfp8: operands, output, bias and residual must be 16-byte aligned (ldc, ldr %% 8 == 0), scale arrays 4-byte aligned");
    return mx_launch(c, {a, a_scales, nullptr, nullptr, w, w_scales, out, out_scales, bias, nullptr, residual, nullptr}, stream);
}
