// Operand and scale map of v_mfma_scale_f32_16x16x128_f8f6f4 with fp8 (e4m3) operands, measured: one-hot operands and coded scales, one
// wave per block, block = one register position p = (lane l, byte j) of the one-hot operand.  Prints what differs from the map that
// csrc/gemm_mx.hip relies on:
//   lane l = (row / column l & 15, group g = l >> 4), byte j of its 32 holds K-element k = 64 (j / 16) + 16 g + j % 16;
//   A position p meets B position p (both operands use the same map);
//   the scale byte of lane (row, group b) applies to the elements k in [32 b, 32 b + 32) of that row - held by OTHER lanes' registers;
//   op_sel picks the byte of the scale register (0 = low byte).
// MI355X: 0 differences in every line.      hipcc --offload-arch=gfx950 -O2 -o ubench_mfma_scale_map tools/ubench_mfma_scale_map.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
typedef int i8v __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
#define ONE 0x38u
__device__ unsigned char code8(int v) {  // e4m3 byte of integer v in 1..16
    const unsigned char t[17] = {0, 0x38, 0x40, 0x44, 0x48, 0x4A, 0x4C, 0x4E, 0x50, 0x51, 0x52, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58};
    return t[v];
}
// exp 0: A one-hot(p) = 1, B all ones, scales 127            -> which D row the A position feeds
// exp 1: A one-hot(p), B[pos q] = 1 + (q & 15)                -> low 4 bits of the B position paired with p   (q = (l>>4)*32 + j)
// exp 2: A one-hot(p), B[pos q] = 1 + (q >> 4)                -> high 3 bits
// exp 3: A one-hot(p), B ones, scale_a(lane l) = 127 + (l>>4) -> which lane group's scale applies to p
// exp 4: A one-hot(p), B ones, scale_a(lane l) = 127 + (l&15) -> which lane row's scale applies
// exp 5: A one-hot(p), B ones, scale_a reg bytes {127,128,129,130} in every lane, opsel 0 -> which byte
// exp 6..8: as 0, 3, 4 with the roles of A and B swapped (B one-hot, scale_b coded)
// exp 9: as 5 with opsel 2
__global__ void probe(float* out) {
    const int p = blockIdx.x, pl = p >> 5, pj = p & 31;
    const int l = threadIdx.x;
    for (int e = 0; e < 10; ++e) {
        unsigned char a[32], b[32];
        const bool swap = e >= 6 && e <= 8;
        for (int j = 0; j < 32; ++j) {
            const int q = (l >> 4) * 32 + j;
            unsigned char hot = (l == pl && j == pj) ? ONE : 0;
            unsigned char oth = ONE;
            if (e == 1) oth = code8(1 + (q & 15));
            if (e == 2) oth = code8(1 + (q >> 4));
            a[j] = swap ? oth : hot;
            b[j] = swap ? hot : oth;
        }
        i8v av, bv;
        for (int r = 0; r < 8; ++r) {
            av[r] = a[4 * r] | (a[4 * r + 1] << 8) | (a[4 * r + 2] << 16) | (a[4 * r + 3] << 24);
            bv[r] = b[4 * r] | (b[4 * r + 1] << 8) | (b[4 * r + 2] << 16) | (b[4 * r + 3] << 24);
        }
        int sa = 127, sb = 127;
        int sc = 127;
        if (e == 3 || e == 7) sc = 127 + (l >> 4);
        if (e == 4 || e == 8) sc = 127 + (l & 15);
        if (e == 5 || e == 9) sc = 127 | (128 << 8) | (129 << 16) | (130 << 24);
        if (swap) sb = sc; else sa = sc;
        f4 c = {0.f, 0.f, 0.f, 0.f};
        f4 d;
        if (e == 9) d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 0, 0, 2, sa, 0, sb);
        else d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 0, 0, 0, sa, 0, sb);
        // D: row = 4 (l >> 4) + r, col = l & 15
        for (int r = 0; r < 4; ++r) out[((size_t)(p * 10 + e) * 16 + 4 * (l >> 4) + r) * 16 + (l & 15)] = d[r];
    }
}
int main() {
    const int P = 2048;
    const size_t n = (size_t)P * 10 * 256;
    float* d;
    if (hipMalloc(&d, n * 4) != hipSuccess) { printf("malloc failed\n"); return 1; }
    hipMemset(d, 0, n * 4);
    hipLaunchKernelGGL(probe, dim3(P), dim3(64), 0, 0, d);
    if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 1; }
    std::vector<float> h(n);
    hipMemcpy(h.data(), d, n * 4, hipMemcpyDeviceToHost);
    auto D = [&](int p, int e, int i, int c) { return h[((size_t)(p * 10 + e) * 16 + i) * 16 + c]; };
    // exp 0 / 6: which row (A) / column (B) is fed
    for (int e : {0, 6}) {
        int bad = 0;
        for (int p = 0; p < P; ++p) {
            int l = p >> 5, hits = 0, where = -1; bool uniform = true;
            for (int i = 0; i < 16; ++i) for (int c = 0; c < 16; ++c) {
                float v = D(p, e, i, c);
                if (v != 0.f) { ++hits; where = e == 0 ? i : c; if (v != 1.f) uniform = false; }
            }
            if (hits != 16 || where != (l & 15) || !uniform) { if (bad++ < 6) printf("exp%d p=(%d,%d): hits %d where %d uniform %d\n", e, l, p & 31, hits, where, (int)uniform); }
        }
        printf("exp%d (%s one-hot feeds %s l&15 with value 1): %d of %d positions differ\n", e, e ? "B" : "A", e ? "column" : "row", bad, P);
    }
    // exp 1, 2: pairing of positions
    {
        int bad = 0;
        for (int p = 0; p < P; ++p) {
            int l = p >> 5, j = p & 31, row = l & 15;
            float lo = D(p, 1, row, 0), hi = D(p, 2, row, 0);
            int q = ((int)hi - 1) * 16 + ((int)lo - 1), want = (l >> 4) * 32 + j;
            if (q != want) { if (bad++ < 40) printf("pair: A pos (lane grp %d, byte %d) = %d pairs with B pos %d (lo %g hi %g)\n", l >> 4, j, want, q, lo, hi); }
        }
        printf("pairing (A position p meets B position p): %d of %d differ\n", bad, P);
    }
    for (int e : {3, 4, 7, 8}) {
        int bad = 0;
        for (int p = 0; p < P; ++p) {
            int l = p >> 5, j = p & 31;
            float v = (e < 6) ? D(p, e, l & 15, 0) : D(p, e, 0, l & 15);
            const int k = 64 * (j / 16) + 16 * (l >> 4) + j % 16;      // the K-element this register byte holds
            int want = (e == 3 || e == 7) ? (k >> 5) : (l & 15);
            float wantv = (float)(1 << want);
            if (v != wantv) { if (bad++ < 24) printf("exp%d p=(lane %d = row %d grp %d, byte %d): scale factor %g, expected %g\n", e, l, l & 15, l >> 4, j, v, wantv); }
        }
        printf("exp%d (the scale applied is the one of lane %s): %d of %d differ\n", e, (e == 3 || e == 7) ? "group k / 32" : "row l & 15", bad, P);
    }
    printf("exp5 opsel 0 factor at p=0: %g ; p=(lane 17, byte 3): %g ; exp9 opsel 2: %g %g\n", D(0, 5, 0, 0), D(17 * 32 + 3, 5, 1, 0), D(0, 9, 0, 0), D(17 * 32 + 3, 9, 1, 0));
    return 0;
}
