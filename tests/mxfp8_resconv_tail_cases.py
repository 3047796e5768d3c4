"""Operands for tests/test_mxfp8_resconv_tail_gpu.py, and the calls it runs under a forced tile configuration: VCX_GEMM_MX_CFG (include/vcx.h
vcx_gemm_mxfp8_cfg) is read once per process, so the test starts `python -m tests.mxfp8_resconv_tail_cases OUT.pt` once per knob value and
compares the tensors the two processes leave behind.  Every input is built on the CPU from fixed seeds: two processes see identical operands."""
import sys

import torch

from tests import cpu_kernels_mx_tail as CT
from tests import mx_emulation as MX

DEV = "cuda"
GUARD = 777.0
# (n, H, W, Cin, Ct, N) of the forced-configuration calls: 128 rows (two whole moment strips); 320 = two wide tiles or two and a half square
# ones, 200 = ragged in both, 64 = one partial tile in both
CFG_CASES = [(2, 8, 8, 160, 96, 320), (2, 8, 8, 160, 96, 200), (2, 8, 8, 32, 160, 64)]


def exact_problem(n, H, W, cin, ct, N, seed=0):
    """Integer-grid operands (tests/mx_emulation.exact_operand) of a tailed convolution: scale bytes per (row, block), the tail source's one
    binade above and the tail weight's one below the main operands' (126 .. 128 | 127 .. 129 | 125 .. 127: products on the same 2^-2 grid, a
    scale byte fetched from the wrong part an exact mismatch), tail rows distinct per row; `seed` moves the two sources, not the weights.  -> a, t, w9, wt as (q, s, fp64 values), w as the
    kernel's joined pair, bias."""
    M = n * H * W
    a = MX.exact_operand(M, cin, 1000 + M + cin + seed)
    t = MX.exact_operand(M, ct, 1500 + M + ct + seed, e_offset=1)
    w9 = MX.exact_operand(9 * N, cin, 2000 + N + cin)
    wt = MX.exact_operand(N, ct, 2500 + N + ct, e_offset=-1)
    bias = torch.randint(-256, 257, (N,), generator=torch.Generator().manual_seed(3000 + N)).float() * MX.GRID
    assert torch.unique(t[2], dim=0).shape[0] == M, "the tail rows differ from each other: a row read from a neighbour is an exact mismatch"
    assert (9 * cin + ct) * MX.PRODUCT_MAX + 64 < (1 << 24) * MX.GRID, "every partial sum is exact in fp32"
    w = CT.join_weight(CT.slab_major(w9[0], w9[1], N), (wt[0], wt[1]))
    return a, t, (w9[0], w9[1], w9[2].view(N, 9, cin)), wt, w, bias


def rand_mx(rows, K, seed, spread=3):
    """(element bytes, scale bytes) of N(0, 1) values whose 32-blocks are 2^-spread .. 2^spread loud: the scale bytes differ per (row, block)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, K), generator=g) * torch.exp2(torch.randint(-spread, spread + 1, (rows, K // 32), generator=g).float()).repeat_interleave(32, 1)
    return MX.quant((x * K ** -0.25).half())


def random_problem(n, H, W, cin, ct, N, seed, spread=3):
    """Random MXFP8 operands of a tailed convolution (outputs of a few tens at most) -> a, t, w (joined pair), bias"""
    M = n * H * W
    a, t = rand_mx(M, cin, seed + 1, spread), rand_mx(M, ct, seed + 2, spread)
    w9, wt = rand_mx(9 * N, cin, seed + 3, spread), rand_mx(N, ct, seed + 4, spread)
    g = torch.Generator().manual_seed(seed + 5)
    w = CT.join_weight(CT.slab_major(w9[0], w9[1], N), wt)
    return a, t, w, torch.randn((N,), generator=g)


def pair(p):
    return p[0].to(DEV), p[1].to(DEV)


def run_cfg_cases():
    from viewcrafter_amd import ops
    out = {}
    for n, H, W, cin, ct, N in CFG_CASES:
        M = n * H * W
        a, t, w, bias = random_problem(n, H, W, cin, ct, N, 100 + N)
        key = f"tail {n}x{H}x{W} {cin}+{ct} N{N}"
        buf = torch.full((M + 2, N + 24), GUARD, dtype=torch.float16, device=DEV)
        cs = torch.full((M // 64, N + 64, 2), 5.0, device=DEV)
        out[key + " cfg"] = torch.tensor([ops.gemm_mxfp8_cfg(N, gather_mode=2)])
        ops.conv3x3_tail_mxfp8(pair(a), pair(t), pair(w), bias.to(DEV), n=n, H=H, W=W, cin=cin, ct=ct, out=buf[1:M + 1], ldc=N + 24, colstats=cs, colstats_ld=N + 64,
                               colstats_col=32)
        plain = ops.conv3x3_tail_mxfp8(pair(a), pair(t), pair(w), bias.to(DEV), n=n, H=H, W=W, cin=cin, ct=ct)
        torch.cuda.synchronize()
        out[key], out[key + " moments"], out[key + " plain"] = buf.cpu(), cs.cpu(), plain.view(M, N).cpu()
    n, H, W, cin, ct, N = 2, 9, 16, 160, 96, 320
    a, t, w9, wt, w, bias = exact_problem(n, H, W, cin, ct, N)
    y = ops.conv3x3_tail_mxfp8(pair(a), pair(t), pair(w), bias.to(DEV), n=n, H=H, W=W, cin=cin, ct=ct)
    torch.cuda.synchronize()
    out["exact"] = y.view(n * H * W, N).cpu()
    return out


if __name__ == "__main__":
    torch.save(run_cfg_cases(), sys.argv[1])
