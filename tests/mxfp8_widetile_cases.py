"""The calls of tests/test_mxfp8_widetile_gpu.py, run in a process of their own: VCX_GEMM_MX_CFG (include/vcx.h vcx_gemm_mxfp8_cfg) is read
once per process, so the test starts one process per knob value - `python -m tests.mxfp8_widetile_cases OUT.pt GROUP[,GROUP...]` - and
compares the tensors they leave behind.  Every input is built on the CPU from fixed seeds: two processes see identical operands.

Groups: `bytes` (every epilogue of the three entry points on random MXFP8 operands, outputs with their guard bands), `exact` (the integer
operands of tests/mx_emulation.py, one case per gather mode at N = 320), `extent` (output offsets past 2^31), `graph` (a ResBlock with its
temporal block at width 320)."""
import sys

import torch

from tests import mx_emulation as MX

DEV = "cuda"
GUARD = 777.0
NS = (160, 320, 480, 200)          # 200: ragged - columns 160 .. 199 sit in a second wide tile whose other 120 weight rows are zero-filled
KS = (32, 64, 320, 1280)           # 32 / 64: one K-step of which three quarters / half is padding
MS = (1, 130, 256)
T3_SMALL = (2, 3, 5)               # B, T, P: 30 rows - the one row tile straddles videos and frames
T3_STATS = (1, 4, 32)              # 128 rows: two whole moment strips
C9_SMALL = (2, 3, 5)               # n, H, W: 30 rows - the tile straddles both frames, every pixel but three has a border tap
C9_STATS = (2, 8, 8)               # 128 rows
EXACT_N = 320
EXACT_LINEAR = (130, 320)          # M, K
EXACT_T3 = (2, 3, 40, 320)         # B, T, P, Cin: 240 rows, two row tiles
EXACT_C9 = (2, 5, 7, 320)          # n, H, W, Cin
EXTENT = (8192, 160, 32, 131096)   # M, N, K, ldc: the last row's byte offset is 8191 x 131096 x 2 = 2 147 614 672 > 2^31 = 2 147 483 648


def rand_mx(rows, K, seed, spread=3):
    """(element bytes, scale bytes) of N(0, 1) values whose 32-blocks are 2^-spread .. 2^spread loud: the scale bytes differ per (row, block)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, K), generator=g) * torch.exp2(torch.randint(-spread, spread + 1, (rows, K // 32), generator=g).float()).repeat_interleave(32, 1)
    return MX.quant((x * K ** -0.25).half())


def rand_f(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def slab_major(q, s, N):
    """[N * 9, Kp] / [N * 9, Kp / 32] (one row per (n, tap)) -> vcx_conv3x3_mxfp8's [N, Kp / 128, 9, 128] / [N, Kp / 128, 9, 4]"""
    slabs = q.shape[1] // 128
    return (q.view(N, 9, slabs, 128).permute(0, 2, 1, 3).reshape(N, -1).contiguous(), s.view(N, 9, slabs, 4).permute(0, 2, 1, 3).reshape(N, -1).contiguous())


W_ELEM_MAX = 3                     # exact tier: weight elements in [-3, 3], activation elements in [-7, 7]


def exact_weight(N, taps, cin, seed):
    """MX.exact_operand for N x taps weight rows with scale exponents in {-2, -1, 0} (bytes 125 .. 127) for output columns 0 .. 127 of every
    160 and in {1, 2, 3} (bytes 128 .. 130) for columns 128 .. 159 - the same draws, moved: no scale byte of a row that the second scale-DMA
    pass of the wide tile fetches occurs in a row of the first pass, so a wrong scale row is an exact mismatch in every block."""
    q, s0, v0 = MX.exact_operand(N * taps, cin, seed, elem_max=W_ELEM_MAX, e_offset=-1)
    q1, s1, v1 = MX.exact_operand(N * taps, cin, seed, elem_max=W_ELEM_MAX, e_offset=2)
    assert torch.equal(q, q1)
    hi = ((torch.arange(N) % 160) >= 128).repeat_interleave(taps)[:, None]
    return q, torch.where(hi, s1, s0), torch.where(hi, v1, v0)


def exact_problems():
    """name -> (a triple, w triple, bias, residual, rowadd): triples are (element bytes, scale bytes, fp64 values).  Activation exponents in
    {0, 1, 2}: a product is an integer of magnitude <= 21 times 2^(-2 .. 5), a multiple of 2^-2 (MX.GRID) of magnitude <= 672."""
    g = torch.Generator().manual_seed(77)
    grid = lambda *shape: torch.randint(-256, 257, shape, generator=g).float() * MX.GRID
    N = EXACT_N
    out = {}
    M, K = EXACT_LINEAR
    out["linear"] = (MX.exact_operand(M, K, 4101, e_offset=1), exact_weight(N, 1, K, 4102), grid(N), grid(M, N).half(), None)
    B, T, P, cin = EXACT_T3
    out["t3"] = (MX.exact_operand(B * T * P, cin, 4201, e_offset=1), exact_weight(N, 3, cin, 4202), grid(N), grid(B * T * P, N).half(), None)
    n, H, W, cin = EXACT_C9
    out["c9"] = (MX.exact_operand(n * H * W, cin, 4301, e_offset=1), exact_weight(N, 9, cin, 4302), grid(N), grid(n * H * W, N).half(), grid(2, N))
    return out


def _dev(pair):
    return pair[0].to(DEV), pair[1].to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _linear(a, w, bias, M, N, K, ldc, res=None, ldr=0):
    """vcx_gemm_mxfp8 into rows 1 .. M of a guarded [M + 2, ldc] buffer; the whole buffer comes back"""
    from viewcrafter_amd import _lib
    buf = torch.full((M + 2, ldc), GUARD, dtype=torch.float16, device=DEV)
    flags = _lib.GEMM_BIAS_N | (_lib.GEMM_RESIDUAL if res is not None else 0)
    _lib.check(_lib.lib().vcx_gemm_mxfp8(a[0].data_ptr(), a[1].data_ptr(), w[0].data_ptr(), w[1].data_ptr(), buf[1].data_ptr(), None, bias.data_ptr(),
                                         None if res is None else res.data_ptr(), M, N, K, ldc, ldr, flags, _stream()), "gemm_mxfp8")
    return buf


def run_bytes(out):
    from viewcrafter_amd import ops
    bias_all = rand_f((max(NS),), 11).to(DEV)
    # ---- linear
    for K in KS:
        a_all, w_all = _dev(rand_mx(max(MS), K, 100 + K)), _dev(rand_mx(max(NS), K, 200 + K))
        for N in NS:
            w, bias = (w_all[0][:N], w_all[1][:N]), bias_all[:N].contiguous()
            for M in MS:
                a = (a_all[0][:M], a_all[1][:M])
                res = rand_f((M, N + 8), 300 + M + N).half().to(DEV)
                out[f"linear N{N} K{K} M{M} bias"] = _linear(a, w, bias, M, N, K, N + 24).cpu()
                out[f"linear N{N} K{K} M{M} residual"] = _linear(a, w, bias, M, N, K, N + 24, res, N + 8).cpu()
    # ---- temporal 3-tap
    for (B, T, P), cins, stats in ((T3_SMALL, (32,), False), (T3_STATS, (64, 320), True)):
        M = B * T * P
        for cin in cins:
            a = _dev(rand_mx(M, cin, 400 + cin))
            wq, ws = rand_mx(3 * max(NS), cin, 500 + cin)
            for N in NS:
                w = (wq[:3 * N].view(N, -1).contiguous().to(DEV), ws[:3 * N].view(N, -1).contiguous().to(DEV))
                bias, ldc = bias_all[:N].contiguous(), N + 24
                for residual in (False, True):
                    res = rand_f((M, N + 8), 600 + N).half().to(DEV)[:, :N] if residual else None          # ldr = N + 8
                    buf = torch.full((M + 2, ldc), GUARD, dtype=torch.float16, device=DEV)
                    cs = torch.full((M // 64, N + 64, 2), 5.0, device=DEV) if stats else None
                    ops.temporal_conv3_mxfp8(a, w, bias, B=B, T=T, P=P, cin=cin, residual=res, out=buf[1:M + 1], ldc=ldc, colstats=cs,
                                             colstats_ld=N + 64 if stats else None, colstats_col=32 if stats else 0)
                    name = f"t3 {B}x{T}x{P} cin{cin} N{N} residual={residual}"
                    out[name] = buf.cpu()
                    if stats:
                        out[name + " moments"] = cs.cpu()
    # ---- 3x3
    cases = [(C9_SMALL, cin, dict(), False) for cin in (32, 320)]
    cases += [(C9_STATS, 64, kw, True) for kw in (dict(), dict(div=64), dict(div=48, residual=True), dict(div=64, residual=True))]
    cases += [(C9_STATS, 64, dict(div=48), False)]
    for (n, H, W), cin, kw, stats in cases:
        M = n * H * W
        a = _dev(rand_mx(M, cin, 700 + cin + M))
        wq, ws = rand_mx(9 * max(NS), cin, 800 + cin)
        for N in NS:
            w = _dev(slab_major(wq[:9 * N].contiguous(), ws[:9 * N].contiguous(), N))
            bias, ldc, div = bias_all[:N].contiguous(), N + 24, kw.get("div", 0)
            res = rand_f((M, N + 8), 900 + N).half().to(DEV)[:, :N] if kw.get("residual") else None
            rowadd = rand_f(((M + div - 1) // div, N), 950 + N).to(DEV) if div else None          # div = 48: rows 0 .. 47 | 48 .. 95 | 96 .. 127 of one tile
            buf = torch.full((M + 2, ldc), GUARD, dtype=torch.float16, device=DEV)
            cs = torch.full((M // 64, N + 64, 2), 5.0, device=DEV) if stats else None
            ops.conv3x3_mxfp8(a, w, bias, n=n, H=H, W=W, cin=cin, rowadd=rowadd, rowadd_div=div, residual=res, out=buf[1:M + 1], ldc=ldc, colstats=cs,
                              colstats_ld=N + 64 if stats else None, colstats_col=32 if stats else 0)
            name = f"c9 {n}x{H}x{W} cin{cin} N{N} rowadd_div={div} residual={res is not None}"
            out[name] = buf.cpu()
            if stats:
                out[name + " moments"] = cs.cpu()


def run_exact(out):
    from viewcrafter_amd import ops
    N = EXACT_N
    pr = exact_problems()
    a, w, bias, res, _ = pr["linear"]
    M, K = EXACT_LINEAR
    out["exact linear"] = ops.linear_mxfp8(_dev(a), _dev(w), bias.to(DEV), K=K, residual=res.to(DEV)).cpu()
    a, w, bias, res, _ = pr["t3"]
    B, T, P, cin = EXACT_T3
    out["exact t3"] = ops.temporal_conv3_mxfp8(_dev(a), (w[0].view(N, -1).contiguous().to(DEV), w[1].view(N, -1).contiguous().to(DEV)), bias.to(DEV), B=B, T=T, P=P,
                                               cin=cin, residual=res.to(DEV)).view(B * T * P, N).cpu()
    a, w, bias, res, rowadd = pr["c9"]
    n, H, W, cin = EXACT_C9
    out["exact c9"] = ops.conv3x3_mxfp8(_dev(a), _dev(slab_major(w[0], w[1], N)), bias.to(DEV), n=n, H=H, W=W, cin=cin, rowadd=rowadd.to(DEV), rowadd_div=H * W,
                                        residual=res.to(DEV)).view(n * H * W, N).cpu()


def run_extent(out):
    from viewcrafter_amd import _lib
    M, N, K, ldc = EXTENT
    a, w = _dev(rand_mx(M, K, 1201)), _dev(rand_mx(N, K, 1202))
    bias = rand_f((N,), 1203).to(DEV)
    buf = torch.full(((M - 1) * ldc + N + 8,), GUARD, dtype=torch.float16, device=DEV)
    _lib.check(_lib.lib().vcx_gemm_mxfp8(a[0].data_ptr(), a[1].data_ptr(), w[0].data_ptr(), w[1].data_ptr(), buf.data_ptr(), None, bias.data_ptr(), None,
                                         M, N, K, ldc, 0, _lib.GEMM_BIAS_N, _stream()), "gemm_mxfp8")
    rows = lambda r0, r1: torch.stack([buf[r * ldc:r * ldc + N + 8] for r in range(r0, r1)]).cpu()
    out["extent first tile"] = rows(0, 128)
    out["extent last tile"] = rows(M - 128, M)
    out["extent guard behind row 4096"] = buf[4096 * ldc + N:4097 * ldc].cpu()


def run_graph(out):
    """ResBlock 320 -> 320 with its TemporalConvBlock, two videos of four 8 x 8 frames, under the environment's MX switches"""
    from viewcrafter_amd import ops
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as U
    C, EMB, B, F, H, W = 320, 64, 2, 4, 8, 8
    assert U.RESCONV_MXFP8 and U.TCONV_MXFP8 and not U.TCONV_MXFP8_SKIP_DIMS and not U.RESCONV_MXFP8_SKIP_DIMS, "run with the MX switches on"
    torch.manual_seed(C)
    blk = U.ResBlock(C, EMB, 0.0, out_channels=C, use_temporal_conv=True).eval()
    with torch.no_grad():
        for gn in (blk.in_layers[0], blk.out_layers[0]):
            gn.weight.copy_(1.0 + 0.2 * torch.randn(gn.weight.shape))
            gn.bias.copy_(0.1 * torch.randn(gn.bias.shape))
        for conv in (blk.in_layers[2], blk.out_layers[3]):
            conv.weight.copy_(torch.randn(conv.weight.shape) * (9 * C) ** -0.5)
            conv.bias.copy_(0.1 * torch.randn(C))
        for seq in (blk.temopral_conv.conv1, blk.temopral_conv.conv2, blk.temopral_conv.conv3, blk.temopral_conv.conv4):
            seq[-1].weight.copy_(torch.randn(seq[-1].weight.shape) * (3 * C) ** -0.5)
            seq[-1].bias.copy_(0.1 * torch.randn(C))
    blk = blk.to(DEV)
    x = (rand_f((B * F, H, W, C), 1301) * 1.3).half().to(DEV)
    emb = rand_f((B, EMB), 1302).half().to(DEV)
    with torch.no_grad():
        both = blk(x, emb, batch_size=B)[0].clone()
        ones = torch.cat([blk(x[i * F:(i + 1) * F].contiguous(), emb[i:i + 1].contiguous(), batch_size=1)[0] for i in range(B)])
    out["graph B=2"] = both.cpu()
    out["graph 2 x B=1"] = ones.cpu()
    out["graph mx packs"] = torch.tensor([len(blk._mx), len(blk.temopral_conv._mx or ())])
    out["graph cfg"] = torch.tensor([ops.gemm_mxfp8_cfg(C, 1 | 4 | 0x200, 2), ops.gemm_mxfp8_cfg(C, 1 | 0x200, 1)])


def main(path, groups):
    out = {}
    for g in groups.split(","):
        {"bytes": run_bytes, "exact": run_exact, "extent": run_extent, "graph": run_graph}[g](out)
    torch.cuda.synchronize()
    torch.save(out, path)
    print(f"{len(out)} tensors -> {path}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
