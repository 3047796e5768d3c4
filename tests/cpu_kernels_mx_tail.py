"""TEST INFRASTRUCTURE ONLY - CPU stand-ins (fp64 arithmetic on the dequantised operands, tests/mx_emulation.py) for the launchers of the
MXFP8 skip-convolution tail: ops.group_norm_mxfp8_raw and ops.conv3x3_tail_mxfp8 (include/vcx.h vcx_groupnorm_apply(2)_mxfp8_raw_f16,
vcx_conv3x3_tail_mxfp8).  The emulation the GPU tests compare the kernels with; tests/cpu_kernels.py is left as it is."""
import torch

from tests import mx_emulation as MX


def shift2(a, ky, kx):
    """a [n, H, W, C] -> the pixels (y + ky - 1, x + kx - 1) of the same frame, zeros where they do not exist"""
    n, H, W, _ = a.shape
    out = torch.zeros_like(a)
    dy, dx = ky - 1, kx - 1
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[:, yd, xd] = a[:, ys, xs]
    return out


def conv_tail_ref(a, w9, t, wt, bias, n, H, W):
    """fp64: a [n H W, Cin], w9 [N, 9, Cin], t [n H W, Ct], wt [N, Ct] -> bias + the nine taps' sums + t wt^T (the tail reads row m itself)"""
    cin, M = a.shape[1], n * H * W
    a4 = a.view(n, H, W, cin)
    ref = bias.double().unsqueeze(0).expand(M, -1).clone()
    for tap in range(9):
        ref += shift2(a4, tap // 3, tap % 3).reshape(M, cin) @ w9[:, tap].t()
    return ref + t @ wt.t()


def slab_major(q, s, N):
    """[N * 9, Kp] / [N * 9, Kp / 32] (one row per (n, tap)) -> the kernel's [N, Kp / 128, 9, 128] / [N, Kp / 128, 9, 4]"""
    slabs = q.shape[1] // 128
    return (q.view(N, 9, slabs, 128).permute(0, 2, 1, 3).reshape(N, -1).contiguous(), s.view(N, 9, slabs, 4).permute(0, 2, 1, 3).reshape(N, -1).contiguous())


def join_weight(main, tail):
    """(main pair [N, 9 Kp], tail pair [N, Kpt]) -> the pair of vcx_conv3x3_tail_mxfp8's weight rows"""
    return torch.cat([main[0], tail[0]], dim=1).contiguous(), torch.cat([main[1], tail[1]], dim=1).contiguous()


def split_weight(w, cin, ct):
    """the packed pair of vcx_conv3x3_tail_mxfp8 -> fp64 (w9 [N, 9, cin], wt [N, ct])"""
    N, kp, kpt = w[0].shape[0], MX.kp_of(cin), MX.kp_of(ct)
    assert w[0].shape == (N, 9 * kp + kpt) and w[1].shape == (N, (9 * kp + kpt) // 32)
    slabs = kp // 128
    q = w[0][:, :9 * kp].cpu().view(N, slabs, 9, 128).permute(0, 2, 1, 3).reshape(N * 9, kp).contiguous()
    s = w[1][:, :9 * kp // 32].cpu().view(N, slabs, 9, 4).permute(0, 2, 1, 3).reshape(N * 9, kp // 32).contiguous()
    return MX.dequant(q, s, cin).view(N, 9, cin), MX.dequant(w[0][:, 9 * kp:].contiguous(), w[1][:, 9 * kp // 32:].contiguous(), ct)


def conv3x3_tail_mxfp8(a, tail, w, bias, *, n, H, W, cin, ct, out=None, ldc=None, colstats=None, colstats_ld=None, colstats_col=0):
    """ops.conv3x3_tail_mxfp8 on the CPU: fp64 of the dequantised operands, rounded to fp16 once; moments (mean, M2) per 64-row strip of
    the fp16 output."""
    M = n * H * W
    w9, wt = split_weight(w, cin, ct)
    N = w9.shape[0]
    y = conv_tail_ref(MX.dequant(a[0], a[1], cin), w9, MX.dequant(tail[0], tail[1], ct), wt, bias.cpu(), n, H, W).half()
    if colstats is not None:
        ld = N if colstats_ld is None else colstats_ld
        yd = y.double().view(M // 64, 64, N)
        mean = yd.mean(1)
        colstats.view(M // 64, ld, 2)[:, colstats_col:colstats_col + N] = torch.stack([mean, ((yd - mean.unsqueeze(1)) ** 2).sum(1)], dim=-1).float()
    if out is None:
        return y.view(n, H, W, N)
    ldc = out.stride(0) if ldc is None else ldc
    torch.as_strided(out, (M, N), (ldc, 1), out.storage_offset())[:] = y
    return torch.as_strided(out, (n, H, W, ldc), (H * W * ldc, W * ldc, ldc, 1), out.storage_offset())


def group_norm_mxfp8_raw(x, gamma, beta, eps, silu, groups=32, stats=None, x2=None):
    """ops.group_norm_mxfp8_raw on the CPU: (quant(fp16(group_norm([x | x2]))), quant([x | x2])) - the normalisation in fp32 as
    tests/cpu_kernels.group_norm restates it."""
    from tests import cpu_kernels as CK
    xc = x if x2 is None else torch.cat([x, x2], dim=2).contiguous()
    n_outer, pixels, C = xc.shape
    y = CK.group_norm(xc, gamma, beta, eps, silu, groups=groups, stats=stats)
    return MX.quant(y.reshape(n_outer * pixels, C).half().contiguous()), MX.quant(xc.reshape(n_outer * pixels, C).contiguous())
