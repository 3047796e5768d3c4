"""One-time repacking of reference-layout parameters into the layouts the gfx950 kernels read.

Reference layouts (binding because checkpoints are loaded with strict=True):
conv weights [Cout, Cin, kh, kw] / [Cout, Cin, 3, 1, 1] / [Cout, Cin, 1], linear [out, in].
Kernel layouts: fp16 [N_out][K] with K ordered (tap, cin); GEGLU rows interleaved in blocks of 32; MXFP8 (opt-in feed-forward, temporal
and ResBlock convolutions): element bytes [N_out][Kp] + scale bytes [N_out][Kp / 32] per tap.
"""
import torch


def conv_slab_major(cin, taps):
    """Convolutions with cin % 64 == 0 and more than one tap keep their K axis in slabs of 64 input channels with the taps
    inside (VCX_GEMM_CONV_SLABK, include/vcx.h): the 9 (or 3) tap re-reads of a tile's input are then consecutive K-steps
    and hit L2 instead of going back to the memory side.  pack_conv and ops.conv2d / temporal_conv3 share this predicate."""
    return cin % 64 == 0 and taps > 1


def pack_conv(w):
    """[Cout, Cin, *kernel] -> [Cout, taps*Cin]: K ordered (tap, c) - the im2col order of the channels-last gather in
    csrc/gemm.hip - or (c / 64, tap, c % 64) where conv_slab_major() says so."""
    cout, cin = w.shape[0], w.shape[1]
    wk = w.reshape(cout, cin, -1)            # [Cout, Cin, taps]
    taps = wk.shape[2]
    if conv_slab_major(cin, taps):
        return wk.view(cout, cin // 64, 64, taps).permute(0, 1, 3, 2).reshape(cout, -1).contiguous()
    return wk.permute(0, 2, 1).reshape(cout, -1).contiguous()


def pack_conv_ups_folded(w, dtype=torch.float16):
    """Nearest-2x followed by a 3x3 / padding-1 convolution (reference openaimodel3d.py Upsample) as four 2x2 convolutions on the SOURCE
    grid, one per parity class (a, b) of the output pixel (2i + a, 2j + b): its tap rows -1, 0, +1 read source rows (i-1, i, i) for
    a = 0 and (i, i, i+1) for a = 1, so the 2x2 kernel of class a over source rows (i - 1 + a, i + a) has row weights
    (w[0], w[1] + w[2]) or (w[0] + w[1], w[2]); columns alike with b.  The zero padding of the upsampled image is the zero padding of
    the source, so the border needs nothing.  [Cout, Cin, 3, 3] -> [4, Cout, 4*Cin], class order 2a + b, each class packed as pack_conv
    packs a 2x2 kernel (VCX ups = 2, include/vcx.h).  The sums are made in fp64 and rounded ONCE to `dtype` (None: left in fp64)."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"pack_conv_ups_folded: need a [Cout, Cin, 3, 3] weight, got {tuple(w.shape)}")
    w64 = w.detach().double()
    fold = w64.new_tensor([[[1, 0, 0], [0, 1, 1]], [[1, 1, 0], [0, 0, 1]]])      # [parity][tap of the 2x2 kernel][tap of the 3x3 kernel]
    classes = [pack_conv(torch.einsum("ky,oiyx,lx->oikl", fold[a], w64, fold[b])) for a in (0, 1) for b in (0, 1)]
    out = torch.stack(classes)
    return out if dtype is None else out.to(dtype)


def pad_cin(w, cin_to):
    """Zero-pad the input-channel dim of a conv weight (e.g. the VAE's 4-channel conv_in to 8)."""
    if w.shape[1] == cin_to:
        return w
    out = w.new_zeros((w.shape[0], cin_to) + tuple(w.shape[2:]))
    out[:, :w.shape[1]] = w
    return out


def pack_geglu(w, b):
    """GEGLU.proj (lvdm/modules/attention.py:415-422) has rows [0, D) = x and [D, 2D) = gate.  Interleave them in
    blocks of 32 so that x_j and gate_j land in the same lane of one wave's accumulators (VCX_GEMM_GEGLU)."""
    two_d = w.shape[0]
    d = two_d // 2
    assert d % 32 == 0, "GEGLU inner dim must be a multiple of 32"
    idx = torch.arange(d, device=w.device).view(-1, 32)
    perm = torch.cat([idx, idx + d], dim=1).reshape(-1)     # [x0..x31, g0..g31, x32.., ...]
    return w[perm].contiguous(), (b[perm].contiguous() if b is not None else None)


def fold_layernorm(w, gamma, beta, bias=None):
    """nn.LayerNorm(gamma, beta) followed by nn.Linear(w [N, K], bias) as ONE projection of the un-normalised rows
    (VCX_GEMM_LNFOLD, include/vcx.h):  LN(x) w^T + bias = rstd (x w'^T - mean colsum) + bias'  with
    w' = gamma o w rounded to fp16, colsum = the fp32 row sums of that ROUNDED w' (so that x w'^T - mean colsum is
    sum_k (x_k - mean) w'_k exactly, whatever the common offset of the row), bias' = bias + w beta in fp32.
    Returns (w' fp16, colsum fp32, bias' fp32)."""
    w32, g32, b32 = w.detach().float(), gamma.detach().float(), beta.detach().float()
    wf = (w32 * g32[None, :]).to(torch.float16)
    colsum = wf.double().sum(dim=1).float()        # exact sum of the fp16 values, rounded once
    bias_f = w32 @ b32
    if bias is not None:
        bias_f = bias_f + bias.detach().float()
    return wf.contiguous(), colsum.contiguous(), bias_f.contiguous()


def pack_ff_out_folded(w2, b2, wout, bout):
    """A transformer's last two linear layers have nothing between them (lvdm/modules/attention.py: ff.net[2] + block residual, then
    proj_out):  Wout (W2 g + b2 + t) + bout = [Wout W2 | Wout] [g ; t] + (Wout b2 + bout) - ONE GEMM over K = 4D + D whose last D columns
    read the token stream t (the K tail of a linear layer, include/vcx.h).  w2 [D, 4D], b2 [D], wout [C, D], bout [C] ->
    (wcat fp16 [C, 4D + D], bcat fp32 [C]).  The product is formed in fp64 from the fp16-ROUNDED W2 and Wout - the values the two-step
    form multiplies by - and rounded once; the bias in fp64 from the fp32 biases.  torch ops only: runs on meta tensors."""
    w2h, wouth = w2.detach().to(torch.float16), wout.detach().to(torch.float16)
    w2d, woutd = w2h.double(), wouth.double()
    wcat = torch.cat([(woutd @ w2d).to(torch.float16), wouth], dim=1).contiguous()
    bcat = (woutd @ b2.detach().float().double() + bout.detach().float().double()).float().contiguous()
    return wcat, bcat


def pack_mxfp8(w):
    """fp16 [rows, K] (K % 32 == 0) -> (element bytes uint8 [rows, Kp], scale bytes uint8 [rows, Kp / 32]), Kp = K rounded up to 128: the
    MXFP8 format of include/vcx.h ("MXFP8 operands") for weights, computed once at pack time with integer arithmetic on the fp16 bit
    patterns - byte for byte what vcx_quant_mxfp8_f16 writes for the same values (tests/test_mxfp8_gpu.py).  Runs on the host (the
    fp8 cast of every torch build, no device kernel) and returns tensors on w's device."""
    if w.dtype is not torch.float16 or w.dim() != 2 or w.shape[1] % 32 != 0:
        raise ValueError(f"pack_mxfp8: need an fp16 [rows, K] matrix with K % 32 == 0, got {w.dtype} {tuple(w.shape)}")
    rows, K = w.shape
    kp = (K + 127) // 128 * 128
    x = w.detach().cpu().contiguous()
    mag = (x.view(torch.int16).to(torch.int32) & 0x7FFF).view(rows, K // 32, 32).amax(dim=2)        # fp16 magnitudes order like their bits
    expo = mag >> 10
    lead = torch.zeros_like(mag)                     # position of a subnormal's leading mantissa bit
    for bit in range(1, 10):
        lead = torch.where(mag >> bit > 0, torch.full_like(mag, bit), lead)
    E = torch.where(expo > 0, expo - 15, lead - 24)
    bad, zero = mag >= 0x7C00, mag == 0
    scale = torch.where(bad, torch.full_like(E, 255), torch.where(zero, torch.zeros_like(E), E + 119))
    mul = torch.ldexp(torch.ones((), dtype=torch.float32), torch.where(bad | zero, torch.zeros_like(E), 8 - E))
    y = (x.float().view(rows, K // 32, 32) * mul[..., None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    y = torch.where(bad[..., None], torch.full_like(y, 0x7F), y)
    q = torch.zeros((rows, kp), dtype=torch.uint8)
    q[:, :K] = y.view(rows, K)
    s = torch.full((rows, kp // 32), 127, dtype=torch.uint8)
    s[:, :K // 32] = scale.to(torch.uint8)
    return q.to(w.device), s.to(w.device)


def pack_conv_t3_mxfp8(weight):
    """Conv3d weight [Cout, Cin, 3, 1, 1] (Cin % 32 == 0) -> (element bytes uint8 [Cout, 3 * Kp], scale bytes uint8 [Cout, 3 * Kp / 32]),
    Kp = Cin rounded up to 128: the weight operand of vcx_conv_t3_mxfp8 (include/vcx.h).  Tap-major - columns [tau Kp, tau Kp + Cin) are
    weight[:, :, tau] - and every tap is quantised and padded on its own with pack_mxfp8's rule (per 32-channel block inside the tap), so
    that no MX block and no 128-element K-step of the kernel straddles two taps.  The weight is rounded to fp16 first, as the fp16 route's
    pack_conv copy is."""
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 1, 1) or weight.shape[1] % 32 != 0:
        raise ValueError(f"pack_conv_t3_mxfp8: need a Conv3d weight [Cout, Cin, 3, 1, 1] with Cin % 32 == 0, got {tuple(weight.shape)}")
    cout, cin = weight.shape[:2]
    taps = weight.detach().reshape(cout, cin, 3).permute(0, 2, 1).to(torch.float16).contiguous()      # [Cout, 3, Cin]
    q, s = pack_mxfp8(taps.view(cout * 3, cin))
    return q.view(cout, -1).contiguous(), s.view(cout, -1).contiguous()


def pack_conv3x3_mxfp8(weight):
    """Conv2d weight [Cout, Cin, 3, 3] (Cin % 32 == 0) -> (element bytes uint8 [Cout, (Kp / 128) * 9 * 128], scale bytes uint8
    [Cout, (Kp / 128) * 9 * 4]), Kp = Cin rounded up to 128: the weight operand of vcx_conv3x3_mxfp8 (include/vcx.h).  Slab-major, for the
    reason conv_slab_major gives for the fp16 engine: the 128 columns at K-step 9 s + 3 ky + kx are channels 128 s .. 128 s + 127 of
    weight[:, :, ky, kx], so the nine tap re-reads of a tile's input rows are consecutive K-steps.  Every tap is quantised and padded on
    its own with pack_mxfp8's rule (per 32-channel block inside the tap): no MX block and no K-step straddles two taps.  The weight is
    rounded to fp16 first, as the fp16 route's pack_conv copy is."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[1] % 32 != 0:
        raise ValueError(f"pack_conv3x3_mxfp8: need a Conv2d weight [Cout, Cin, 3, 3] with Cin % 32 == 0, got {tuple(weight.shape)}")
    cout, cin = weight.shape[:2]
    taps = weight.detach().reshape(cout, cin, 9).permute(0, 2, 1).to(torch.float16).contiguous()      # [Cout, 9, Cin]
    q, s = pack_mxfp8(taps.view(cout * 9, cin))                                                        # [Cout * 9, Kp], [Cout * 9, Kp / 32]
    slabs = q.shape[1] // 128
    q = q.view(cout, 9, slabs, 128).permute(0, 2, 1, 3).reshape(cout, -1).contiguous()
    s = s.view(cout, 9, slabs, 4).permute(0, 2, 1, 3).reshape(cout, -1).contiguous()
    return q, s


def pack_conv3x3_tail_mxfp8(weight3x3, weight1x1):
    """Conv2d weights [Cout, Cin, 3, 3] and [Cout, Ct, 1, 1] (Cin % 32 == 0, Ct % 32 == 0) -> (element bytes uint8 [Cout, 9 Kp(Cin) + Kp(Ct)],
    scale bytes uint8 [Cout, (9 Kp(Cin) + Kp(Ct)) / 32]): the weight operand of vcx_conv3x3_tail_mxfp8 (include/vcx.h), a ResBlock's second
    convolution with its 1x1 skip convolution as a linear K tail.  The main columns are exactly pack_conv3x3_mxfp8(weight3x3), the tail
    columns pack_mxfp8 of the 1x1 weight rounded to fp16: the tail is quantised and padded on its own, so no MX block and no K-step
    straddles main and tail.  (The two biases are summed by the caller.)"""
    if weight1x1.dim() != 4 or tuple(weight1x1.shape[2:]) != (1, 1) or weight1x1.shape[1] % 32 != 0:
        raise ValueError(f"pack_conv3x3_tail_mxfp8: need a Conv2d weight [Cout, Ct, 1, 1] with Ct % 32 == 0 as the tail, got {tuple(weight1x1.shape)}")
    q, s = pack_conv3x3_mxfp8(weight3x3)
    if weight1x1.shape[0] != q.shape[0]:
        raise ValueError(f"pack_conv3x3_tail_mxfp8: {q.shape[0]} output channels in the 3x3 weight, {weight1x1.shape[0]} in the 1x1 weight")
    tq, ts = pack_mxfp8(weight1x1.detach().reshape(weight1x1.shape[0], -1).to(torch.float16).contiguous())
    return torch.cat([q, tq.to(q.device)], dim=1).contiguous(), torch.cat([s, ts.to(s.device)], dim=1).contiguous()
