"""The MXFP8 format of tests/mx_emulation.py on device tensors, for tensors of several GB (tests/test_mxfp8_large_extent_gpu.py).

tests/mx_emulation.py stays the definition (CPU only); tests/test_mxfp8_large_cpu.py holds quant_rows / dequant_rows, run on CPU tensors,
to it byte for byte.  What differs is the form, not the arithmetic:
  * rows go through in chunks, so that no fp32 temporary of the whole tensor exists;
  * the element rounding is written out - round to nearest even onto the e4m3 grid of the value's binade (quantum 2^(max(E, -6) - 3)) in
    fp32, where every step is exact - so that the final cast to float8_e4m3fn converts a representable value and cannot depend on how a
    device build of torch rounds; powers of two are put together from their exponent field (pow2), never computed by a device's pow();
  * the integer-grid operands are drawn on the device, different everywhere, and their fp64 values are never stored: dequant_rows gives
    them back per chunk.
No kernel of the library is called here."""
import torch

from tests import mx_emulation as MX

BLOCK, KPAD, E4M3_MAX = MX.BLOCK, MX.KPAD, MX.E4M3_MAX
DRAW = 1 << 28          # elements per draw of exact_operand_dev


def pow2(e, dtype=torch.float32):
    """2^e exactly, from the exponent field: e an integer tensor within the normal range of dtype (fp32: -126 .. 127)"""
    if dtype == torch.float32:
        return ((e.to(torch.int32) + 127) << 23).view(torch.float32)
    assert dtype == torch.float64
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def _e4m3_round(y):
    """fp32 |y| <= 448 -> the nearest e4m3fn value (ties to even), still fp32: normal binades 2^-6 .. 2^8 with 3 mantissa bits, subnormals
    on the 2^-9 grid.  y / quantum has at most 4 integer bits, so round() and both scalings are exact."""
    e = torch.frexp(y)[1] - 1                                  # floor(log2 |y|); frexp(0) = (0, 0) puts zero on the subnormal grid
    qe = e.clamp_min(-6) - 3
    return torch.round(y * pow2(-qe)) * pow2(qe)               # round(): half to even; the sign (of zero too) survives


def _quant_chunk(x, q, s):
    rows, K = x.shape
    nb = K // BLOCK
    xb = x.float().view(rows, nb, BLOCK)
    bad = ~torch.isfinite(xb).all(dim=2)
    xb = torch.where(bad[..., None], torch.zeros_like(xb), xb)
    amax = xb.abs().amax(dim=2)
    zero = amax == 0
    E = torch.where(zero, torch.zeros_like(amax, dtype=torch.int32), MX.block_exponent(amax.clamp_min(2.0 ** -30)))
    scale = torch.where(bad, torch.full_like(E, 255), torch.where(zero, torch.zeros_like(E), E - 8 + 127))
    mul = pow2(torch.where(zero | bad, torch.zeros_like(E), 8 - E))
    y = _e4m3_round((xb * mul[..., None]).clamp(-E4M3_MAX, E4M3_MAX)).to(torch.float8_e4m3fn).view(torch.uint8)
    y = torch.where(bad[..., None], torch.full_like(y, 0x7F), y)
    q[:, :K] = y.view(rows, K)
    s[:, :nb] = scale.to(torch.uint8)


def quant_rows(x, chunk=1 << 20):
    """mx_emulation.quant on the device of x: fp16 [rows, K] (K % 32 == 0, any row stride) -> (element bytes uint8 [rows, Kp], scale bytes
    uint8 [rows, Kp / 32]), `chunk` rows at a time."""
    assert x.dtype == torch.float16 and x.dim() == 2 and x.shape[1] % BLOCK == 0
    rows, K = x.shape
    kp = MX.kp_of(K)
    q = torch.zeros((rows, kp), dtype=torch.uint8, device=x.device)
    s = torch.full((rows, kp // BLOCK), 127, dtype=torch.uint8, device=x.device)
    for r0 in range(0, rows, chunk):
        _quant_chunk(x[r0:r0 + chunk], q[r0:r0 + chunk], s[r0:r0 + chunk])
    return q, s


def dequant_rows(q, s, K, dtype=torch.float64):
    """mx_emulation.dequant on the device of q, for the rows handed in (the caller passes a chunk): [rows, K] of float(element) 2^(s - 127),
    NaN under a NaN scale.  fp8 -> fp32 is exact in any implementation; fp32 -> dtype widens."""
    rows = q.shape[0]
    v = q[:, :K].contiguous().view(torch.float8_e4m3fn).float().to(dtype).view(rows, K // BLOCK, BLOCK)
    sc = s[:, :K // BLOCK].to(torch.int32)
    f = pow2(sc - 127, torch.float64).to(dtype)                # (2^-127, scale byte 0, is an fp32 subnormal: exact from fp64)
    f = torch.where(sc == 255, torch.full_like(f, float("nan")), f)
    return (v * f[..., None]).view(rows, K)


def int_table(device):
    """the 15 e4m3fn bytes of the integers -ELEM_MAX .. ELEM_MAX"""
    return MX.e4m3_bytes_of_ints(torch.arange(-MX.ELEM_MAX, MX.ELEM_MAX + 1)).to(device)


def exact_operand_dev(rows, K, seed, device, draw=DRAW, e_offset=0):
    """The on-device counterpart of mx_emulation.exact_operand: (q [rows, Kp], s [rows, Kp / 32]) with integer elements in [-7, 7] (as e4m3
    bytes through the 15-entry table) and scale exponents in {-1, 0, 1} per (row, block); K padding: element byte 0, scale byte 127.  One
    generator per tensor, `draw` elements at a time (whole rows; the scale bytes of those rows from the same generator right behind them),
    never a repeated block: the bytes at `offset mod 2^31` or `mod 2^32` are other draws.  The values are not returned - dequant_rows
    re-derives them per chunk.  `e_offset` moves every scale exponent, as in mx_emulation."""
    assert K % BLOCK == 0 and rows > 0
    g = torch.Generator(device=device).manual_seed(seed)
    kp, nb = MX.kp_of(K), K // BLOCK
    table = int_table(device)
    q = torch.zeros((rows, kp), dtype=torch.uint8, device=device)
    s = torch.full((rows, kp // BLOCK), 127, dtype=torch.uint8, device=device)
    step = max(1, draw // K)
    lo, hi = MX.EXPONENTS[0] + 127 + e_offset, MX.EXPONENTS[-1] + 127 + e_offset
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        idx = torch.randint(0, 2 * MX.ELEM_MAX + 1, (n, K), generator=g, device=device, dtype=torch.uint8)
        q[r0:r0 + n, :K] = torch.take(table, idx.long())
        del idx
        s[r0:r0 + n, :nb] = torch.randint(lo, hi + 1, (n, nb), generator=g, device=device, dtype=torch.uint8)
    return q, s


def exact_addend_dev(shape, seed, device, dtype, span=256, draw=DRAW):
    """Multiples of GRID in [-span GRID, span GRID] (bias, residual, row addend of an exact problem), drawn on the device as above."""
    g = torch.Generator(device=device).manual_seed(seed)
    t = torch.empty(shape, dtype=dtype, device=device)
    flat = t.view(-1)
    for i in range(0, flat.numel(), draw):
        n = min(draw, flat.numel() - i)
        flat[i:i + n] = (torch.randint(-span, span + 1, (n,), generator=g, device=device, dtype=torch.int32).float() * MX.GRID).to(dtype)
    return t
