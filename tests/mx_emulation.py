"""The MXFP8 format of include/vcx.h ("MXFP8 operands") in torch, on the CPU: the definition that vcx_quant_mxfp8_f16,
vcx_layernorm_mxfp8_f16, the quantising GEGLU epilogue of vcx_gemm_mxfp8 and packing.pack_mxfp8 are compared with byte for byte, and
the operands with exactly known products for tests/test_mxfp8_gpu.py (conditions checked by tests/test_mxfp8_cpu.py).  No GPU code.

A block is 32 consecutive K-elements of a row.  amax = max |x| (exact); E = floor(log2 amax), here from torch.frexp of the fp32 value
(exact for fp16 subnormals too - another route to the same integer than the kernels' exponent-field arithmetic); scale byte
s = E - 8 + 127 (0 for an all-zero block, 0xFF for a block with a non-finite value, whose element bytes are all 0x7F); element byte =
e4m3fn round-to-nearest-even of clamp(x 2^(8 - E), -448, 448).  `x.clamp(-448, 448).to(torch.float8_e4m3fn)` is that saturating cast
(without the clamp torch returns NaN above 464).  K extents are padded to a multiple of 128 with element bytes 0 and scale bytes 127.
"""
import torch

BLOCK = 32
KPAD = 128
E4M3_MAX = 448.0


def kp_of(K):
    return (K + KPAD - 1) // KPAD * KPAD


def block_exponent(amax_f32):
    """floor(log2 amax) of a positive finite fp32 tensor: frexp gives amax = m 2^e with m in [0.5, 1)."""
    return torch.frexp(amax_f32)[1].to(torch.int32) - 1


def quant(x):
    """fp16 [rows, K] (CPU, K % 32 == 0) -> (element bytes uint8 [rows, Kp], scale bytes uint8 [rows, Kp / 32])."""
    assert x.dtype == torch.float16 and x.dim() == 2 and x.shape[1] % BLOCK == 0 and not x.is_cuda
    rows, K = x.shape
    nb, kp = K // BLOCK, kp_of(K)
    xb = x.float().view(rows, nb, BLOCK)
    bad = ~torch.isfinite(xb).all(dim=2)
    amax = torch.where(bad[..., None], torch.zeros_like(xb), xb).abs().amax(dim=2)
    zero = amax == 0
    E = torch.where(zero, torch.zeros_like(amax, dtype=torch.int32), block_exponent(amax.clamp_min(2.0 ** -30)))
    scale = torch.where(bad, torch.full_like(E, 255), torch.where(zero, torch.zeros_like(E), E - 8 + 127))
    mul = torch.ldexp(torch.ones((), dtype=torch.float32), torch.where(zero | bad, torch.zeros_like(E), 8 - E))
    y = (torch.where(bad[..., None], torch.zeros_like(xb), xb) * mul[..., None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    y = torch.where(bad[..., None], torch.full_like(y, 0x7F), y)
    q = torch.zeros((rows, kp), dtype=torch.uint8)
    q[:, :K] = y.reshape(rows, K)
    s = torch.full((rows, kp // BLOCK), 127, dtype=torch.uint8)
    s[:, :nb] = scale.to(torch.uint8)
    return q, s


def dequant(q, s, K, dtype=torch.float64):
    """The values an MXFP8 pair represents, [rows, K]: float(element) * 2^(s - 127)  (NaN scale: NaN)."""
    q, s = q.cpu(), s.cpu()
    rows = q.shape[0]
    v = q[:, :K].contiguous().view(torch.float8_e4m3fn).to(dtype).view(rows, K // BLOCK, BLOCK)
    sc = s[:, :K // BLOCK].to(torch.int32)
    f = torch.ldexp(torch.ones((), dtype=dtype), sc - 127)
    f = torch.where(sc == 255, torch.full_like(f, float("nan")), f)
    return (v * f[..., None]).view(rows, K)


def boundary_blocks():
    """name -> (32 fp16 values, expected scale byte, {element index: expected byte}) for the edges of the format."""
    def blk(fill, **at):
        v = torch.full((BLOCK,), fill, dtype=torch.float32)
        for i, val in at.items():
            v[int(i[1:])] = val
        return v.half()
    sub = 2.0 ** -24
    return {
        # amax exactly a power of two: E = 3, s = 122, factor 2^5: 8 -> 256 = 0x78 (2^8: exponent field 15, mantissa 0)
        "pow2": (blk(0.5, _0=8.0, _1=-8.0, _2=1.0), 122, {0: 0x78, 1: 0xF8, 2: 0x60, 3: 0x58}),
        # amax = 15.5: E = 3, factor 32: 496 is in (448, 512) and clamps to 448 = 0x7E; 14.5 * 32 = 464 rounds (ties to even) to 448 too
        "clamp": (blk(1.0, _0=15.5, _1=-15.5, _2=14.5, _3=14.0), 122, {0: 0x7E, 1: 0xFE, 2: 0x7E, 3: 0x7E, 4: 0x60}),
        # an fp16-subnormal amax: 3 * 2^-24: E = -23, s = 96, factor 2^31: 3 * 2^7 = 384 = 0x7C, 2^-24 -> 128 = 0x70
        "subnormal": (blk(0.0, _0=3 * sub, _1=-sub, _5=2 * sub), 96, {0: 0x7C, 1: 0xF0, 5: 0x78, 2: 0x00}),
        # the smallest amax of all, 2^-24: E = -24, s = 95, factor 2^32: 256 = 0x78
        "min_subnormal": (blk(0.0, _7=sub), 95, {7: 0x78, 0: 0x00}),
        # the largest finite amax, 65504: E = 15, s = 134, factor 2^-7: 511.75 clamps to 448
        "max_finite": (blk(1.0, _0=65504.0, _1=-32768.0), 134, {0: 0x7E, 1: 0xF8}),
        "zero": (blk(0.0), 0, {0: 0x00, 31: 0x00}),
        "neg_zero": (blk(0.0, _3=-0.0), 0, {3: 0x80, 0: 0x00}),
        # e4m3 subnormals of a block with a large maximum: factor 2^0 at amax 256 .. 511: 1.5 * 2^-10 -> 2^-9 = 0x01, 2^-10 -> 0 (tie to even)
        "tiny_elements": (blk(0.0, _0=256.0, _1=1.5 * 2.0 ** -10, _2=2.0 ** -10, _3=-(2.0 ** -9), _4=3 * 2.0 ** -10), 127, {0: 0x78, 1: 0x01, 2: 0x00, 3: 0x81, 4: 0x02}),
        "inf": (blk(1.0, _9=float("inf")), 255, {0: 0x7F, 9: 0x7F}),
        "nan": (blk(1.0, _2=float("nan")), 255, {0: 0x7F, 2: 0x7F}),
    }


def plant_boundaries(x):
    """Writes the boundary blocks into known places of x (fp16 [rows, K], rows >= 2 * count, K >= 64): block `i` into row 2 i + 1, K-block
    (i mod (K / 32)).  Returns {name: (row, block)}."""
    where = {}
    nb = x.shape[1] // BLOCK
    for i, (name, (v, _, _)) in enumerate(boundary_blocks().items()):
        r, b = 2 * i + 1, i % nb
        x[r, b * BLOCK:(b + 1) * BLOCK] = v
        where[name] = (r, b)
    return where


# ------------------------------------------------------------------------------------------------------------------ exact GEMM operands
# Elements are integers in [-7, 7] (every one an exact e4m3 value: 3 significant bits), block scale exponents in {-1, 0, 1} on each
# operand, drawn per (row, block).  A product is then (integer of magnitude <= 49) x 2^(ea + ew) with ea + ew in [-2, 2]: a multiple of
# 2^-2 of magnitude <= 196.  At K = 1280 every partial sum, in any order, is a multiple of 2^-2 below 1280 x 196 = 250880 < 2^24 x 2^-2:
# exact in fp32 whatever the summation order, the tile or the lane map - and one swapped block or misplaced scale byte is an exact
# mismatch.  W is asymmetric by construction (independent draws per row and column, scales per (row, block)).
ELEM_MAX = 7
EXPONENTS = (-1, 0, 1)
PRODUCT_MAX = ELEM_MAX * ELEM_MAX * 4
GRID = 0.25


def e4m3_bytes_of_ints(v):
    """int tensor in [-7, 7] -> the e4m3fn bytes that hold exactly those integers."""
    f8 = v.to(torch.float32).to(torch.float8_e4m3fn)
    assert torch.equal(f8.float(), v.float())
    return f8.view(torch.uint8)


def exact_operand(rows, K, seed, elem_max=ELEM_MAX, e_offset=0):
    """(q [rows, Kp], s [rows, Kp / 32], values fp64 [rows, K]) of a random operand under the conditions above.  `e_offset` moves every
    scale exponent by the same amount (the whole problem by a power of two: nothing about exactness changes)."""
    g = torch.Generator().manual_seed(seed)
    kp = kp_of(K)
    v = torch.randint(-elem_max, elem_max + 1, (rows, K), generator=g)
    e = torch.randint(EXPONENTS[0], EXPONENTS[-1] + 1, (rows, K // BLOCK), generator=g) + e_offset
    q = torch.zeros((rows, kp), dtype=torch.uint8)
    q[:, :K] = e4m3_bytes_of_ints(v)
    s = torch.full((rows, kp // BLOCK), 127, dtype=torch.uint8)
    s[:, :K // BLOCK] = (e + 127).to(torch.uint8)
    val = v.double().view(rows, K // BLOCK, BLOCK) * torch.exp2(e.double())[..., None]
    return q, s, val.view(rows, K)
