"""The MXFP8 kernel family where byte offsets pass 2 GiB: the 16 instantiations of gemm_mx_kernel behind vcx_gemm_mxfp8, vcx_conv_t3_mxfp8,
vcx_conv3x3_mxfp8 and vcx_conv3x3_tail_mxfp8 (32-bit buffer offsets, zero fill by the descriptors' range check, a tile grid that reaches 127
rows past M), the quantisers and the quantising attention kernels (64-bit indexing).  The cases, their regimes (`2g`, `lim`, `past_4g`) and
the slices are tests/mxfp8_large_cases.py; tests/test_mxfp8_large_cpu.py checks that table against the library's predicates.

Rule of the module, as in tests/test_large_extent_gpu.py - every comparison is a byte equality:
  (a) the exact forms (linear, temporal, 3x3 and tailed calls with BIAS_N, RESIDUAL or ROWADD epilogues on integer-grid operands): EVERY
      output row bit for bit against an fp64 reference formed on the device in row chunks - dequant_rows(..., float64) operands, one fp64
      matmul per tap over explicitly shifted, zero-filled source rows (fp64 on purpose: nothing here relies on an fp32 matmul being exact);
  (b) every large call of every form byte for byte against the same entry point called on slices whose buffers all stay below 2^31 bytes
      (row ranges, whole videos, whole frames, whole groups): output, output scales and column moments.  GEGLU, COLSTATS, the quantisers
      and the attention kernels have only this check and (c);
  (c) the quantising kernels against quant_rows (tests/mx_device_ref.py) of the fp16 kernel's output over the whole tensor, the raw second
      output of the `_raw` GroupNorm forms against quant_rows of the input;
  (d) outputs sit between sentinel guard rows, with sentinel guard columns where ldc > N: untouched;
  (e) gathered `lim` cases first compare, by name, the rows whose taps must read zero.
Operands are different everywhere (one device generator per tensor, never a tiled block): a read from `offset mod 2^31` or `mod 2^32`
fetches other bytes."""
import time

import pytest
import torch

from tests import mx_device_ref as D
from tests import mx_emulation as MX
from tests import mxfp8_large_cases as C
from tests.test_large_extent_gpu import _t, edges, need
from tests.test_mxfp8_sattn_gpu import _knobs

pytestmark = pytest.mark.gpu
DEV = "cuda"
GIB = 1 << 30
GUARD = 64                    # sentinel rows in front of and behind every output
SENT16, SENT8, SENT32 = 777.0, 0xAB, 7.0
CHUNK = 1 << 16               # rows per reference chunk
ids = lambda cases: [c["id"] for c in cases]


@pytest.fixture(autouse=True)
def _memory_report(request):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"\n[mxfp8-large] {request.node.name}: peak {torch.cuda.max_memory_allocated() / GIB:.2f} GiB, {time.time() - t0:.1f} s")
    torch.cuda.empty_cache()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """[GUARD + rows + GUARD, ld] of `dtype` filled with a sentinel; .mid = the rows a kernel may write"""

    def __init__(self, rows, ld, dtype, tail=()):
        self.rows, self.sent = rows, {torch.float16: SENT16, torch.uint8: SENT8, torch.float32: SENT32}[dtype]
        self.buf = torch.full((rows + 2 * GUARD, ld) + tuple(tail), self.sent, dtype=dtype, device=DEV)
        self.mid = self.buf[GUARD:GUARD + rows]

    def check(self, name, cols=None):
        """(d): guard rows, and the columns from `cols` on, still hold the sentinel"""
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == self.sent).all()), f"{name}: the guard rows in front were written"
        assert bool((self.buf[GUARD + self.rows:] == self.sent).all()), f"{name}: the guard rows behind were written"
        if cols is not None and cols < self.buf.shape[1]:
            for r0 in range(0, self.rows, 1 << 22):
                assert bool((self.mid[r0:r0 + (1 << 22), cols:] == self.sent).all()), f"{name}: guard columns written in rows {r0}..."


def same_bytes(got, want, name, rows_per=1 << 22):
    """byte equality of two 2-d tensors, in row blocks; the first difference by row and column"""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    gv, wv = (t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32) if t.dtype == torch.float32 else t for t in (got, want))
    for r0 in range(0, got.shape[0], rows_per):
        g, w = gv[r0:r0 + rows_per], wv[r0:r0 + rows_per]
        if not torch.equal(g, w):
            bad = (g != w).reshape(g.shape[0], -1)
            r = int(bad.any(dim=1).nonzero()[0])
            col = int(bad[r].nonzero()[0])
            raise AssertionError(f"{name}: {int(bad.sum())} elements differ in rows {r0} .. {r0 + g.shape[0]}; first at row {r0 + r} (byte offset "
                                 f"{(r0 + r) * got.stride(0) * got.element_size()}), column {col}: got {got[r0 + r].reshape(-1)[col].item()!r}, "
                                 f"want {want[r0 + r].reshape(-1)[col].item()!r}")


# ------------------------------------------------------------------------------------------------------------------ the reference on the device
def test_device_reference_on_the_device_equals_the_definition():
    """tests/test_mxfp8_large_cpu.py holds quant_rows / dequant_rows to the definition on CPU tensors; here the same functions on device
    tensors against the definition on the CPU (every fp16 bit pattern, shuffled, and the planted edges), and exact_operand_dev's
    conditions for device draws, with the blocks at byte offsets 0 and 2^31 of a long operand different."""
    allh = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    x = torch.cat([allh.view(-1, 64), allh[torch.randperm(65536, generator=torch.Generator().manual_seed(1))].view(-1, 64)])
    MX.plant_boundaries(x)
    q, s = MX.quant(x)
    qd, sd = D.quant_rows(x.to(DEV), chunk=777)
    same_bytes(qd.cpu(), q, "quant_rows on the device, elements")
    same_bytes(sd.cpu(), s, "quant_rows on the device, scales")
    a, b = MX.dequant(q, s, 64), D.dequant_rows(qd, sd, 64).cpu()
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    rows = C.G31 // 1024 + 8
    eq, es = D.exact_operand_dev(rows, 1024, C.SEED_A, DEV)
    flat = eq.view(-1)
    assert not torch.equal(flat[:4096], flat[C.G31:C.G31 + 4096]), "the bytes at offsets 0 and 2^31 are equal"
    head = eq[:4096].contiguous().view(torch.float8_e4m3fn).float()
    assert torch.equal(head, head.round()) and float(head.abs().max()) == MX.ELEM_MAX and len(torch.unique(head)) == 15
    assert set(torch.unique(es).tolist()) == {126, 127, 128}
    assert torch.unique(eq[-4096:], dim=0).shape[0] == 4096, "rows repeat"


# ------------------------------------------------------------------------------------------------------------------ the matrix kernels
def _flags(c):
    from viewcrafter_amd import ops as G
    names = dict(residual=G.GEMM_RESIDUAL, geglu=G.GEMM_GEGLU, mx_out=G.GEMM_MXFP8_OUT, rowadd=G.GEMM_ROWADD, colstats=G.GEMM_COLSTATS)
    f = G.GEMM_BIAS_N
    for n in c["flags"]:
        f |= names[n]
    return f


class Problem:
    """The operands of a GEMM case on the device.  Activation (and tail source) from exact_operand_dev, residual and row addend multiples of
    GRID drawn on the device, weights and bias from the CPU (mxfp8_large_cases.weights)."""

    def __init__(self, c):
        self.c = c
        self.M, self.per, self.units, self.taps, _ = C.geometry(c)
        self.K, self.N, self.nout = C.k_of(c), c["N"], C.n_out(c)
        self.ldc, self.ldr = C.pitches(c)
        M = self.M
        self.a = D.exact_operand_dev(M, self.K, C.SEED_A, DEV)
        self.t = D.exact_operand_dev(M, c["Ct"], C.SEED_T, DEV, e_offset=1) if c["form"] == "tail" else None
        pair, vals, bias = C.weights(c)
        self.w = (pair[0].to(DEV), pair[1].to(DEV))
        self.wv = tuple(v.to(DEV) for v in vals) if c["form"] == "tail" else (vals.to(DEV), None)
        self.bias = bias.to(DEV)
        self.res = D.exact_addend_dev((M, self.ldr), C.SEED_R, DEV, torch.float16)[:, :self.nout] if self.ldr else None
        self.rowadd = D.exact_addend_dev((self.units, self.N), C.SEED_RA, DEV, torch.float32) if "rowadd" in c["flags"] else None
        self.mx_out, self.colstats = "mx_out" in c["flags"], "colstats" in c["flags"]

    def outputs(self, rows):
        """guarded (output, output scales or None, column moments or None) for a call on `rows` rows"""
        c = self.c
        if self.mx_out:
            kpo = MX.kp_of(self.nout)
            return Guarded(rows, kpo, torch.uint8), Guarded(rows, kpo // 32, torch.uint8), None
        return Guarded(rows, self.ldc, torch.float16), None, Guarded(rows // 64, c["ldcs"], torch.float32, tail=(2,)) if self.colstats else None

    def run(self, lo, hi, outs):
        """the case's entry point on slice units [lo, hi) into `outs`"""
        from viewcrafter_amd import _lib, ops
        c, per = self.c, self.per
        r0, r1 = lo * per, hi * per
        m = r1 - r0
        a = (self.a[0][r0:r1], self.a[1][r0:r1])
        res = None if self.res is None else self.res[r0:r1]
        out, out_s, cs = outs
        kw = {}
        if cs is not None:
            kw = dict(colstats=cs.mid, colstats_ld=c["ldcs"], colstats_col=c["cs_col"])
        if c["form"] == "linear":
            ops.check(_lib.lib().vcx_gemm_mxfp8(a[0].data_ptr(), a[1].data_ptr(), self.w[0].data_ptr(), self.w[1].data_ptr(), out.mid.data_ptr(),
                                                None if out_s is None else out_s.mid.data_ptr(), self.bias.data_ptr(), None if res is None else res.data_ptr(),
                                                m, self.N, self.K, self.nout if self.mx_out else self.ldc, self.ldr, _flags(c), _stream()), c["id"])
        elif c["form"] == "t3":
            ops.temporal_conv3_mxfp8(a, self.w, self.bias, B=hi - lo, T=c["T"], P=c["P"], cin=self.K, residual=res, out=out.mid, **kw)
        elif c["form"] == "c9":
            ra = None if self.rowadd is None else self.rowadd[lo:hi]
            ops.conv3x3_mxfp8(a, self.w, self.bias, n=hi - lo, H=c["H"], W=c["W"], cin=self.K, rowadd=ra, rowadd_div=c.get("rowadd_div", 0), residual=res,
                              out=out.mid, **kw)
        else:
            ops.conv3x3_tail_mxfp8(a, (self.t[0][r0:r1], self.t[1][r0:r1]), self.w, self.bias, n=hi - lo, H=c["H"], W=c["W"], cin=self.K, ct=c["Ct"],
                                   out=out.mid, **kw)
        return outs

    def check_guards(self, outs, name):
        out, out_s, cs = outs
        out.check(f"{name} output", None if self.mx_out else self.nout)
        if out_s is not None:
            out_s.check(f"{name} output scales")
        if cs is not None:
            cs.check(f"{name} column moments")
            col = self.c["cs_col"]
            assert bool((cs.mid[:, :col] == SENT32).all()) and bool((cs.mid[:, col + self.N:] == SENT32).all()), f"{name}: moments outside their columns"

    # -------------------------------------------------------------------------------------------------------------- (a)
    def tap(self, idx, tap):
        """(distance in rows of the tap's source row, the source row exists inside the row's own video / frame) for output rows idx"""
        c = self.c
        if c["form"] == "linear":
            return 0, None
        if c["form"] == "t3":
            t = (idx // c["P"]) % c["T"] + (tap - 1)
            return (tap - 1) * c["P"], (t >= 0) & (t < c["T"])
        ky, kx = divmod(tap, 3)
        y, x = (idx // c["W"]) % c["H"] + (ky - 1), idx % c["W"] + (kx - 1)
        return (ky - 1) * c["W"] + (kx - 1), (y >= 0) & (y < c["H"]) & (x >= 0) & (x < c["W"])

    def ref(self, idx):
        """fp64: the output rows idx (int64 on the device) from the dequantised operands, tap by tap, source rows shifted and zero-filled"""
        w, wt = self.wv
        ref = self.bias.double().unsqueeze(0).repeat(idx.numel(), 1)
        for tap in range(self.taps):
            d, exists = self.tap(idx, tap)
            src = idx + d
            if exists is not None:
                src = torch.where(exists, src, idx)
            assert int(src.min()) >= 0 and int(src.max()) < self.M
            x = D.dequant_rows(self.a[0][src], self.a[1][src], self.K)
            if exists is not None:
                x = torch.where(exists.unsqueeze(1), x, torch.zeros_like(x))
            ref += x @ w[:, tap].t()
        if wt is not None:
            ref += D.dequant_rows(self.t[0][idx], self.t[1][idx], self.c["Ct"]) @ wt.t()
        if self.rowadd is not None:
            ref += self.rowadd[idx // self.c["rowadd_div"]].double()
        if self.res is not None:
            ref += self.res[idx].double()
        assert float(ref.abs().max()) < 65504, "the reference leaves fp16"
        return ref

    def where(self, r):
        c = self.c
        if c["form"] == "linear":
            return f"row {r}"
        if c["form"] == "t3":
            return f"row {r} = (video {r // (c['T'] * c['P'])}, t {(r // c['P']) % c['T']}, pixel {r % c['P']})"
        return f"row {r} = (frame {r // (c['H'] * c['W'])}, y {(r // c['W']) % c['H']}, x {r % c['W']})"

    def check_rows(self, out, idx, name):
        want = self.ref(idx).half()
        got = out[idx, :self.N]
        if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
            bad = (got.view(torch.int16) != want.view(torch.int16))
            i = int(bad.any(dim=1).nonzero()[0])
            r, col = int(idx[i]), int(bad[i].nonzero()[0])
            raise AssertionError(f"{self.c['id']}, {name}: {int(bad.any(dim=1).sum())} of {idx.numel()} rows differ from fp64; first {self.where(r)} at byte "
                                 f"{r * MX.kp_of(self.K)} of the activation, column {col}: got {float(got[i, col])}, want {float(want[i, col])}")

    def check_every_row(self, out):
        for r0 in range(0, self.M, CHUNK):
            self.check_rows(out, torch.arange(r0, min(r0 + CHUNK, self.M), device=DEV), f"rows {r0}...")

    # -------------------------------------------------------------------------------------------------------------- (e)
    def spots(self):
        """[(name, rows)]: rows whose taps must read zero - the first and last frame of the first and last video (t3), the border pixels of
        the first and last frame (3x3) - and the rows around byte 2^31 (and, where the buffer is that long, 2^32 - reach Kp) of the activation"""
        c, kp = self.c, MX.kp_of(self.K)
        ar = lambda n: torch.arange(n, device=DEV)
        out = []
        if c["form"] == "t3":
            T, P = c["T"], c["P"]
            for b in sorted({0, c["B"] - 1}):
                out.append((f"video {b}, t = 0: the tap at t - 1 must read zero, not video {b - 1}", (b * T) * P + ar(P)))
                out.append((f"video {b}, t = T - 1: the tap at t + 1 must read zero, not video {b + 1}", (b * T + T - 1) * P + ar(P)))
            reach = P
        else:
            H, W = c["H"], c["W"]
            for f in sorted({0, c["n"] - 1}):
                base = f * H * W
                out.append((f"frame {f}, y = 0: the taps at y - 1 must read zero, not frame {f - 1}", base + ar(W)))
                out.append((f"frame {f}, y = H - 1: the taps at y + 1 must read zero, not frame {f + 1}", base + (H - 1) * W + ar(W)))
                out.append((f"frame {f}, x = 0: the taps at x - 1 must read zero, not the image row above", base + ar(H) * W))
                out.append((f"frame {f}, x = W - 1: the taps at x + 1 must read zero, not the image row below", base + ar(H) * W + (W - 1)))
            reach = W + 1
        # the row ranges straddling bytes 2^31 and 2^32 of the activation (edges: where it is that long), wide enough for every tap of their rows
        for lo, hi in edges(self.M, kp, span=2 * (reach + 128))[1:-1]:
            out.append((f"rows {lo} .. {hi}, whose taps straddle byte {'2^31' if lo * kp < C.G31 else '2^32'} of the activation", torch.arange(lo, hi, device=DEV)))
        r = (C.G32 - reach * kp) // kp
        if r + reach + 128 < self.M:
            out.append(("the rows whose farthest tap straddles byte 2^32 - reach Kp of the activation", torch.arange(r - 128, r + reach + 128, device=DEV)))
        return out


@pytest.mark.parametrize("c", C.GEMM_CASES, ids=ids(C.GEMM_CASES))
def test_matrix_kernel(c):
    need(2.6 * max(C.buffer_bytes(c).values()) / GIB + 4)
    p = Problem(c)
    big = p.run(0, p.units, p.outputs(p.M))
    p.check_guards(big, "the large call")                                                                        # (d)
    assert C.in_regime(C.named_extent(c), c["regime"])
    out, out_s, cs = big
    if c["exact"]:
        if c["regime"] == "lim" and c["form"] != "linear":
            for name, rows in p.spots():                                                                         # (e)
                p.check_rows(out.mid, rows, name)
        p.check_every_row(out.mid)                                                                               # (a)
    for lo, hi in C.slices(c):                                                                                   # (b)
        r0, r1 = lo * p.per, hi * p.per
        part = p.run(lo, hi, p.outputs(r1 - r0))
        name = f"{c['id']}: units {lo} .. {hi} (rows {r0} .. {r1}) called alone"
        p.check_guards(part, name)
        cols = part[0].mid.shape[1] if p.mx_out else p.nout
        same_bytes(out.mid[r0:r1, :cols], part[0].mid[:, :cols], name + ", output")
        if out_s is not None:
            same_bytes(out_s.mid[r0:r1], part[1].mid, name + ", output scales")
        if cs is not None:
            same_bytes(cs.mid[r0 // 64:r1 // 64].reshape(-1, 2 * c["ldcs"]), part[2].mid.reshape(-1, 2 * c["ldcs"]), name + ", column moments")
        del part
    if p.mx_out:
        assert len(torch.unique(out_s.mid[:4096])) > 3, "the data should spread over several scale bytes"


# ------------------------------------------------------------------------------------------------------------------ the quantisers
def _plant(x):
    """the format's edges into the first rows and into the rows around byte offsets 2^31 and 2^32 of q (Kp = 128)"""
    for r in (0, C.G31 // 128 - 10, C.G32 // 128 - 10):
        if r + 32 <= x.shape[0]:
            MX.plant_boundaries(x[r:r + 32])


def _quantiser_outputs(rows):
    return Guarded(rows, 128, torch.uint8), Guarded(rows, 4, torch.uint8)


def _check_pair(got, want, name):
    for g, w, part in zip(got, want, ("elements (+ padding)", "scales (+ padding)")):
        g.check(f"{name} {part}")
        same_bytes(g.mid, w, f"{name} {part}")


@pytest.mark.parametrize("c", [c for c in C.QUANT_CASES if c["form"] in ("quant", "layernorm")], ids=lambda c: c["id"])
def test_row_quantiser(c):
    """vcx_quant_mxfp8_f16 (K = 64 of a row pitch of 72: half of every q row is padding) and vcx_layernorm_mxfp8_f16 at C = 64 with q past
    2^31 and past 2^32 bytes: (c) against quant_rows of the input / of vcx_layernorm_f16's output, (b) row ranges called alone."""
    from viewcrafter_amd import _lib, ops
    L = _lib.lib()
    rows, K = c["rows"], c["K"]
    need(4.5 * rows * 128 / GIB + 2)
    if c["form"] == "quant":
        x = _loud_rows(_t((rows, c["ldx"]), 301, 2.0, 0.3), 305, 0)[:, :K]
        _plant(x)
        call = lambda xs, q, s: ops.check(L.vcx_quant_mxfp8_f16(xs.data_ptr(), xs.stride(0), q.mid.data_ptr(), s.mid.data_ptr(), xs.shape[0], K, _stream()), c["id"])
        want = D.quant_rows(x)
    else:
        x = _t((rows, K), 302, 2.0, 0.5)
        g, b = 1 + _t((K,), 303, 0.2, dtype=torch.float32), _t((K,), 304, 0.1, dtype=torch.float32)
        call = lambda xs, q, s: ops.check(L.vcx_layernorm_mxfp8_f16(xs.data_ptr(), q.mid.data_ptr(), s.mid.data_ptr(), g.data_ptr(), b.data_ptr(), xs.shape[0], K,
                                                                    1e-5, _stream()), c["id"])
        want = D.quant_rows(ops.layer_norm(x, g, b))
    big = _quantiser_outputs(rows)
    call(x, *big)
    assert C.in_regime(big[0].mid.numel(), c["regime"])
    _check_pair(big, want, c["id"])                                                                               # (c), (d)
    del want
    for lo, hi in C.quant_slices(c):                                                                             # (b)
        part = _quantiser_outputs(hi - lo)
        call(x[lo:hi], *part)
        _check_pair(part, (big[0].mid[lo:hi], big[1].mid[lo:hi]), f"{c['id']}: rows {lo} .. {hi} called alone")
        del part


@pytest.mark.parametrize("c", [c for c in C.QUANT_CASES if c["form"] == "groupnorm"], ids=lambda c: c["id"])
def test_groupnorm_quantiser(c):
    """vcx_groupnorm_apply[2]_mxfp8[_raw]_f16 at (3, 12 000 000, 64): frame 1 straddles byte 2^31 of q, frame 2 byte 2^32.  (c) against
    quant_rows of vcx_groupnorm_apply[2]_f16's output - the raw pair against quant_rows of the input -, (b) every frame called alone."""
    from viewcrafter_amd import _lib, ops
    L = _lib.lib()
    n, pix, K, c1, groups, raw = c["n_outer"], c["pixels"], c["K"], c["c1"], c["groups"], c["raw"]
    rows = n * pix
    need((7 if raw else 5) * rows * 128 / GIB + 2)
    x1 = _t((n, pix, c1), 311, 2.0, 0.3)
    x2 = _t((n, pix, K - c1), 312, 0.5, -1.0) if c1 < K else None
    g, b = 1 + _t((K,), 313, 0.2, dtype=torch.float32), _t((K,), 314, 0.1, dtype=torch.float32)
    xc = x1 if x2 is None else torch.cat([x1, x2], dim=2)
    stats = ops.group_norm_stats(xc, groups)

    def call(lo, hi, outs):
        ptrs = [o.mid.data_ptr() for o in outs] + [stats[lo:hi].data_ptr(), g.data_ptr(), b.data_ptr(), hi - lo, pix, K, groups, 1e-5, 1, _stream()]
        name = f"vcx_groupnorm_apply{'' if x2 is None else '2'}_mxfp8{'_raw' if raw else ''}_f16"
        head = [x1[lo:hi].data_ptr()] if x2 is None else [x1[lo:hi].data_ptr(), c1, x2[lo:hi].data_ptr()]
        ops.check(getattr(L, name)(*head, *ptrs), name)

    outputs = lambda r: _quantiser_outputs(r) + (_quantiser_outputs(r) if raw else ())
    big = outputs(rows)
    call(0, n, big)
    assert pix * 128 < C.G31 < 2 * pix * 128 < C.G32 < rows * 128
    want = D.quant_rows(ops.group_norm(x1, g, b, 1e-5, True, groups=groups, stats=stats, x2=x2).view(rows, K))
    _check_pair(big[:2], want, c["id"])                                                                           # (c), (d)
    del want
    if raw:
        _check_pair(big[2:], D.quant_rows(xc.view(rows, K)), c["id"] + ", the raw pair")
    del xc
    for lo, hi in C.quant_slices(c):                                                                             # (b)
        part = outputs((hi - lo) * pix)
        call(lo, hi, part)
        for j in range(0, len(part), 2):
            _check_pair(part[j:j + 2], tuple(o.mid[lo * pix:hi * pix] for o in big[j:j + 2]), f"{c['id']}: frames {lo} .. {hi} called alone, pair {j // 2}")
        del part


# ------------------------------------------------------------------------------------------------------------------ the quantising attention
def _loud_rows(t, seed, dim):
    """scales the rows (dim 0) or columns (dim 1) of t by binades 2^-6 .. 2^6 of their own: the output blocks then get many scale bytes"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    shape = (t.shape[0], 1) if dim == 0 else (1, t.shape[1])
    f = torch.exp2(torch.randint(-6, 7, shape, generator=g, device=DEV).float()).half()
    for r0 in range(0, t.shape[0], 1 << 22):
        t[r0:r0 + (1 << 22)] *= f[r0:r0 + (1 << 22)] if dim == 0 else f
    return t


@pytest.mark.parametrize("c", [c for c in C.ATTN_CASES if c["form"] == "tattn"], ids=lambda c: c["id"])
def test_temporal_attention_quantiser(c):
    """vcx_attn_temporal_d64_mxfp8 at B = 1, T = 2, P = 2^23 + 4096 (output rows x Kp = 2 148 532 224 bytes; heads = 1: Kp = 128, the odd-head
    padding stores): (c) against quant_rows of vcx_attn_temporal_d64[_masked]_f16 with the same arguments, (b) pixel ranges called alone."""
    from viewcrafter_amd import _lib, ops
    L = _lib.lib()
    B, T, P, heads, causal = c["B"], c["T"], c["P"], c["heads"], c["causal"]
    Dm, rows = 64 * heads, B * T * P
    kp = MX.kp_of(Dm)
    need((rows * 3 * Dm * 2 * 1.6 + rows * kp * 3.5) / GIB + 2)
    qkv = _t((rows, 3 * Dm), 321)
    _loud_rows(qkv[:, 2 * Dm:], 322, 0)

    def call(x, pixels, q, s):
        ops.check(L.vcx_attn_temporal_d64_mxfp8(x.data_ptr(), q.mid.data_ptr(), s.mid.data_ptr(), B, T, pixels, heads, 3 * Dm, Dm, 2 * Dm, 0.125,
                                                ops.ATTN_CAUSAL if causal else 0, _stream()), c["id"])

    big = Guarded(rows, kp, torch.uint8), Guarded(rows, kp // 32, torch.uint8)
    call(qkv, P, *big)
    assert C.in_regime(big[0].mid.numel(), "2g")
    o16 = torch.full((rows, Dm), float("nan"), dtype=torch.float16, device=DEV)
    ops.temporal_attn(qkv, o16, B=B, T=T, P=P, heads=heads, ld=3 * Dm, k_off=Dm, v_off=2 * Dm, ldo=Dm, scale=0.125, causal=causal)
    want = D.quant_rows(o16)
    del o16
    assert len(torch.unique(want[1][:4096, :2 * heads])) > 3, "the data should spread over several scale bytes"
    _check_pair(big, want, c["id"])                                                                               # (c), (d)
    del want
    for lo, hi in C.attn_slices(c):                                                                              # (b)
        n = hi - lo
        part = Guarded(T * n, kp, torch.uint8), Guarded(T * n, kp // 32, torch.uint8)
        call(qkv.view(T, P, 3 * Dm)[:, lo:hi].contiguous(), n, *part)
        _check_pair(part, tuple(o.mid.view(T, P, -1)[:, lo:hi].reshape(T * n, -1) for o in big), f"{c['id']}: pixels {lo} .. {hi} called alone")
        del part


@pytest.mark.parametrize("c", [c for c in C.ATTN_CASES if c["form"] in ("flash", "dual")], ids=lambda c: c["id"])
def test_flash_attention_quantiser(c):
    """vcx_attn_flash_d64_mxfp8 - one case per kernel the entry dispatches to - and vcx_attn_flash_dual_d64_mxfp8 at 4100 groups x 4096
    queries, one head (output 2 149 580 800 bytes, the odd-head padding stores): (c) against quant_rows of the fp16 entry with the same
    arguments and knobs, (b) halves of the groups called alone."""
    from viewcrafter_amd import _lib, ops
    L = _lib.lib()
    G, heads, nq = c["n_groups"], c["heads"], c["nq"]
    Dm, rows = 64 * heads, G * nq
    kp = MX.kp_of(Dm)
    need((rows * Dm * 2 * 2 + rows * kp * 3.5) / GIB + 2)
    dual = c["form"] == "dual"
    q = _t((rows, Dm), 331)
    if dual:
        sets = G // c["kv_div"]
        keys = [(c["kv_rows1"], 332), (c["nk2"], 334)]
    else:
        sets = G
        keys = [(c["nk"], 332)]
    kv = []
    for per, seed in keys:
        kv += [_t((sets * per, Dm), seed), _loud_rows(_t((Dm, sets * per), seed + 1), seed + 100, 1)]

    def operands(lo, hi):
        """q, then (K, V^T) per key set, of the groups lo .. hi"""
        div = c["kv_div"] if dual else 1
        out = [q[lo * nq:hi * nq]]
        for (per, _), k, vt in zip(keys, kv[0::2], kv[1::2]):
            s = slice(lo // div * per, hi // div * per)
            out += [k[s], vt[:, s].contiguous()]
        return out

    def call(lo, hi, oq, os_):
        geo, t = C.attn_geo(c, hi - lo), operands(lo, hi)
        assert (ops.flash_attn_dual_mxfp8_ok if dual else ops.flash_attn_mxfp8_ok)(**geo), L.vcx_last_error()
        p = [x.data_ptr() for x in t] + [oq.mid.data_ptr(), os_.mid.data_ptr()]
        if dual:
            ops.check(L.vcx_attn_flash_dual_d64_mxfp8(*p, geo["n_groups"], heads, nq, geo["nk1"], geo["kv_rows1"], geo["kv_div1"], geo["ldk1"], geo["ldvt1"], geo["nk2"],
                                                      geo["kv_rows2"], geo["kv_div2"], geo["ldk2"], geo["ldvt2"], geo["ldq"], 1.0, ops.ATTN_LOG2_LOGITS, _stream()), c["id"])
        else:
            ops.check(L.vcx_attn_flash_d64_mxfp8(*p, geo["n_groups"], heads, nq, geo["nk"], geo["kv_rows"], geo["kv_div"], geo["ldq"], geo["ldk"], geo["ldvt"], 1.0,
                                                 ops.ATTN_LOG2_LOGITS, _stream()), c["id"])

    with _knobs(**c.get("knobs", {})):
        big = Guarded(rows, kp, torch.uint8), Guarded(rows, kp // 32, torch.uint8)
        call(0, G, *big)
        assert big[0].mid.numel() == 2_149_580_800
        o16 = torch.full((rows, Dm), float("nan"), dtype=torch.float16, device=DEV)
        (ops.flash_attn_dual if dual else ops.flash_attn)(*operands(0, G), o16, ldo=Dm, scale=1.0, log2_logits=True, **C.attn_geo(c))
        want = D.quant_rows(o16)
        del o16
        assert len(torch.unique(want[1][:4096, :2 * heads])) > 3, "the data should spread over several scale bytes"
        _check_pair(big, want, c["id"])                                                                           # (c), (d)
        del want
        for lo, hi in C.attn_slices(c):                                                                          # (b)
            part = Guarded((hi - lo) * nq, kp, torch.uint8), Guarded((hi - lo) * nq, kp // 32, torch.uint8)
            call(lo, hi, *part)
            _check_pair(part, tuple(o.mid[lo * nq:hi * nq] for o in big), f"{c['id']}: groups {lo} .. {hi} called alone")
            del part
        torch.cuda.synchronize()
