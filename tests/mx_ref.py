"""Test reference of the MX block-scaled quantizer (OCP Microscaling Formats v1.0), on the CPU in float64, written from the
definition and independent of the package's arithmetic:

  * ``ref_grid``  enumerates the element format's codes into its value grid and rounds by searching that grid (all five formats);
  * ``ref_cast``  clamps and lets ATen's own ``float8_e4m3fn`` / ``float8_e5m2`` casts round (the two FP8 formats).

``reference()`` insists that the two agree wherever both exist before it returns anything.  Comparisons are bit for bit
(``same``): NaNs equal each other, ``-0.0`` differs from ``+0.0``."""
import torch

# name -> (exponent bits, mantissa bits, bias, emax, largest normal)
FORMATS = {
    "mxfp8_e4m3": (4, 3, 7, 8, 448.0),
    "mxfp8_e5m2": (5, 2, 15, 15, 57344.0),
    "mxfp6_e2m3": (2, 3, 1, 2, 7.5),
    "mxfp6_e3m2": (3, 2, 3, 4, 28.0),
    "mxfp4_e2m1": (2, 1, 1, 2, 6.0),
}
WIDTH = {f: 1 + v[0] + v[1] for f, v in FORMATS.items()}
FP8 = {"mxfp8_e4m3": torch.float8_e4m3fn, "mxfp8_e5m2": torch.float8_e5m2}
BLOCK = 32
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit-for-bit equality with all NaNs alike (and -0.0 != +0.0)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu(), b.detach().cpu()
    if not a.is_floating_point():
        return torch.equal(a, b)
    a, b = a.double(), b.double()
    nan = a.isnan() & b.isnan()
    return bool((nan | ((a == b) & (torch.signbit(a) == torch.signbit(b)))).all())


def grid(fmt):
    """(values, codes): the non-negative values of the format up to its largest normal, ascending, and the code of each"""
    eb, mb, bias, emax, top = FORMATS[fmt]
    seen = {}
    for code in range(1 << (eb + mb)):
        E, M = code >> mb, code & ((1 << mb) - 1)
        val = M / (1 << mb) * 2.0 ** (1 - bias) if E == 0 else (1 + M / (1 << mb)) * 2.0 ** (E - bias)
        if val <= top:                 # (beyond it lie e5m2's Inf / NaN exponent and e4m3's NaN mantissa)
            seen.setdefault(val, code)
    vals = sorted(seen)
    return torch.tensor(vals, dtype=torch.float64), torch.tensor([seen[v] for v in vals], dtype=torch.int64)


def _floor_log2_f32(a32: torch.Tensor) -> torch.Tensor:
    """unbiased binary exponent of positive float32 values from their bit pattern, subnormals included"""
    bits = a32.contiguous().view(torch.int32).to(torch.int64)
    field, frac = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    length = (frac.unsqueeze(-1) >= (1 << torch.arange(23, dtype=torch.int64))).sum(-1)       # bit length of the fraction
    return torch.where(field > 0, field - 127, length - 1 - 149)


def _blocks(x, dim):
    v = x.detach().cpu().movedim(dim, -1).float()
    n = v.shape[-1]
    nb = -(-n // BLOCK)
    pad = torch.zeros(v.shape[:-1] + (nb * BLOCK - n,))
    return torch.cat([v, pad], -1).reshape(v.shape[:-1] + (nb, BLOCK)), n


def _scale(blk, fmt):
    emax = FORMATS[fmt][3]
    amax = blk.abs().amax(-1, keepdim=True)
    bad = amax.isnan() | amax.isinf()
    zero = amax == 0
    fl = _floor_log2_f32(torch.where(bad | zero, torch.ones_like(amax), amax))
    e = torch.where(zero, torch.full_like(fl, -127), (fl - emax).clamp(-127, 127))
    return e, bad


def _finish(y, code, e, bad, n, dim, out_dtype):
    y = torch.where(bad, torch.full_like(y, float("nan")), y)
    code = torch.where(bad, torch.zeros_like(code), code)
    scale = torch.where(bad, torch.full_like(e, 255), e + 127).squeeze(-1)
    unblock = lambda t: t.reshape(t.shape[:-2] + (-1,))[..., :n].movedim(-1, dim).contiguous()
    return unblock(y).to(out_dtype), unblock(code).to(torch.uint8), scale.movedim(-1, dim).contiguous().to(torch.uint8)


def ref_grid(x, fmt, dim=-1, out_dtype=torch.float32):
    eb, mb, bias, emax, top = FORMATS[fmt]
    g, gcode = grid(fmt)
    blk, n = _blocks(x, dim)
    e, bad = _scale(blk, fmt)
    X = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())
    v = torch.where(bad, torch.zeros_like(blk), blk).double() / X
    a = v.abs().clamp(max=top)
    hi = torch.bucketize(a, g).clamp(max=len(g) - 1)
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = a - g[lo], g[hi] - a
    pick = torch.where(dlo < dhi, lo, torch.where(dhi < dlo, hi, torch.where(lo % 2 == 0, lo, hi)))     # tie: the even mantissa
    q = torch.copysign(g[pick], v)
    code = gcode[pick] + (torch.signbit(v).to(torch.int64) << (eb + mb))
    return _finish(q * X, code, e, bad, n, dim, out_dtype)


def ref_cast(x, fmt, dim=-1, out_dtype=torch.float32):
    top = FORMATS[fmt][4]
    blk, n = _blocks(x, dim)
    e, bad = _scale(blk, fmt)
    X = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())
    v = torch.where(bad, torch.zeros_like(blk), blk).double() / X
    q8 = v.clamp(-top, top).float().to(FP8[fmt])
    code = q8.view(torch.uint8).to(torch.int64)
    return _finish(q8.double() * X, code, e, bad, n, dim, out_dtype)


def reference(x, fmt, dim=-1, out_dtype=torch.float32):
    """(y, codes, scales) by the grid definition, checked against the cast definition for the FP8 formats first"""
    out = ref_grid(x, fmt, dim, out_dtype)
    if fmt in FP8:
        other = ref_cast(x, fmt, dim, out_dtype)
        assert all(same(a, b) for a, b in zip(out, other)), f"the two reference definitions disagree for {fmt}"
    return out


def expand_scale(scales, n, dim):
    """X = 2^(scale - 127) per element (float64; NaN for 0xFF), the block axis expanded back to n"""
    s = scales.cpu().to(torch.int64)
    X = torch.where(s == 255, torch.full((), float("nan"), dtype=torch.float64), torch.pow(torch.tensor(2.0, dtype=torch.float64), (s - 127).double()))
    return X.repeat_interleave(BLOCK, dim=dim).narrow(dim, 0, n)


def all_patterns(dtype):
    """every 16-bit pattern of a 2-byte float dtype, ascending"""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


def permuted_finite_patterns(dtype):
    """the same patterns in a fixed permutation, the non-finite ones replaced by 0: every block is finite"""
    p = all_patterns(dtype)[torch.randperm(65536, generator=torch.Generator().manual_seed(1))]
    return torch.where(torch.isfinite(p.float()), p, torch.zeros_like(p))


def midpoints(fmt):
    """every midpoint between neighbouring grid values (exact in float32)"""
    g, _ = grid(fmt)
    return ((g[:-1] + g[1:]) / 2).float()
