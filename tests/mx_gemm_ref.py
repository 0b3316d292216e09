"""Test reference of the matrix product on MX codes, on the CPU in float64, written from the definition and independent of the
package's arithmetic: the value of every code comes from enumerating the element format's grid here (as tests/mx_ref.py does),
not from ``mx_dequantize``.

    y[m, n] = sum_k val_a(a[m, k]) 2^(sa[m, k / 32] - 127) val_b(b[n, k]) 2^(sb[n, k / 32] - 127) + bias[n]

``reference`` returns the float64 sum, its rounding to the output dtype and ``S = sum_k |a_k b_k|`` (the scale of the error
bounds).  ``exact_operand`` draws the EXACT CLASS: codes whose values are multiples of q with magnitude at most R q and scale
bytes within a window of r consecutive values, for which -- when K R_a R_b 2^(r_a + r_b) <= 2^24 -- every partial sum of the
products, in any order, is an integer multiple of one quantum below 2^24 of them: exact in float32, so any summation order
gives the same bits."""
import math

import torch

from mx_ref import BLOCK, FORMATS, WIDTH

FMTS = list(FORMATS)
MANT = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}
EMIN = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}
# format -> (q, R): the drawn subset holds the codes whose value is a multiple of q with |value| <= R q
EXACT = {"mxfp8_e4m3": (1.0, 16), "mxfp8_e5m2": (1.0, 16), "mxfp6_e2m3": (0.125, 60), "mxfp6_e3m2": (0.25, 16), "mxfp4_e2m1": (0.5, 12)}


def table(fmt):
    """float64 value of every byte 0..255 read as a code of `fmt` (bits above the format's width ignored; codes past the largest
    normal -- which the quantizer never writes -- NaN)"""
    eb, mb, bias, emax, top = FORMATS[fmt]
    out = []
    for byte in range(256):
        code = byte & ((1 << WIDTH[fmt]) - 1)
        sign, E, M = code >> (eb + mb), (code >> mb) & ((1 << eb) - 1), code & ((1 << mb) - 1)
        val = M / (1 << mb) * 2.0 ** (1 - bias) if E == 0 else (1 + M / (1 << mb)) * 2.0 ** (E - bias)
        out.append(float("nan") if val > top else (-val if sign else val))
    return torch.tensor(out, dtype=torch.float64)


def values(codes, scales, fmt):
    """float64 values [..., K]; NaN throughout a block whose scale byte is 0xFF"""
    K = codes.shape[-1]
    s = scales.cpu().to(torch.int64)
    X = torch.where(s == 255, torch.full((), float("nan"), dtype=torch.float64), torch.pow(torch.tensor(2.0, dtype=torch.float64), (s - 127).double()))
    return table(fmt)[codes.cpu().to(torch.int64)] * X.repeat_interleave(BLOCK, dim=-1)[..., :K]


def reference(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, bias=None, out_dtype=torch.float32):
    """(y rounded to out_dtype, y in float64, S): NaN exactly where the dot product reads a 0xFF block"""
    a, b = values(a_codes, a_scales, a_fmt), values(b_codes, b_scales, b_fmt)
    bad = a.isnan().any(-1).unsqueeze(-1) | b.isnan().any(-1)                 # [..., N]
    a0, b0 = torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)
    y = a0 @ b0.t()
    S = a0.abs() @ b0.abs().t()
    if bias is not None:
        y = y + bias.cpu().double()
    y = torch.where(bad, torch.full((), float("nan"), dtype=torch.float64), y)
    return y.to(out_dtype), y, S


def ulp(y64, dtype):
    """spacing of `dtype` at |y| (float64 tensor)"""
    e = torch.frexp(torch.where(y64 == 0, torch.ones_like(y64), y64.abs()))[1] - 1
    e = torch.where(y64 == 0, torch.full_like(e, EMIN[dtype]), e).clamp(min=EMIN[dtype])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - (MANT[dtype] - 1)).double())


def same(a, b):
    """bit-for-bit equality with all NaNs alike"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return bool(((a.isnan() & b.isnan()) | ((a == b) & (torch.signbit(a) == torch.signbit(b)))).all())


def within(y, y64, bound):
    """|y - y64| <= bound elementwise, NaN where and only where y64 is NaN; returns (ok, largest |err| / bound)"""
    y = y.detach().cpu().double()
    nan = y64.isnan()
    if not torch.equal(y.isnan(), nan):
        return False, float("inf")
    err = torch.where(nan, torch.zeros_like(y64), (y - y64).abs())
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return bool((err <= bound).all()), float(ratio.max()) if ratio.numel() else 0.0


def exact_subset(fmt):
    q, R = EXACT[fmt]
    t = table(fmt)[: 1 << WIDTH[fmt]]
    ok = (~t.isnan()) & (t.abs() <= R * q) & ((t / q) == (t / q).round())
    return ok.nonzero().reshape(-1)


def scale_windows(K, fa, fb, cap=4):
    """(r_a, r_b): the widest equal scale windows (at most `cap`) with K R_a R_b 2^(r_a + r_b) <= 2^24"""
    room = 2.0 ** 24 / (K * EXACT[fa][1] * EXACT[fb][1])
    r = min(cap, int(math.floor(math.log2(room) / 2))) if room >= 1 else 0
    return r, r


def assert_exact_class(K, fa, fb, ra, rb):
    assert ra >= 1 and rb >= 1 and K * EXACT[fa][1] * EXACT[fb][1] * 2 ** (ra + rb) <= 2 ** 24, (K, fa, fb, ra, rb)


def exact_operand(g, rows, K, fmt, r, base=None):
    """codes [rows, K] from the exact subset and scale bytes [rows, ceil(K / 32)] within [base, base + r)"""
    sub = exact_subset(fmt)
    codes = sub[torch.randint(0, len(sub), (rows, K), generator=g)].to(torch.uint8)
    base = int(torch.randint(100, 150, (1,), generator=g)) if base is None else base
    scales = (base + torch.randint(0, r, (rows, -(-K // BLOCK)), generator=g)).to(torch.uint8)
    return codes, scales


# ---- one-term products: every valid code of a format crossed with scale bytes over the whole E8M0 range ---------------------------
ONE_TERM_SCALES = (0, 1, 64, 126, 127, 128, 190, 253, 254)


def valid_codes(fmt):
    """every code of `fmt` that has a value (E4M3 254, E5M2 248, FP6 64, FP4 16): the special patterns are left out"""
    return (~table(fmt)[: 1 << WIDTH[fmt]].isnan()).nonzero().reshape(-1)


def one_term_operand(g, fmt, K, k0):
    """(codes [rows, K], scales [rows, ceil(K / 32)], value [rows] in float64): row r holds ONE code that may be nonzero, at column
    k0, and runs over every valid code of `fmt` crossed with ONE_TERM_SCALES at the block of k0.  Every other code is the zero code
    and every other block carries a random scale byte 0..254, which must not matter."""
    codes = valid_codes(fmt)
    c = codes.repeat_interleave(len(ONE_TERM_SCALES))
    s = torch.tensor(ONE_TERM_SCALES).repeat(len(codes))
    rows = len(c)
    cm = torch.zeros(rows, K, dtype=torch.uint8)
    cm[:, k0] = c.to(torch.uint8)
    sm = torch.randint(0, 255, (rows, -(-K // BLOCK)), generator=g).to(torch.uint8)
    sm[:, k0 // BLOCK] = s.to(torch.uint8)
    return cm, sm, table(fmt)[c] * torch.pow(torch.tensor(2.0, dtype=torch.float64), (s - 127).double())


class OneTerm:
    """the outputs of the one-term product of two operands of one_term_operand (row values va, vb), worked out once per format pair:
    they depend on neither K, k0 nor the kernel.
    p: the product in float64, exact (at most 8 significant bits, exponents within +-300).
    strict: the exact value is zero or has a magnitude in [2^-126, 2^128), where float32 holds it; under: 0 < magnitude < 2^-126;
    over: magnitude >= 2^128."""

    def __init__(self, va, vb):
        self.p = va.reshape(-1, 1) * vb.reshape(1, -1)
        mag = self.p.abs()
        self.under, self.over = (mag > 0) & (mag < 2.0 ** -126), mag >= 2.0 ** 128
        self.strict = ~(self.under | self.over)
        self.y64 = self.p + 0.0            # the sum over K of the definition: every other term is +0, so a -0 product sums to +0
        self.p32 = self.p.float() + 0.0

    def expected(self, bias, dt):
        """(strict_want, measured_want).  `bias` holds zeros of either sign only, so the classes are those of the product.
        `strict_want` is the float64 value of the definition cast once to float32 and from there to `dt` -- binding on the strict
        class.  `measured_want` states every output, as the MI355X was measured to give them for all 25 format pairs alike
        (include/qsparse_hip.h, "MX matrix product"): the product rounded to float32 to nearest-even with GRADUAL underflow
        (subnormal results are kept), Inf of the product's sign from 2^128 on, and a product that rounds to zero in float32 sums
        to +0 whatever its sign, as an exact zero does -- the accumulator starts at +0 and the other terms are +0; then the bias,
        in float32 (+0 + -0 = +0); then one IEEE cast to `dt`, which keeps the sign (a small negative sum is -0 in fp16 / bf16)."""
        assert bias is None or bool((bias == 0).all())
        strict_want = (self.y64 if bias is None else self.y64 + bias.double()).float().to(dt)
        measured = (self.p32 if bias is None else self.p32 + bias.float()).to(dt)
        assert bool(bits_equal(strict_want, measured)[self.strict].all())    # the measured behaviour is one reading of the definition
        return strict_want, measured


def bits_equal(a, b):
    """elementwise bit-for-bit equality of two tensors of one floating dtype (all NaNs alike), on their device"""
    assert a.dtype == b.dtype and a.shape == b.shape
    return (a.isnan() & b.isnan()) | ((a == b) & (torch.signbit(a) == torch.signbit(b)))
