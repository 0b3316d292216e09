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


# ---- the bound that follows the instruction's measured accumulation ("Accumulation"; profiles/mx_mfma_scale_probe.txt) ------
GROUP = 8             # probe 4c: the k of one group are eight consecutive ones, 8 j .. 8 j + 7, for every pair that can tell
KEPT = 13             # probe 4b / 4d: inside a group a bit survives down to 2^-13 of the group's reference, and is cut below
STEP = 128            # one instruction; the kernels walk K in these steps, a split-K slice starts a new walk
F_ACROSS = 18         # quanta of 2^-23 S lost per step outside the groups: the figure the bound was set with BEFORE the probe's 4e / 4f
#                       (one alignment of 16 group sums, C and a normalisation).  The measured structure accounts for 16 of them
#                       (model_bound's docstring); the two spare ones are attributed to nothing and are kept only because a bound is
#                       not re-tuned, in either direction, after the kernels were seen against it


def operand_exponents(codes, scales, fmt):
    """float64 [..., K]: the exponent the instruction reads off each operand, scale included: the exponent FIELD's, which for a
    subnormal is the format's smallest and not floor(log2 |value|) (probe 4f: next to E4M3's 2^-9 a term survives to 2^-19, not
    2^-22).  A zero code does not count (4f: next to 0 x 256 every term is kept): -10^4 here"""
    eb, mb, bias, _, _ = FORMATS[fmt]
    c = torch.arange(256) & ((1 << WIDTH[fmt]) - 1)
    field = ((c >> mb) & ((1 << eb) - 1)).clamp(min=1) - bias
    K = codes.shape[-1]
    s = scales.cpu().to(torch.int64).repeat_interleave(BLOCK, dim=-1)[..., :K]
    c = codes.cpu().to(torch.int64)
    return torch.where(table(fmt)[c] == 0, torch.full((), -1e4, dtype=torch.float64), (field[c] + s - 127).double())


def _products(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt):
    """(p [M, N, G, 8] exact products, q [M, N, G] the quantum of each group of eight): K padded to whole groups with the zero code
    under its block's scale byte, as the kernels pad a short block.  q = 2^(max over the group of (e_a + e_b) - 13): probe 4d -- the
    reference is the SUM OF THE TWO OPERANDS' EXPONENTS, not the product's (1.75 x 1.75 = 3.0625 keeps what 1.0 x 1.0 keeps)"""
    va, vb = torch.nan_to_num(values(a_codes, a_scales, a_fmt), nan=0.0), torch.nan_to_num(values(b_codes, b_scales, b_fmt), nan=0.0)
    out = []
    for codes, scales, fmt, v in ((a_codes, a_scales, a_fmt, va), (b_codes, b_scales, b_fmt, vb)):
        K = codes.shape[-1]
        pad = -K % GROUP
        zero = torch.zeros(codes.shape[0], pad, dtype=torch.uint8)
        e = operand_exponents(torch.cat([codes.cpu(), zero], -1), torch.where(scales.cpu() == 255, 127, scales.cpu()), fmt)
        out.append((torch.cat([v, zero.double()], -1), e))
    (va, ea), (vb, eb) = out
    M, N, Kp = va.shape[0], vb.shape[0], va.shape[1]
    p = (va[:, None, :] * vb[None, :, :]).reshape(M, N, Kp // GROUP, GROUP)
    top = (ea[:, None, :] + eb[None, :, :]).reshape(M, N, Kp // GROUP, GROUP).amax(-1)
    q = torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.where(top < -5e3, torch.zeros_like(top), top - KEPT))     # (a group of zeros: any q)
    return p, q


def inside_groups(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt):
    """[M, N]: sum over the groups g of sum_{k in g} [p_k is no multiple of q_g] q_g -- what the cut inside the groups can cost.  A
    term that is a multiple of its quantum loses nothing, whichever way the cut goes (the probe: toward zero)"""
    p, q = _products(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt)
    r = p / q[..., None]                                                      # exact: a power of two
    return ((r != r.round()) * q[..., None]).sum((-1, -2))


def model_bound(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, y64, S, bias=None, out_dtype=torch.float32, slices=1, inside=None):
    """[M, N] bound on |y - y64| for a kernel that walks K in steps of 128 through v_mfma_scale_f32_16x16x128_f8f6f4, from the codes and
    scale bytes alone (M N K of a call: 10^7 or less, the products are materialised):

        inside_groups                       the cut inside every group of eight, term by term
      + F_ACROSS steps 2^-23 S              across the groups and C, steps = ceil(K / 128) (per split-K slice: the sum over slices)
      + (slices - 1) 2^-23 S                split-K: one float32 rounding of the running sum per added partial
      + ulp_ydt(y64) + 2^-23 |bias|         the bias added in float32, one rounding to the output dtype

    F_ACROSS = 18, from probe 4, 4b and 4e: a step adds its four blocks of 32 to the accumulator one after the other (`C = -2^30,
    products 2^30 + 1` gives 1; `C = 2^24` plus one product 1 in each of four blocks gives 2^24, plus four in one block 2^24 + 4).  In a
    block the four group sums are aligned to the largest of them, which loses nothing, the other three each less than one quantum
    2^-23 of it (4b: kept at 2^-23, gone at 2^-24): 12 a step.  Each of the four additions cuts the smaller operand below one guard
    bit, less than half a quantum of the larger, and rounds the sum to nearest even, at most half a quantum of it (`2^24 + 3 -> 2^24
    + 4`, `2^25 + 3 -> 2^25`, `2^24 - 1` exact): 4 a step.  The block sum itself is carried wide (4f: `C = -2^24` plus a block
    of `2^24 + 3` gives 3).  That is 16; F_ACROSS stays at the 18 it was set to beforehand (see there).  Every quantum is 2^-23 of a partial sum's binade, at most 2^-23 S.  `inside`: inside_groups of the same operands,
    where a caller has it already (it depends on neither the bias nor the output dtype).

    The one rounding to the output dtype costs the bound a whole ulp, which cannot tell a wrong rounding rule from the right one.  That
    rounding is asserted bit for bit, apart from this bound, by tests/test_mx_epilogue_rounding_gpu.py on the operands of `method_a` /
    `method_b` below, whose float32 value before the cast is exact (tests/test_mx_epilogue_rounding.py: the same on the CPU paths)."""
    K = a_codes.shape[-1]
    steps = -(-K // STEP)                                                 # (split-K slices are whole steps: the same count)
    inside = inside_groups(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt) if inside is None else inside
    bound = inside + (F_ACROSS * steps + (slices - 1)) * 2.0 ** -23 * S
    y = torch.nan_to_num(y64, nan=0.0)
    bound = bound + ulp(y, out_dtype)
    return bound if bias is None else bound + 2.0 ** -23 * bias.cpu().double().abs()


def _round24(x):
    """x (float64) to 24 significant bits, nearest even"""
    m, e = torch.frexp(x)
    return torch.ldexp((m * 2.0 ** 24).round(), e - 24)


def _cut(x, quantum):
    return torch.trunc(x / quantum) * quantum


def model_emulate(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, bias=None, out_dtype=torch.float32):
    """float64 emulation of the measured model, a CPU sanity tool and no bit-exact oracle of the GPU: every product cut toward zero to
    its group's quantum; per block of 32 the four group sums cut to 2^-23 of the largest of them; the block sum added to the
    accumulator with the smaller of the two cut below one guard bit (2^-24 of the larger) and the sum rounded to 24 bits, nearest
    even; then the bias in float32 and one cast"""
    p, q = _products(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt)
    groups = _cut(p, q[..., None]).sum(-1)                                # [M, N, G]: exact, at most 8 x 2^14 quanta
    pad = -groups.shape[-1] % (BLOCK // GROUP)
    groups = torch.cat([groups, torch.zeros(groups.shape[:2] + (pad,), dtype=torch.float64)], -1)
    two = torch.tensor(2.0, dtype=torch.float64)

    def binade(x):
        return torch.pow(two, (torch.frexp(torch.where(x == 0, torch.ones_like(x), x))[1] - 1).double())

    acc = torch.zeros(groups.shape[:2], dtype=torch.float64)
    for b in range(groups.shape[-1] // 4):
        g4 = groups[..., 4 * b: 4 * b + 4]
        top = g4.abs().amax(-1)
        block = _cut(g4, (binade(top) * 2.0 ** -23)[..., None]).sum(-1)
        big = torch.maximum(acc.abs(), block.abs())
        guard = binade(big) * 2.0 ** -24
        acc = torch.where(big == 0, acc, _round24(_cut(acc, guard) + _cut(block, guard)))
    y = acc.float()
    if bias is not None:
        y = y + bias.cpu().float()
    return y.to(out_dtype).double()


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


# ---- the output rounding, bit for bit: products whose float32 value before the cast is known exactly and has a full mantissa ------------
# (tests/test_mx_epilogue_rounding.py and its GPU twin).  Everything below works on bit patterns held as Python ints or int64
# tensors; a float tensor is built from them only to be handed to the code under test.
TWO_BYTE = (torch.bfloat16, torch.float16)
# unbiased exponents of the binades the targets are drawn from: the lowest normal one of the dtype, two next to 1, one far on either
# side, the top one
BINADES = {torch.bfloat16: (-126, -60, -1, 0, 60, 127), torch.float16: (-14, -8, -1, 0, 9, 15)}


def f32_from_bits(bits):
    """float32 tensor of the given bit patterns (ints 0 .. 2^32 - 1)"""
    u = torch.as_tensor(bits, dtype=torch.int64).reshape(-1)
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)


def f32_bits(t):
    """int64 tensor of the bit patterns of a float32 tensor"""
    assert t.dtype == torch.float32
    return t.detach().cpu().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def two_byte_from_bits(bits, dtype):
    """bfloat16 / float16 tensor of the given 16-bit patterns (int64 tensor)"""
    u = torch.as_tensor(bits, dtype=torch.int64)
    return torch.where(u >= 2 ** 15, u - 2 ** 16, u).to(torch.int16).view(dtype)


def rounding_targets(dtype):
    """float32 tensor [T] of the values the output cast to `dtype` (bfloat16 or float16) is asserted on, every one a float32 normal
    (2^-126 <= |t| < 2^128), none repeated.  BINADES[dtype] crossed with four patterns of the kept mantissa bits (all clear: kept lsb
    even; the lsb alone: odd; an alternating one, even; all set, odd -- its round-up carries into the next binade, from the top binade to
    Inf), the six discarded parts 0, one float32 ulp, half - ulp, half, half + ulp, all ones, and both signs; then the overflow edge
    and, for float16, the underflow edge with its ties on either side of the subnormals.  bfloat16's subnormals are float32's and are
    left to the one-term test."""
    keep = MANT[dtype] - 1                     # mantissa bits the dtype stores: 7, 10
    drop = 23 - keep                           # discarded ones: 16, 13
    half = 1 << (drop - 1)
    alternating = int("10" * 5, 2) >> (10 - keep) << 1 & ((1 << keep) - 1)         # ...1010100 / ...10101010100: lsb clear
    out = []
    for e in BINADES[dtype]:
        for hi in (0, 1, alternating, (1 << keep) - 1):
            for d in (0, 1, half - 1, half, half + 1, 2 * half - 1):
                out.append((e + 127) << 23 | hi << drop | d)
    if dtype == torch.float16:
        top = (15 + 127) << 23 | 0x3FF << 13                                   # 65504
        out += [top, top + half - 1, top + half, (16 + 127) << 23]             # 65504, just below 65520, 65520 (tie -> Inf), 2^16
        ex = lambda e: (e + 127) << 23
        out += [ex(-14),                       # the smallest normal
                ex(-15) | 0x3FF << 13,         # 2^-14 - 2^-25: the tie between the largest subnormal and 2^-14 (-> 2^-14, even)
                ex(-24),                       # the smallest subnormal
                ex(-24) | 1 << 22,             # 1.5 2^-24: a tie -> 2^-23
                ex(-25),                       # a tie -> 0
                ex(-25) | 1,                   # -> 2^-24
                ex(-26)]                       # -> 0
    else:
        top = 0x7F7F0000                                                       # the largest finite bfloat16
        out += [top, top + 0x7FFF, top + 0x8000, 0x7F7FFFFF]                   # finite, finite, a tie -> Inf, FLT_MAX
    seen, bits = set(), []
    for b in out:
        if b not in seen:
            seen.add(b)
            bits += [b, b | 1 << 31]
    t = f32_from_bits(bits)
    assert bool(((t.abs().double() >= 2.0 ** -126) & (t.abs().double() < 2.0 ** 128)).all())
    return t


def round_once_bits(t, dtype):
    """int64 tensor: the bit patterns of float32 `t` rounded once, to nearest with ties to even, to bfloat16 or float16.  Integer
    arithmetic on the float32 bit pattern, from the definition: |t| = sig 2^E; the result is the multiple of the quantum 2^q, q =
    max(floor(log2 |t|), emin) - (P - 1), nearest to it -- then encoded (zero, subnormal, normal, Inf past the largest finite).
    Every NaN becomes the quiet NaN 0x7FC0 / 0x7E00."""
    P, emin = MANT[dtype], EMIN[dtype]
    emax, ebits = (127, 8) if dtype == torch.bfloat16 else (15, 5)
    u = f32_bits(t)
    sign, exp, man = u >> 31, (u >> 23) & 0xFF, u & 0x7FFFFF
    sig = torch.where(exp > 0, man | 1 << 23, man)
    E = exp.clamp(min=1) - 127 - 23
    length = torch.zeros_like(sig)
    for i in range(24):
        length += ((sig >> i) > 0).to(torch.int64)                            # bit length of sig
    q = torch.maximum(E + length - 1, torch.full_like(E, emin)) - (P - 1)
    shift = (q - E).clamp(max=40)              # >= 13 for either dtype; past 25 nothing of sig is left of the half
    kept, rem, tie = sig >> shift, sig & ((1 << shift) - 1), 1 << (shift - 1)
    kept = kept + ((rem > tie) | ((rem == tie) & (kept & 1 == 1))).to(torch.int64)
    carry = kept >= 1 << P                     # rounded up to 2^P: one more binade
    kept, q = torch.where(carry, kept >> 1, kept), q + carry.to(torch.int64)
    normal = kept >= 1 << (P - 1)
    field = torch.where(normal, q + (P - 1) + emax, torch.zeros_like(q))       # the biased exponent; 0: zero or subnormal
    inf = (1 << ebits) - 1
    mag = torch.where(field >= inf, torch.full_like(q, inf << (P - 1)), field << (P - 1) | (kept & ((1 << (P - 1)) - 1)))
    mag = torch.where(exp == 255, torch.where(man > 0, torch.full_like(q, inf << (P - 1) | 1 << (P - 2)), torch.full_like(q, inf << (P - 1))), mag)
    return torch.where((exp == 255) & (man > 0), mag, sign << 15 | mag)


def cast_bits(t, dtype):
    """the same through torch's own cast: the second definition"""
    return t.detach().cpu().to(dtype).view(torch.int16).to(torch.int64) & 0xFFFF


def expected_rounded(t, dtype):
    """what an output whose float32 value before the cast is `t` must be, in `dtype`: `t` itself, or round_once_bits' value"""
    return t.clone() if dtype == torch.float32 else two_byte_from_bits(round_once_bits(t, dtype), dtype).reshape(t.shape)


def strict_class(want32):
    """the outputs that are compared bit for bit: those whose exact value before the cast is a float32 -- finite, which a float32
    tensor of exact values is by construction.  The share is asserted to be 1.0 wherever it is used"""
    return want32.isfinite() & (want32.double().float() == want32)


def one_codes(fmt):
    """(the code of +1.0, the code of -1.0) of `fmt`: every format has both"""
    t = table(fmt)[: 1 << WIDTH[fmt]]
    return int((t == 1.0).nonzero()[0]), int((t == -1.0).nonzero()[0])


def _power(sign, e):
    """float32 bits of (-1)^sign 2^e, -126 <= e <= 127"""
    assert -126 <= e <= 127
    return sign << 31 | (e + 127) << 23


def _as_int(terms, floor):
    return sum((-1 if s else 1) << (e - floor) for s, e in terms)


def representable24(x):
    """the integer x (times any power of two) has at most 24 significant bits"""
    x = abs(x)
    return x == 0 or x.bit_length() - ((x & -x).bit_length() - 1) <= 24


def subsets_exact(terms):
    """every subset of the signed powers of two `terms` [(sign, e)] sums to something 24 bits hold: then every float32 addition of
    them, in any order and any grouping, is exact"""
    floor = min(e for _, e in terms)
    return all(representable24(_as_int([terms[i] for i in range(len(terms)) if mask >> i & 1], floor)) for mask in range(1 << len(terms)))


def power_terms(bits):
    """the float32 normal with the bit pattern `bits` as at most four signed powers of two [(sign, e)] of distinct exponents -126 ..
    127, every subset of which 24 bits hold -- or None where there is no such form (more than four, or it needs 2^128).  Its set
    bits where they are at most four; else the non-adjacent form (a run of ones 2^a + ... + 2^b as 2^(a + 1) - 2^b: `half - ulp`
    becomes + half - ulp), which is the shortest signed form."""
    sign, e = bits >> 31, ((bits >> 23) & 0xFF) - 127
    sig = (bits & 0x7FFFFF) | 1 << 23
    binary = [(sign, e - 23 + i) for i in range(24) if sig >> i & 1]
    naf, x, i = [], sig, 0
    while x:
        if x & 1:
            digit = 2 - (x & 3)                # +1 or -1
            naf.append((sign if digit > 0 else sign ^ 1, e - 23 + i))
            x -= digit
        x >>= 1
        i += 1
    for terms in (binary, naf):
        if len(terms) <= 4 and all(-126 <= te <= 127 for _, te in terms) and subsets_exact(terms):
            return terms[::-1]                 # leading term first
    return None


def tile_targets(targets, N, shift=0):
    """[N]: the targets repeated cyclically from index `shift` on, so that every one meets every position of the store"""
    return targets[(torch.arange(N) + shift) % len(targets)]


def _sprinkle(g, rows, K):
    """zero codes [rows, K] under random scale bytes 0 .. 254, which must not matter"""
    return torch.zeros(rows, K, dtype=torch.uint8), torch.randint(0, 255, (rows, -(-K // BLOCK)), generator=g).to(torch.uint8)


def method_a(g, fa, fb, M, K, k0, t, zero_rows=()):
    """METHOD A, one term plus a bias: (a_codes [M, K], a_scales, b_codes [N, K], b_scales, bias [N], want [M, N] float32).  Column n
    of B holds one +-1.0 code at k0 under the scale byte that makes p_n = sign(t_n) 2^floor(log2 |t_n|) -- the byte is t_n's own
    exponent field -- every row of A 1.0 at k0 under scale byte 127, and bias[n] = t_n - p_n: exact in float32 since the two share a
    binade, so fl32(p_n + bias[n]) = t_n with no rounding (both asserted in float64 here).  A bias that comes out as zero is -0 in
    every other such column.  The rows `zero_rows` of A hold zero codes only: their output is fl32(+0 + bias[n]), in which -0 becomes
    +0.  Blocks of zero codes carry random scale bytes."""
    N, bits = len(t), f32_bits(t)
    one_a, (one_b, minus_b) = one_codes(fa)[0], one_codes(fb)
    ac, asc = _sprinkle(g, M, K)
    bc, bsc = _sprinkle(g, N, K)
    ac[:, k0], asc[:, k0 // BLOCK] = one_a, 127
    for r in zero_rows:
        ac[r, k0] = 0
    bc[:, k0] = torch.where(bits >> 31 == 1, minus_b, one_b).to(torch.uint8)
    bsc[:, k0 // BLOCK] = ((bits >> 23) & 0xFF).to(torch.uint8)
    assert int(bsc[:, k0 // BLOCK].min()) >= 1 and int(bsc[:, k0 // BLOCK].max()) <= 254
    p = f32_from_bits(bits & 0xFF800000)
    bias = t - p
    assert torch.equal(bias.double(), t.double() - p.double()) and torch.equal(p.double() + bias.double(), t.double())
    zero = (bias == 0).nonzero().reshape(-1)
    bias[zero[::2]] = -0.0
    want = t.repeat(M, 1)
    for r in zero_rows:
        want[r] = torch.zeros(N) + bias
    return ac, asc, bc, bsc, bias, want


def method_b_targets(dtype, with_bias=False):
    """the targets of `dtype` that METHOD B can state, as (t [T] float32, terms: a list of [(sign, e)] per target, bias [T] float32 or
    None).  Without a bias the terms sum to t.  With one they sum to t with its discarded bits below the half bit cleared, and bias
    = t minus that sum: the two share t's binade, so the bias is exact and fl32(sum + bias) = t without rounding; the accumulator
    then holds an exact tie (or an exact value of the dtype) and only the bias decides the rounding."""
    drop = 23 - (MANT[dtype] - 1)
    ts, terms, biases = [], [], []
    for b in f32_bits(rounding_targets(dtype)).tolist():
        acc = b & ~((1 << (drop - 1)) - 1) if with_bias else b
        found = power_terms(acc)
        if found is None:
            continue
        ts.append(b)
        terms.append(found)
        biases.append(acc)
    t = f32_from_bits(ts)
    if not with_bias:
        return t, terms, None
    acc = f32_from_bits(biases)
    bias = t - acc
    assert torch.equal(bias.double(), t.double() - acc.double()) and torch.equal(acc.double() + bias.double(), t.double())
    return t, terms, bias


def method_b(g, fa, fb, M, K, blocks, terms):
    """METHOD B, a few signed powers of two and no product bias: (a_codes [M, K], a_scales, b_codes [N, K], b_scales).  `blocks` names
    four blocks of 32 along K.  Column n of B holds its term i -- in an order shuffled per column -- as a +-1.0 code in block
    blocks[i] under the scale byte e_i + 127, every row of A 1.0 at the same four places under scale byte 127.  Everything else is
    the zero code under a random scale byte.  The sum over K is then the sum of the terms, each float32 addition of which is exact
    (subsets_exact), whatever the instruction's, the K loop's or the split's order."""
    assert len(blocks) == 4 and len(set(blocks)) == 4 and max(blocks) < -(-K // BLOCK)
    N = len(terms)
    one_a, (one_b, minus_b) = one_codes(fa)[0], one_codes(fb)
    ac, asc = _sprinkle(g, M, K)
    bc, bsc = _sprinkle(g, N, K)
    at = [blk * BLOCK + int(torch.randint(0, min(BLOCK, K - blk * BLOCK), (1,), generator=g)) for blk in blocks]
    for blk, k in zip(blocks, at):
        ac[:, k], asc[:, blk] = one_a, 127
    for n, tn in enumerate(terms):
        order = torch.randperm(4, generator=g).tolist()
        for i, (s, e) in enumerate(tn):
            bc[n, at[order[i]]], bsc[n, blocks[order[i]]] = (minus_b if s else one_b), e + 127
    return ac, asc, bc, bsc
