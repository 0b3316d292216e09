"""Test reference of the gated (GLU) MX kernels' activations, in float64, written from the mathematical definition and independent
of the package's arithmetic and of ATen's float32 ``silu`` / ``gelu``: ``act64`` / ``dact64``, the pointwise error bounds ``E_a`` /
``E_da`` of the header's float32 expressions (include/qsparse_hip.h, "MX gated products" and "MX gated backward quantizer"), the
bounds of the float outputs (``glu_bound``, ``dv_bound``), and ``codes_agree``, which compares emitted MX codes and scale bytes
with the float64 value quantized by the MX definition and exempts only what the bound cannot decide.  The input sets of
tests/test_mx_glu_f64.py and tests/test_mx_glu_f64_gpu.py are built here, once, so that both files see the same ones.

Notation.  u = 2^-24 is float32's unit roundoff: a float32 operation returns its exact result times (1 + delta), |delta| <= u, while
the result is a float32 normal.  ulp(y) is float32's spacing at |y| (``mx_gemm_ref.ulp``).  ``expf`` is taken at 1 ulp and ``erff`` at 2
ulp of the true value, the figures tests/test_mx_glu_train.py states.  eta = 2^-126, float32's smallest normal, stands for whatever
a result below it suffers, gradual underflow or a flush to zero.  Second-order terms (products of two roundoffs, the float64
reference's own 2^-53) are covered by the factor SLACK = 1 + 2^-20 on every first-order sum.  Below e = exp(-g), s = 1 / (1 + e),
c = 1 - s = e / (1 + e) (evaluated as sigmoid(-g): no cancellation in the reference), x = g sqrt(1/2).

silu, a = g / (1 + e).  expf gives e within ulp(e) <= 2 u e; the sum 1 + e adds u (1 + e): the denominator carries rho_D = u (1 + 2 c)
relative, at most 3 u.  The quotient adds u: E_a = (rho_D + u) |a|, at most 4 u |a| (32 u for |g| <= 8).  Saturation: where e reaches
FLT_MAX (g < -88.72) expf may return Inf and a becomes g / Inf = -0, while the true value, down to 2.6e-37, is still above eta: there
E_a is at least |a| itself.
silu, a' = s (1 + g (1 - s)).  s carries rho = rho_D + u relative (the quotient).  1 - s cancels: absolute rho s + u c.  Times g:
|g| (rho s + u c) + u |g| c.  Plus one: that, plus u |1 + g c|.  Times s: E_da = s (|g| (rho s + 2 u c) + u |1 + g c|) + (rho + u) |a'|.
For g < -87.3 s is below eta and may be flushed: eta (2 + |g|) covers its product with 1 + g (1 - s); the saturation as for a.
gelu, a = (g * 0.5) * (1 + erff(g * alpha)).  alpha is rounded (u) and so is the product (u): the argument moves by 2 u |x|, erf by at
most 2 u p(x), p(x) = 2 / sqrt(pi) |x| exp(-x^2) <= 0.484.  erff adds 2 ulp(erf x): that is 4 u |erf| at worst but 2 u next to +-1, where
the sum 1 + erf cancels and nothing else is left of it.  d_erf = 2 u p + 2 ulp(erf x).  The sum: d_w = d_erf + u (1 + erf x).  g * 0.5 is
exact; the product adds u |a|: E_a = |g| / 2 d_w + u |a| (24 u at g = 8, 8 u at g = -8 where a itself is 5e-15).
gelu, a' = fmaf(g, expf(-0.5 g g) kBeta, 0.5 (1 + erff(g kAlpha))).  cdf = 0.5 (1 + erf) carries d_w / 2.  The argument of expf is (-0.5
g) g, one rounding (the first product is exact): E = exp(-g^2 / 2) moves by E expm1(u g^2 / 2), expf adds ulp(E); kBeta's rounding and
the product add 2 u E kBeta: d_pdf = kBeta (E expm1(u g^2 / 2) + ulp(E)) + 2 u E kBeta.  The fma rounds once: E_da = |g| d_pdf + d_w / 2 +
u |a'|.
Every bound gets + eta (for a' of silu eta (2 + |g|), for gelu's pdf eta |g|): an absolute floor wherever a value or an intermediate
is below float32's normals.  relu: both factors are exact, the bounds are zero.
For |g| <= 8 the bounds stay below the constants ``ACT_ERR`` of tests/test_mx_glu_train.py (asserted in tests/test_mx_glu_f64.py).
For large |g| they stay true but grow with |g| (the derivation does not use that erff and expf saturate to exact values there).

Non-finite arguments follow the expressions, in float64 as in float32: silu(-Inf) = -Inf * 0 = NaN, gelu(-Inf) = NaN, act'(+-Inf) =
NaN.  The bounds are 0 there: such values are compared by class (``within_glu``)."""
import math

import torch

import mx_gemm_ref as G
from mx_ref import BLOCK, FORMATS, grid

U = 2.0 ** -24
ETA = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -20
ALPHA = math.sqrt(0.5)
BETA = 2.0 / math.sqrt(math.pi) * math.sqrt(0.5) * 0.5          # 1 / sqrt(2 pi)
FLT_MAX = (2.0 - 2.0 ** -23) * 2.0 ** 127
ACTS = ("silu", "gelu", "relu")
CAP = 0.02                       # the largest exempt share of elements and of blocks any case may have


# ---- the 32-run interleave of v, restated (the package's mx_glu_interleave along the last dim) ----------------------------------------
def interleave(gate, up):
    """[..., 2 H]: runs of 32 gate columns followed by the 32 up columns of the same hidden units"""
    H = gate.shape[-1]
    lead = gate.shape[:-1]
    return torch.stack((gate.reshape(lead + (H // BLOCK, BLOCK)), up.reshape(lead + (H // BLOCK, BLOCK))), -2).reshape(lead + (2 * H,))


def deinterleave(v):
    """(gate, up) [..., H] of v [..., 2 H]"""
    N = v.shape[-1]
    c = v.reshape(v.shape[:-1] + (N // (2 * BLOCK), 2, BLOCK))
    return tuple(c.select(-2, i).reshape(v.shape[:-1] + (N // 2,)) for i in (0, 1))


# ---- the functions ------------------------------------------------------------------------------------------------------------------
def _relu_like(g, positive):
    return torch.where(g > 0, positive, torch.where(g != g, g, torch.zeros_like(g)))


def act64(g, act):
    """act(g) in float64: g sigmoid(g), g Phi(g) (the erf form, through erfc: no cancellation in the tail), or the package's ReLU (NaN
    stays NaN, everything else not positive becomes +0)"""
    g = g.double()
    if act == "relu":
        return _relu_like(g, g)
    if act == "silu":
        return g * torch.sigmoid(g)
    assert act == "gelu", act
    return g * (0.5 * torch.erfc(-g * ALPHA))


def dact64(g, act):
    """act'(g) in float64"""
    g = g.double()
    if act == "relu":
        return _relu_like(g, torch.ones_like(g))
    if act == "silu":
        return torch.sigmoid(g) * (1 + g * torch.sigmoid(-g))
    assert act == "gelu", act
    return 0.5 * torch.erfc(-g * ALPHA) + g * (torch.exp(-0.5 * g * g) * BETA)


def _ulp32(y):
    return G.ulp(y, torch.float32)


def _finish(E, g):
    return torch.where(g.isfinite(), E, torch.zeros_like(E))


def _silu_parts(g):
    s, c = torch.sigmoid(g), torch.sigmoid(-g)
    rho_d = U * (1 + 2 * c)
    saturated = -g >= math.log(FLT_MAX) - 1e-5           # expf(-g) may already be Inf
    return s, c, rho_d, saturated


def _gelu_dw(g):
    x = g * ALPHA
    er = torch.erf(x)
    p = 2 / math.sqrt(math.pi) * x.abs() * torch.exp(-x * x)
    return 2 * U * p + 2 * _ulp32(er) + U * torch.erfc(-x)


def E_a(g, act):
    """absolute bound on |act_float32(g) - act64(g)| for the header's expression, pointwise (module docstring)"""
    g = g.double()
    if act == "relu":
        return torch.zeros_like(g)
    gf = torch.where(g.isfinite(), g, torch.zeros_like(g))
    a = act64(gf, act).abs()
    if act == "silu":
        s, c, rho_d, saturated = _silu_parts(gf)
        E = SLACK * (rho_d + U) * a + ETA
        return _finish(torch.where(saturated, torch.maximum(E, a + ETA), E), g)
    return _finish(SLACK * (gf.abs() / 2 * _gelu_dw(gf) + U * a) + ETA, g)


def E_da(g, act):
    """absolute bound on |act'_float32(g) - dact64(g)| for the header's expression, pointwise (module docstring)"""
    g = g.double()
    if act == "relu":
        return torch.zeros_like(g)
    gf = torch.where(g.isfinite(), g, torch.zeros_like(g))
    da = dact64(gf, act).abs()
    ag = gf.abs()
    if act == "silu":
        s, c, rho_d, saturated = _silu_parts(gf)
        rho = rho_d + U
        E = SLACK * (s * (ag * (rho * s + 2 * U * c) + U * (1 + gf * c).abs()) + (rho + U) * da) + ETA * (2 + ag)
        return _finish(torch.where(saturated, torch.maximum(E, da + ETA * (2 + ag)), E), g)
    Eg = torch.exp(-0.5 * gf * gf)
    moved = torch.where(Eg > 0, Eg * torch.expm1((U * 0.5 * gf * gf).clamp(max=1.0)), torch.zeros_like(Eg))
    d_pdf = BETA * (moved + _ulp32(Eg)) + 2 * U * Eg * BETA + ETA
    return _finish(SLACK * (ag * d_pdf + _gelu_dw(gf) / 2 + U * da) + ETA, g)


# ---- the float outputs --------------------------------------------------------------------------------------------------------------
def glu64(v, act):
    """z = act64(g) * u in float64 from the pre-activations v [..., 2 H], widened"""
    g, up = deinterleave(v.detach().cpu().double())
    return act64(g, act) * up


def glu_bound(v, act, dtype):
    """bound on |z - glu64(v)| for z = act(g) * u evaluated in float32 and rounded once to `dtype`: |u| E_a(g) from the activation, u |a u|
    from the one float32 product, and half an ulp of `dtype` at the float64 value (for float32 that is the product's roundoff once
    more, and the subnormal spacing where z is below the normals).  0 where g or u is not finite"""
    g, up = deinterleave(v.detach().cpu().double())
    z = act64(g, act) * up
    fin = g.isfinite() & up.isfinite() & z.isfinite()
    zf = torch.where(fin, z, torch.zeros_like(z))
    b = torch.where(fin, up.abs(), torch.zeros_like(up)) * E_a(g, act) + U * zf.abs() + 0.5 * G.ulp(zf, dtype)
    return torch.where(fin, b, torch.zeros_like(b))


def _overflow(dtype):
    """the magnitude from which a value rounds to Inf in `dtype`: the largest finite one plus half its ulp"""
    emax = 15 if dtype == torch.float16 else 127
    return 2.0 ** (emax + 1) * (1 - 2.0 ** -(G.MANT[dtype] + 1))


def within_glu(y, z64, bound, dtype):
    """(ok, largest |err| / bound over the finite outputs).  NaN exactly where z64 is NaN; where z64 is +-Inf that Inf; a finite z64
    whose magnitude less the bound rounds to Inf in `dtype` must be that Inf, one that reaches the overflow threshold only with the
    bound may be either; everything else finite and within the bound"""
    y = y.detach().cpu().double()
    if not torch.equal(y.isnan(), z64.isnan()):
        return False, float("inf")
    nan = z64.isnan()
    inf_out = y.isinf()
    sign_ok = torch.signbit(y) == torch.signbit(z64)
    must = (~nan) & (z64.abs() - bound >= _overflow(dtype))
    may = (~nan) & (z64.abs() + bound >= _overflow(dtype))
    ok = bool((inf_out[must] & sign_ok[must]).all()) and bool((~inf_out | (may & sign_ok))[~nan].all())
    fin = (~nan) & (~inf_out) & (~must)
    err = torch.where(fin, (y - z64).abs(), torch.zeros_like(y))
    b = torch.where(fin, bound, torch.ones_like(bound))
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return ok and bool((err <= b)[fin].all()), float(ratio.max()) if ratio.numel() else 0.0


def dv64(dh, v, act):
    """(dv [T, 2 H] in float64, its bound): dg = (d u_) act'(g), du = d act(g) on the widened inputs, interleaved like v, and dv_bound"""
    g, up = deinterleave(v.detach().cpu().double())
    d = dh.detach().cpu().double()
    return interleave(d * up * dact64(g, act), d * act64(g, act)), dv_bound(d, up, g, act)


def dv_bound(d, up, g, act):
    """bound on |dv_float32 - dv64|, interleaved, for |g| <= 8 (asserted).  tests/test_mx_glu_train.py states |d u_| (E_da + 3 u) for dg = (d *
    u_) * act'(g) -- two products, 2 u relative, |act'| <= 1.13 -- and |d| (E_a + 8 u) for du = d * act(g) -- one product, u |d a| <= 8 u |d|.
    Here the products' share is taken at the value it is relative to, pointwise like E: |d u_| (E_da(g) + 2 u SLACK |act'(g)|) and |d|
    (E_a(g) + u |act(g)|, E_a carrying the second order), which never exceed the stated form (``dv_bound_stated``; asserted in tests/test_mx_glu_f64.py) and are zero
    where relu makes the element an exact zero.  No operand may be small enough for a float32 underflow: nothing here covers one"""
    d, up, g = d.double(), up.double(), g.double()
    assert bool((g.abs() <= 8).all()), "dv_bound is stated for |g| <= 8"
    return interleave((d * up).abs() * (E_da(g, act) + 2 * U * SLACK * dact64(g, act).abs()),
                      d.abs() * (E_a(g, act) + U * act64(g, act).abs()))


def dv_bound_stated(d, up, g, act):
    """the form of tests/test_mx_glu_train.py with the pointwise E: the ceiling of dv_bound"""
    d, up, g = d.double(), up.double(), g.double()
    return interleave((d * up).abs() * (E_da(g, act) + 3 * U), d.abs() * (E_a(g, act) + 8 * U))


# ---- the code-level comparison -------------------------------------------------------------------------------------------------------
def _flog2(x):
    """floor(log2 x) of float64 x > 0; -10^4 for x <= 0"""
    e = torch.frexp(torch.where(x > 0, x, torch.ones_like(x)))[1] - 1
    return torch.where(x > 0, e, torch.full_like(e, -10000)).to(torch.int64)


def _to_blocks(t, axis, fill=0):
    t = t.movedim(axis, -1)
    n = t.shape[-1]
    nb = -(-n // BLOCK)
    pad = torch.full(t.shape[:-1] + (nb * BLOCK - n,), fill, dtype=t.dtype)
    return torch.cat([t, pad], -1).reshape(t.shape[:-1] + (nb, BLOCK)), n


def codes_compare(codes, scales, fmt, ref64, tol, axis=-1):
    """The masks behind ``codes_agree``, in block layout [..., blocks, 32] along `axis` (a short last block padded): a dict with `wrong`
    (elements whose code is neither exempt nor the reference's), `wrong_block` (blocks whose scale byte is not allowed), `exempt`,
    `exempt_block` and `real` (not padding).

    The reference is ref64 quantized by the MX definition in float64 (tests/mx_ref.py's, widened): per block X = 2^(clamp(floor(log2
    amax) - emax, -127, 127)), byte 0 for an all-zero block, 0xFF and codes 0 for one that holds a NaN or an Inf; the code of v / X is
    the nearest grid value of min(|v / X|, largest normal), ties to the even mantissa, with v's sign bit.
    Exemptions come from ref64 and tol alone.  A block: the code under test saw some amax within [max_i (|r_i| - tol_i), max_i (|r_i| +
    tol_i)]; where a power of two lies inside (the floors of the two log2 differ) either byte is allowed, otherwise the reference's
    alone.  The codes of every block are compared under the byte the code under test wrote.  An element: exempt where |r| / X is
    within tol / X of a midpoint between two neighbouring grid values.  The clamp at the largest normal is no boundary (everything
    beyond the last midpoint has one code).  Where 0 < |r| <= tol and the reference's code has magnitude zero, the bound does not decide
    the sign of what the code under test saw: of such an element (`sign_free`, from the reference alone; its share is printed) the
    magnitude must be zero and the sign bit is not compared.  An exact zero of the reference (relu's) keeps its sign.  A finite value
    that float32 cannot hold makes its block a 0xFF block, as an Inf does."""
    eb, mb, bias, emax, top = FORMATS[fmt]
    gvals, gcode = grid(fmt)
    mids = (gvals[:-1] + gvals[1:]) / 2
    r, n = _to_blocks(ref64.detach().cpu().double(), axis)
    t, _ = _to_blocks(tol.detach().cpu().double(), axis)
    c, _ = _to_blocks(codes.detach().cpu().to(torch.int64), axis)
    real, _ = _to_blocks(torch.ones(ref64.shape, dtype=torch.bool), axis, False)
    byte = scales.detach().cpu().to(torch.int64).movedim(axis, -1)
    assert byte.shape == r.shape[:-1], (byte.shape, r.shape)
    over = r.isfinite() & (r.abs() - t >= _overflow(torch.float32))          # finite in float64, Inf in float32
    assert not bool((r.isfinite() & ~over & (r.abs() + t >= _overflow(torch.float32))).any()), "a value the bound cannot keep from float32's overflow"
    bad = ((~r.isfinite()) | over).any(-1)
    r0 = torch.where(bad.unsqueeze(-1), torch.zeros_like(r), r)
    lo, hi, mid = (r0.abs() - t).amax(-1), (r0.abs() + t).amax(-1), r0.abs().amax(-1)

    def byte_of(amax):
        return torch.where(amax > 0, (_flog2(amax) - emax).clamp(-127, 127) + 127, torch.zeros_like(byte))

    b_ref, b_lo, b_hi = byte_of(mid), byte_of(lo), byte_of(hi)
    exempt_block = (~bad) & (b_lo != b_hi)
    allowed = torch.where(bad, byte == 255, torch.where(exempt_block, (byte >= b_lo) & (byte <= b_hi), byte == b_ref))
    X = torch.pow(torch.tensor(2.0, dtype=torch.float64), (torch.where(allowed & ~bad, byte, b_ref) - 127).double()).unsqueeze(-1)
    q, tq = r0 / X, t / X
    want = _quantize(q, fmt)[1]
    want = torch.where(bad.unsqueeze(-1), torch.zeros_like(want), want)
    exempt = (~bad.unsqueeze(-1)) & real & (((q.abs().unsqueeze(-1) - mids).abs().amin(-1)) <= tq)
    magnitude = (1 << (eb + mb)) - 1
    sign_free = real & (q != 0) & (q.abs() <= tq) & ((want & magnitude) == 0)
    differs = torch.where(sign_free, (c & magnitude) != 0, c != want)
    wrong_block = ~allowed
    wrong = real & ((differs & ~exempt) | wrong_block.unsqueeze(-1))
    return dict(wrong=wrong, wrong_block=wrong_block, exempt=exempt, exempt_block=exempt_block, real=real, sign_free=sign_free)


def _quantize(q, fmt):
    """(value, code) of q (float64, already divided by the block's X): the nearest grid value of min(|q|, largest normal), ties to
    the even mantissa, with q's sign"""
    eb, mb, bias, emax, top = FORMATS[fmt]
    gvals, gcode = grid(fmt)
    a = q.abs().clamp(max=top)
    up_i = torch.bucketize(a, gvals).clamp(max=len(gvals) - 1)
    lo_i = (up_i - 1).clamp(min=0)
    dlo, dhi = a - gvals[lo_i], gvals[up_i] - a
    pick = torch.where(dlo < dhi, lo_i, torch.where(dhi < dlo, up_i, torch.where(lo_i % 2 == 0, lo_i, up_i)))
    return torch.copysign(gvals[pick], q), gcode[pick] + (torch.signbit(q).to(torch.int64) << (eb + mb))


def quant_spread(fmt, ref64, tol):
    """[..., n]: how far apart the dequantized MX values (blocks along the last dim) of two float32 tensors can lie that are both within
    tol of ref64, from the reference alone.  The quantizer is monotone under one scale, so in a block whose scale byte tol cannot
    move it is Q(r + tol) - Q(r - tol): zero wherever r is further than tol from every rounding midpoint.  In a block whose byte may
    differ (``codes_compare``'s exempt_block) every value is at most twice the block's largest magnitude: 4 max (|r| + tol)"""
    emax = FORMATS[fmt][3]
    r, n = _to_blocks(ref64.detach().cpu().double(), -1)
    t, _ = _to_blocks(tol.detach().cpu().double(), -1)
    assert bool(r.isfinite().all())
    lo, hi, mid = (r.abs() - t).amax(-1), (r.abs() + t).amax(-1), r.abs().amax(-1)
    e = lambda amax: torch.where(amax > 0, (_flog2(amax) - emax).clamp(-127, 127), torch.full_like(_flog2(amax), -127))
    X = torch.pow(torch.tensor(2.0, dtype=torch.float64), e(mid).double()).unsqueeze(-1)
    D = (_quantize((r + t) / X, fmt)[0] - _quantize((r - t) / X, fmt)[0]) * X
    D = torch.where((e(lo) != e(hi)).unsqueeze(-1), 4 * hi.unsqueeze(-1).expand_as(D), D)
    return D.reshape(D.shape[:-2] + (-1,))[..., :n]


def exempt_shares(fmt, ref64, tol, axis=-1):
    """(share of elements, share of blocks) that ``codes_agree`` would exempt: from the reference alone, no codes involved"""
    shape = list(ref64.shape)
    shape[axis] = -(-shape[axis] // BLOCK)
    m = codes_compare(torch.zeros(ref64.shape, dtype=torch.uint8), torch.zeros(shape, dtype=torch.uint8), fmt, ref64, tol, axis)
    return float(m["exempt"].sum()) / max(int(m["real"].sum()), 1), float(m["exempt_block"].sum()) / max(m["exempt_block"].numel(), 1)


def codes_agree(codes, scales, fmt, ref64, tol, axis=-1, what=""):
    """asserts that every scale byte and every code equals the float64 reference's but for the exemptions of ``codes_compare``, and
    that the exempt shares stay within CAP; returns (exempt share of elements, exempt share of blocks)"""
    m = codes_compare(codes, scales, fmt, ref64, tol, axis)
    share = float(m["exempt"].sum()) / max(int(m["real"].sum()), 1)
    share_b = float(m["exempt_block"].sum()) / max(m["exempt_block"].numel(), 1)
    free = float(m["sign_free"].sum()) / max(int(m["real"].sum()), 1)
    print(f"{what} {fmt}: exempt {share:.4%} of elements, {share_b:.4%} of blocks; sign of a zero code free in {free:.4%}")
    assert share <= CAP and share_b <= CAP, (what, fmt, share, share_b)
    assert not bool(m["wrong_block"].any()), (what, fmt, "scale bytes", int(m["wrong_block"].sum()))
    assert not bool(m["wrong"].any()), (what, fmt, "codes", int(m["wrong"].sum()))
    return share, share_b


# ---- one training step on two devices ------------------------------------------------------------------------------------------------
def linear_step_bounds(xq, wq, fmts, bias, dh, act, v_a, v_b, dv_codes_a):
    """(B_y, B_dx, B_dw): bounds on |y_a - y_b|, |dx_a - dx_b|, |dw_a - dw_b| of one ``mx_glu_linear`` step run on a device A whose products
    follow the instruction's model (``mx_gemm_ref.model_bound``) and on a device B whose products are float64 sums rounded once (the CPU
    path).  `xq`, `wq`: (row codes, row scales, col codes, col scales) of x and W, the same bits on both devices (the quantizers are
    pinned bit for bit elsewhere); `fmts` = (x_fmt, w_fmt, grad_fmt); `v_a`, `v_b` the float32 pre-activations of either device and
    `dv_codes_a` A's four outputs of the backward quantizer, used ONLY as said below.  Derivation:

    v.  Both are asserted here against the float64 product v64 of the codes: |v_a - v64| <= model_bound, |v_b - v64| <= ulp(v64) + 2^-23
    |bias|.  Everything after rests on that.
    y = act(g) u.  |y_a - glu64(v_a)| <= glu_bound(v_a), the same for B, and glu64(v_a) - glu64(v_b) is evaluated in float64: B_y is the
    sum of the three.
    dv.  The float32 dv of either device is within dv_bound of dv64 on its own v; the two float64 values are subtracted in float64.  So
    both float32 tensors lie within tau = dv_bound(v_a) + dv_bound(v_b) + |dv64(v_a) - dv64(v_b)| of dv64(v_b), and their dequantized MX
    values differ by at most D = quant_spread(grad_fmt, dv64(v_b), tau), along 2 H for the row pair and along T for the col pair: zero
    wherever tau does not reach a rounding midpoint.  D comes from the reference alone: a wrong derivative on A is not in it.
    dx = Q_row(dv) Q_col(W)^T.  dx_a is within model_bound of the float64 product P_a of A's own codes (A's codes enter this bound of
    A's product and nothing else), dx_b within one float32 ulp of P_b, and |P_a - P_b| <= D |Q_col(W)|^T: B_dx is the sum, the ulp
    taken at |P_a| + D |W|.  dw = Q_col(dv) Q_col(x)^T likewise along T (at T <= 128 the weight gradient is one K step: no split)."""
    fx, fw, fg = fmts
    v64, S = G.reference(xq[0], xq[1], fx, wq[0], wq[1], fw, bias)[1:]
    mb = G.model_bound(xq[0], xq[1], fx, wq[0], wq[1], fw, v64, S, bias)
    cpu = G.ulp(v64, torch.float32) + (0 if bias is None else 2.0 ** -23 * bias.cpu().double().abs())
    assert bool(((v_a.cpu().double() - v64).abs() <= mb).all()) and bool(((v_b.cpu().double() - v64).abs() <= cpu).all())
    B_y = glu_bound(v_a, act, torch.float32) + glu_bound(v_b, act, torch.float32) + (glu64(v_a, act) - glu64(v_b, act)).abs()
    (ref_a, tol_a), (ref_b, tol_b) = dv64(dh, v_a, act), dv64(dh, v_b, act)
    tau = tol_a + tol_b + (ref_a - ref_b).abs()
    out = []
    for codes, scales, other, fo, D in ((dv_codes_a[0], dv_codes_a[1], wq[2:], fw, quant_spread(fg, ref_b, tau)),
                                      (dv_codes_a[2], dv_codes_a[3], xq[2:], fx, quant_spread(fg, ref_b.t(), tau.t()))):
        codes, scales = codes.cpu(), scales.cpu()
        P, S = G.reference(codes, scales, fg, other[0], other[1], fo)[1:]
        moved = SLACK * (D @ G.values(other[0], other[1], fo).abs().t())
        out.append(G.model_bound(codes, scales, fg, other[0], other[1], fo, P, S) + G.ulp(P.abs() + moved, torch.float32) + moved)
    return B_y, out[0], out[1]


# ---- the input sets of both test files ----------------------------------------------------------------------------------------------
BWD_SHAPES = ((130, 96), (144, 96), (33, 32), (1, 32))
BWD_DTYPES = ((torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.float16, torch.bfloat16))      # (dh, v)
FWD_SHAPES = ((45, 32, 40), (144, 96, 64))          # (M, H, K): N = 2 H = 64 and 192
FWD_FMTS = ("mxfp6_e2m3", "mxfp4_e2m1", "mxfp8_e4m3")
BWD_FMTS = FWD_FMTS + ("mxfp8_e5m2",)
FA, FB = "mxfp8_e4m3", "mxfp6_e2m3"                   # the operand formats of the forward cases


NARROW_LOW = -4.0


def bwd_plan(T):
    """[(narrow, fmt, pairs)]: which input set each format's pairs are compared on.  E5M2 takes the narrowed gates for both pairs.  The
    other formats take the wide ones, but for the col pair at T = 1 and T = 33, whose last block along T holds one element: that pair
    alone takes the narrowed gates (bwd_inputs says why); their row pair stays on the wide ones"""
    plan = []
    for fmt in BWD_FMTS:
        if fmt == "mxfp8_e5m2":
            plan.append((True, fmt, ("row", "col")))
        elif T % BLOCK == 1:
            plan += [(False, fmt, ("row",)), (True, fmt, ("col",))]
        else:
            plan.append((False, fmt, ("row", "col")))
    return plan


def bwd_inputs(T, H, ddt=torch.float32, vdt=torch.float32, narrow=False):
    """(dh [T, H] in ddt, v [T, 2 H] in vdt) on the CPU.  Half of the gates are uniform in [-3, 3], where silu and gelu bend, the other
    half in [-8, 8]; up is normal times 2; dh is normal times a per-column factor from 0.1 to 10.
    `narrow`: the gates' lower end is -4 in place of -8.  Below it gelu's absolute error (2 u |g| and more, from the cancellation in 1 +
    erff) is no longer small next to gelu itself (|gelu(-5)| = 1.4e-6 against a bound of 6e-7).  FP6, FP4 and E4M3 round such an element
    to zero next to the others of its block, and zero it is under any error; E5M2 spans 2^-31 of the block's largest element in
    steps of a quarter of the value and resolves it, so its code is not decided by the bound: with the gates down to -8 a tenth of
    gelu's elements would be exempt.  The same happens in any format to an element that is alone in its block, as along T at T = 1 and T = 33."""
    gen = torch.Generator().manual_seed(1000 + 7 * T + H + (5 if narrow else 0))
    low = NARROW_LOW if narrow else -8.0
    wide = torch.rand(T, H, generator=gen) * (8.0 - low) + low
    bend = torch.rand(T, H, generator=gen) * 6 - 3
    g = torch.where(torch.rand(T, H, generator=gen) < 0.5, bend, wide)
    up = torch.randn(T, H, generator=gen) * 2
    d = torch.randn(T, H, generator=gen) * torch.logspace(-1, 1, H)
    return d.to(ddt), interleave(g, up).to(vdt)


def fwd_operands(M, H, K, E=None):
    """(a_codes [M, K], a_scales, b_codes [2 H, K] or [E, 2 H, K], b_scales, bias [2 H] or [E, 2 H]) of mx_gemm_ref's EXACT CLASS: every
    product, every partial sum and the bias added to it are exact in float32, so v is the same bits on every device and equals the
    float64 sum.  Scale bytes 124 for a and 123 .. 124 for b: the gates come out roughly normal with a deviation of 2 to 5, at least
    half of them inside [-3, 3] and some beyond +-8 (asserted where they are used)."""
    gen = torch.Generator().manual_seed(2000 + M + H + K + (E or 0))
    ra, rb = 1, 2
    G.assert_exact_class(K, FA, FB, ra, rb)
    a = G.exact_operand(gen, M, K, FA, ra, 124)
    n = 2 * H * (E or 1)
    b = G.exact_operand(gen, n, K, FB, rb, 123)
    bias = torch.randint(-32, 33, (n,), generator=gen).float() / 16          # multiples of 2^-4; the products' quantum is 2^-10
    if E is not None:
        b = tuple(t.reshape(E, 2 * H, -1) for t in b)
        bias = bias.reshape(E, 2 * H)
    return a + b + (bias,)
