"""The definition of the MX normalising quantizer (include/qsparse_hip.h, "MX normalising quantizer") restated for the tests of
``mx_norm.py``: the fixed summation order built from slices and element-wise additions, the float32 ``y``, the float64 evaluation of
the same formulas, the normalisation's backward and the input generators.  Nothing here calls the code under test."""
import torch

from qsparse_amd import mx_quantize_2way, quantize_with_mx

FMTS = ("mxfp8_e4m3", "mxfp8_e5m2", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp4_e2m1")
DTS = (torch.float32, torch.bfloat16, torch.float16)
NORMS = ("rms", "layer")
WB = ((False, False), (True, False), (False, True), (True, True))       # (weight, bias) present
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
EPS = 1e-6


def same(a, b):
    """bit for bit, a NaN equal to a NaN"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    return bool(((a.view(INT[a.dtype]) == b.view(INT[b.dtype])) | (a.isnan() & b.isnan())).all())


def ref_sum(t):
    """sum over the columns of float32 t [R, C]: +0 padding to a multiple of 512; q_m = (t_4m + t_4m+1) + (t_4m+2 + t_4m+3); P_j = 0 +
    q_j + q_(j+128) + ... in ascending order, j < 128; then P_j += P_(j+s) for s = 64 .. 1"""
    R, C = t.shape
    K = (C + 511) // 512
    p = torch.zeros(R, K * 512, dtype=torch.float32, device=t.device)
    p[:, :C] = t
    q = (p[:, 0::4] + p[:, 1::4]) + (p[:, 2::4] + p[:, 3::4])
    P = torch.zeros(R, 128, dtype=torch.float32, device=t.device)
    for k in range(K):
        P = P + q[:, 128 * k:128 * (k + 1)]
    for s in (64, 32, 16, 8, 4, 2, 1):
        P = P[:, :s] + P[:, s:2 * s]
    return P[:, 0]


def ref_y(x, w, b, norm, eps=EPS):
    """(y float32 [R, C], rstd [R], mean [R] | None) of x [R, C] by the definition, one torch op per rounding"""
    x32 = x.to(torch.float32)
    cf = torch.tensor(float(x.shape[1]), dtype=torch.float32, device=x.device)
    e = torch.tensor(eps, dtype=torch.float32, device=x.device)
    mean = None
    d = x32
    if norm == "layer":
        mean = ref_sum(x32) / cf
        d = x32 - mean[:, None]
    ms = ref_sum(d * d) / cf
    root = torch.sqrt((ms + e).double()).float()        # the correctly rounded float32 sqrt (torch's float32 CPU sqrt is not: its last
    rstd = torch.ones_like(ms) / root                   #  bit differs between machines; a float64 root rounded once more is)
    rstd = torch.where(torch.isfinite(ms), rstd, torch.full_like(ms, float("nan")))
    y = d * rstd[:, None]
    if w is not None:
        y = y * w
    if b is not None:
        y = y + b
    return y, rstd, mean


def ref_quant(y, fmt, col_fmt=None):
    """(codes, scales, col_codes | None, col_scales | None) of the float32 y by the quantizers the package had before"""
    _, rc, rs = quantize_with_mx(y, fmt, -1, return_codes=True)
    cc, cs = mx_quantize_2way(y, None, col_fmt)[2:] if col_fmt is not None else (None, None)
    return rc, rs, cc, cs


def y_float64(x, w, b, norm, eps=EPS):
    """(y, rstd, mean) of the same formulas in float64 (plain sums), from the float32 widening of the operands"""
    x64 = x.to(torch.float64)
    e = float(torch.tensor(eps, dtype=torch.float32))
    mean = x64.mean(-1, keepdim=True) if norm == "layer" else torch.zeros(x.shape[0], 1, dtype=torch.float64)
    d = x64 - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + e)
    y = d * rstd
    if w is not None:
        y = y * w.to(torch.float64)
    if b is not None:
        y = y + b.to(torch.float64)
    return y, rstd, mean


def inputs(seed, R, C, dtype, has_w=True, has_b=True):
    """randn rows with a per-row scale in [2^-6, 2^6], w in [0.5, 1.5], b randn (float32 parameters)"""
    g = torch.Generator().manual_seed(seed)
    scale = torch.exp2(torch.rand(R, 1, generator=g) * 12 - 6)
    x = (torch.randn(R, C, generator=g) * scale).to(dtype)
    w = (torch.rand(C, generator=g) + 0.5) if has_w else None
    b = torch.randn(C, generator=g) if has_b else None
    return x, w, b


def norm_backward_ref(dxhat, x, rstd, mean, w, norm, dtype=torch.float32):
    """(dx, d norm_weight, d norm_bias) by the formulas of ``mx_norm_linear``'s docstring in `dtype` arithmetic"""
    dxhat, x, rstd = dxhat.to(dtype), x.to(dtype), rstd.to(dtype)
    xhat = (x if mean is None else x - mean.to(dtype)[:, None]) * rstd[:, None]
    g = dxhat if w is None else dxhat * w.to(dtype)
    inner = g - xhat * (g * xhat).mean(-1, keepdim=True)
    if norm == "layer":
        inner = inner - g.mean(-1, keepdim=True)
    return rstd[:, None] * inner, (dxhat * xhat).sum(0), dxhat.sum(0)


def norm_backward_margins(dxhat, x, rstd, mean, w, norm):
    """the first-order float32 error bounds of the three results against their float64 evaluation, with u = 2^-23 --
    twice the unit roundoff, which absorbs the second-order terms and the reference's own rounding.  Any summation order of n terms
    errs by at most (n - 1) u' sum|t|.  With A = mean_C|g xhat| and G = mean_C|g| (C terms), R rows:
        dx    : rstd (4 |g| + (C + 10) |xhat| A + (C + 4) G)     g 1 rounding, xhat 2, the products 1 each, the sums C - 1, the
                                                                 divisions 1, two subtractions and the last product 3 on every term
        dw    : (R + 2) sum_R |dxhat xhat|                       xhat 2, the product 1, the sum R - 1
        db    : (R - 1) sum_R |dxhat|"""
    u = 2.0 ** -23
    f = torch.float64
    dxhat, x, rstd = dxhat.to(f), x.to(f), rstd.to(f)
    R, C = x.shape
    xhat = (x if mean is None else x - mean.to(f)[:, None]) * rstd[:, None]
    g = dxhat if w is None else dxhat * w.to(f)
    A = (g * xhat).abs().mean(-1, keepdim=True)
    G = g.abs().mean(-1, keepdim=True) if norm == "layer" else torch.zeros_like(A)
    m_dx = u * rstd[:, None] * (4 * g.abs() + (C + 10) * xhat.abs() * A + (C + 4) * G)
    m_dw = u * (R + 2) * (dxhat * xhat).abs().sum(0)
    m_db = u * (R - 1) * dxhat.abs().sum(0)
    return m_dx, m_dw, m_db
