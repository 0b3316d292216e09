"""The definition of the MX softmax quantizer (include/qsparse_hip.h, "MX softmax quantizer") a second time, for the tests of
``mx_softmax.py``: numpy float32, row by row, with its own ``E``, its own row-sum order and its own NaN rule, plus the seeded inputs.
Nothing here calls the code under test or shares text with it; only the last step -- ``p`` to codes -- is ``quantize_with_mx``, the
quantizer the definition names."""
import numpy as np
import torch

from qsparse_amd import quantize_with_mx

FMTS = ("mxfp8_e4m3", "mxfp8_e5m2", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp4_e2m1")
DTS = (torch.float32, torch.bfloat16, torch.float16)
SIZES = (1, 31, 32, 33, 197, 512, 513)
F = np.float32
# the constants by their bit patterns, as the header prints them
LOG2E, LN2_HI, LN2_LO = (np.array([b], dtype=np.uint32).view(F)[0] for b in (0x3fb8aa3b, 0x3f318000, 0xb95e8083))
COEF = [np.array([b], dtype=np.uint32).view(F)[0] for b in (0x39500d01, 0x3ab60b61, 0x3c088889, 0x3d2aaaab, 0x3e2aaaab)] + [F(0.5), F(1), F(1)]
NEG_INF = F(-np.inf)


def ref_exp(t):
    """E(t) on a float32 array t <= 0 (-inf allowed): every numpy operation is one float32 rounding"""
    t = np.asarray(t, dtype=F)
    out = np.zeros(t.shape, dtype=F)
    live = t >= F(-87.0)
    tl = t[live]
    n = np.rint(tl * LOG2E)                                    # ties to even
    r = (tl - n * LN2_HI) - n * LN2_LO
    P = np.full(tl.shape, COEF[0], dtype=F)
    for c in COEF[1:]:
        P = P * r
        P = P + c
    out[live] = np.ldexp(P, n.astype(np.int32))
    assert out.dtype == F
    return out


def ref_row_sum(e):
    """the sum of one float32 row in the header's order: +0 padding to a multiple of 512, quads, 128 partial sums in ascending
    order, the pairwise tree (float32 array additions: one rounding each)"""
    S = e.shape[0]
    K = (S + 511) // 512
    pad = np.zeros(K * 512, dtype=F)
    pad[:S] = e
    P = np.zeros(128, dtype=F)
    for k in range(K):
        w = pad[512 * k:512 * (k + 1)]
        P = P + ((w[0::4] + w[1::4]) + (w[2::4] + w[3::4]))     # partial sum j takes the quad 128 k + j
    for s in (64, 32, 16, 8, 4, 2, 1):
        P = P[:s] + P[s:2 * s]
    assert P.dtype == F
    return P[0]


def ref_p(s, scale, mask=None, causal=False):
    """p float32 [G, T, S] (numpy) of the tensor s [G, T, S] by the definition; `mask`: additive float32 tensor [T, S] or [G, T, S]"""
    s32 = s.to(torch.float32).numpy()
    G, T, S = s32.shape
    a = None if mask is None else mask.to(torch.float32).numpy()
    sc = F(scale)
    p = np.empty((G, T, S), dtype=F)
    with np.errstate(all="ignore"):
        for g in range(G):
            for t in range(T):
                u = s32[g, t] * sc
                if a is not None:
                    u = u + (a[t] if a.ndim == 2 else a[g, t])
                if causal:
                    u = u.copy()
                    u[t + 1:] = NEG_INF                         # L = t + 1
                assert u.dtype == F
                if np.isnan(u).any() or np.max(u) == np.inf or np.max(u) == -np.inf:
                    p[g, t] = np.nan                            # the row is NaN as a whole
                    continue
                e = ref_exp(u - np.max(u))
                p[g, t] = e / ref_row_sum(e)
    return p


def ref_codes(p, fmt):
    """(codes, scales) of the float32 p by the quantizer the package had before"""
    _, c, sc = quantize_with_mx(torch.from_numpy(p), fmt, -1, return_codes=True)
    return c, sc


def scores(seed, shape, dtype):
    """seeded randn * 3: logits whose softmax spans the formats' range"""
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 3).to(dtype)


def float_mask(seed, shape):
    """an additive float32 mask: randn with a fifth of the entries at -inf, column 0 always admitted"""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(*shape, generator=g)
    m = m.masked_fill(torch.rand(*shape, generator=g) < 0.2, float("-inf"))
    m[..., 0] = 0.5
    return m


def bool_mask(seed, shape):
    """a boolean mask that admits about two thirds of the columns, column 0 always"""
    b = torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) < 0.66
    b[..., 0] = True
    return b


def additive(b):
    """what a boolean mask adds: 0 where True, -inf where False"""
    return torch.zeros(b.shape, dtype=torch.float32).masked_fill(~b, float("-inf"))
