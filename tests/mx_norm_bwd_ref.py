"""The definition of the MX norm backward (include/qsparse_hip.h, "MX norm backward") restated for the tests of ``mx_norm_backward``:
the fixed order of the column sums built from strided slices and element-wise additions, the three results one torch op per rounding,
and the input generator.  The row sums, the float64 evaluation and the margins are ``mx_norm_ref.py``'s.  Nothing here calls the code
under test; the statistics are the forward's, ``mx_norm_quantize(..., return_stats=True)`` on the CPU."""
import torch

import mx_norm_ref as NR
from qsparse_amd import mx_norm_quantize

SHAPES = ((1, 1), (129, 96), (130, 100), (67, 1056), (300, 520), (16520, 40))


def ref_col_sum(t):
    """sum over the rows of float32 t [R, C]: +0 padding to a multiple of 128 rows; in row tile k, S_l = 0 + t[128 k + l] + t[128 k +
    l + 16] + ... in ascending order, l < 16, then S_l += S_(l+s) for s = 8 .. 1; over the tile sums v_k, P_j = 0 + v_j + v_(j+128)
    + ..., j < 128, then P_j += P_(j+s) for s = 64 .. 1"""
    R, C = t.shape
    T = (R + 127) // 128
    p = torch.zeros(T * 128, C, dtype=torch.float32, device=t.device)
    p[:R] = t
    v = torch.zeros(((T + 127) // 128) * 128, C, dtype=torch.float32, device=t.device)
    for k in range(T):
        tile = p[128 * k:128 * (k + 1)]
        S = torch.zeros(16, C, dtype=torch.float32, device=t.device)
        for m in range(8):
            S = S + tile[16 * m:16 * (m + 1)]
        for s in (8, 4, 2, 1):
            S = S[:s] + S[s:2 * s]
        v[k] = S[0]
    P = torch.zeros(128, C, dtype=torch.float32, device=t.device)
    for k in range(v.shape[0] // 128):
        P = P + v[128 * k:128 * (k + 1)]
    for s in (64, 32, 16, 8, 4, 2, 1):
        P = P[:s] + P[s:2 * s]
    return P[0]


def ref_backward(dxhat, x, rstd, mean, w):
    """(dx float32 -- before its one rounding to x's dtype --, dweight, dbias) of the definition; mean None: rms mode"""
    d = dxhat.to(torch.float32)
    x32 = x.to(torch.float32)
    cf = torch.tensor(float(x.shape[1]), dtype=torch.float32)
    xhat = (x32 if mean is None else x32 - mean[:, None]) * rstd[:, None]
    g = d if w is None else d * w
    c1 = NR.ref_sum(g * xhat) / cf
    inner = g - xhat * c1[:, None]
    if mean is not None:
        c2 = NR.ref_sum(g) / cf
        inner = inner - c2[:, None]
    return rstd[:, None] * inner, ref_col_sum(d * xhat), ref_col_sum(d)


_cases = {}


def case(R, C, dtype, norm, has_w=True, gdtype=torch.float32):
    """(dxhat, x, rstd, mean | None, w | None) as `_train_case` of test_mx_norm.py draws them: x = 3 randn + 0.5, w = rand + 0.5, dxhat =
    randn; the statistics from the forward (eps 1e-6).  Computed once per key and shared: do not write into them"""
    key = (R, C, dtype, norm, has_w, gdtype)
    if key not in _cases:
        g = torch.Generator().manual_seed(7919 * R + C)
        x = (torch.randn(R, C, generator=g) * 3 + 0.5).to(dtype)
        w = torch.rand(C, generator=g) + 0.5
        dxhat = torch.randn(R, C, generator=g).to(gdtype)
        rstd, mean = mx_norm_quantize(x, w if has_w else None, norm=norm, eps=NR.EPS, return_stats=True)[-2:]
        _cases[key] = (dxhat, x, rstd, mean, w if has_w else None)
    return _cases[key]


_refs = {}


def reference(R, C, dtype, norm, has_w=True, gdtype=torch.float32):
    """`ref_backward` of `case(...)`, computed once per key"""
    key = (R, C, dtype, norm, has_w, gdtype)
    if key not in _refs:
        _refs[key] = ref_backward(*case(*key))
    return _refs[key]
