"""Test helper of the convolution on MX codes: the im2col operands of the definition, built in pure torch on whatever device the
codes are on.  ``mx_conv2d`` is defined as ``mx_matmul`` on ``A [B OH OW, K']`` and ``Wp [Cout, K']`` with ``K' = KH KW Cp``, ``Cp =
32 ceil(C / 32)`` and ``k' = (kh KW + kw) Cp + c``: codes padded spatially and along C with the zero code, scales padded spatially
with 127 (2^0)."""
import torch
import torch.nn.functional as F

BLOCK = 32


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_size(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def _windows(t, KH, KW, stride, padding, dilation, fill):
    """t [B, H, W, E] -> [B * OH * OW, KH * KW * E], windows gathered in (kh, kw, e) order, `fill` outside the image"""
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    B, H, W, E = t.shape
    OH, OW = out_size(H, KH, sh, ph, dh), out_size(W, KW, sw, pw, dw)
    tp = F.pad(t, (0, 0, pw, pw, ph, ph), value=fill)
    taps = []
    for kh in range(KH):
        for kw in range(KW):
            taps.append(tp[:, kh * dh: kh * dh + (OH - 1) * sh + 1: sh, kw * dw: kw * dw + (OW - 1) * sw + 1: sw, :])
    return torch.stack(taps, dim=3).reshape(B * OH * OW, KH * KW * E).contiguous()


def im2col_codes(x_codes, x_scales, w_codes, w_scales, KH, KW, stride=1, padding=0, dilation=1):
    """(A [M, K'], SA [M, K' / 32], Wp [Cout, K'], SWp [Cout, K' / 32]) of x_codes [B, H, W, C] / w_codes [Cout, KH, KW, C]"""
    stride, padding, dilation = pair(stride), pair(padding), pair(dilation)
    C, Cout = x_codes.shape[-1], w_codes.shape[0]
    Cp = -(-C // BLOCK) * BLOCK
    xc, wc = F.pad(x_codes, (0, Cp - C)), F.pad(w_codes, (0, Cp - C))                  # zero codes up to Cp
    A = _windows(xc, KH, KW, stride, padding, dilation, 0)
    SA = _windows(x_scales, KH, KW, stride, padding, dilation, 127)
    return A, SA, wc.reshape(Cout, KH * KW * Cp).contiguous(), w_scales.reshape(Cout, KH * KW * (Cp // BLOCK)).contiguous()


def conv64(x_vals, w_vals, bias, stride, padding, dilation):
    """float64 F.conv2d of channels-last value tensors x [B, H, W, C], w [Cout, KH, KW, C] -> [B, OH, OW, Cout]"""
    y = F.conv2d(x_vals.permute(0, 3, 1, 2), w_vals.permute(0, 3, 1, 2), None if bias is None else bias.cpu().double(), pair(stride),
                 pair(padding), pair(dilation))
    return y.permute(0, 2, 3, 1).contiguous()
