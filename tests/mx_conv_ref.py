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


def taps_inside(n, k, s, p, d):
    """[out, k] bool: tap j of output position o lies inside an axis of length n"""
    o = torch.arange(out_size(n, k, s, p, d)).view(-1, 1)
    i = o * s - p + torch.arange(k).view(1, -1) * d
    return (i >= 0) & (i < n)


def padding_only(H, W, KH, KW, stride=1, padding=0, dilation=1):
    """[OH, OW] bool: the output pixels whose window lies wholly in the padding (no tap inside the image)"""
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(padding), pair(dilation)
    return ~(taps_inside(H, KH, sh, ph, dh).any(1).view(-1, 1) & taps_inside(W, KW, sw, pw, dw).any(1).view(1, -1))


def pixels_read(H, W, KH, KW, stride=1, padding=0, dilation=1):
    """[H, W] bool: the pixels that at least one window covers"""
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(padding), pair(dilation)
    rows, cols = torch.zeros(H, dtype=torch.bool), torch.zeros(W, dtype=torch.bool)
    for n, k, s, p, d, hit in ((H, KH, sh, ph, dh, rows), (W, KW, sw, pw, dw, cols)):
        for o in range(out_size(n, k, s, p, d)):
            for j in range(k):
                i = o * s - p + j * d
                if 0 <= i < n:
                    hit[i] = True
    return rows.view(-1, 1) & cols.view(1, -1)


def gather_windows(x_codes, x_scales, KH, KW, stride, padding, dilation):
    """(A [M, KH KW C], SA [M, KH KW C / 32], largest byte offset of x_codes read) for C % 32 == 0: the im2col operands built by
    gathering only the pixels that are read, from 64-bit pixel numbers computed here -- for tensors too large to pad and slice"""
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(padding), pair(dilation)
    B, H, W, C = x_codes.shape
    assert C % BLOCK == 0
    dev = x_codes.device
    OH, OW = out_size(H, KH, sh, ph, dh), out_size(W, KW, sw, pw, dw)
    i64 = lambda n: torch.arange(n, dtype=torch.int64, device=dev)
    ih = (i64(OH) * sh - ph).view(1, OH, 1, 1, 1) + (i64(KH) * dh).view(1, 1, 1, KH, 1)
    iw = (i64(OW) * sw - pw).view(1, 1, OW, 1, 1) + (i64(KW) * dw).view(1, 1, 1, 1, KW)
    inside = ((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)).expand(B, OH, OW, KH, KW).reshape(-1)
    px = ((i64(B).view(B, 1, 1, 1, 1) * H + ih) * W + iw).reshape(-1)
    px = torch.where(inside, px, torch.zeros_like(px))
    A = torch.where(inside.view(-1, 1), x_codes.view(-1, C)[px], torch.zeros((), dtype=torch.uint8, device=dev))
    SA = torch.where(inside.view(-1, 1), x_scales.view(-1, C // BLOCK)[px], torch.full((), 127, dtype=torch.uint8, device=dev))
    M = B * OH * OW
    return A.view(M, KH * KW * C), SA.view(M, KH * KW * (C // BLOCK)), int(px.max()) * C + C - 1
