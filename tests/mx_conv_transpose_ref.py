"""Test helper of the transposed convolution on MX codes: the gathered operands of the definition, built in pure torch on whatever
device the codes are on, from integer index arithmetic alone.  ``mx_conv_transpose2d`` is defined as ``mx_matmul`` on ``A [B OH OW,
K']`` and ``Wp [Cout, K']`` with ``K' = KH KW Cp``, ``Cp = 32 ceil(C / 32)`` and ``k' = (kh KW + kw) Cp + c``:

    A[(b, oh, ow), k'] = x[b, (oh + ph - kh dh) / sh, (ow + pw - kw dw) / sw, c]

where both divisions are exact and the pixel lies inside the image; the zero code with scale byte 127 everywhere else (a tap that
does not exist, c >= C).  ``Wp`` is the weight as it lies, its channels padded to ``Cp``: the kernel indices are not flipped."""
import torch
import torch.nn.functional as F

BLOCK = 32


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_size(n, k, s, p, d, op):
    return (n - 1) * s - 2 * p + d * (k - 1) + op + 1


def axis_taps(n, k, s, p, d, op, device="cpu"):
    """(index [out, k] int64, exists [out, k] bool): the input position tap j of output position o reads, and whether it exists"""
    o = torch.arange(out_size(n, k, s, p, d, op), dtype=torch.int64, device=device).view(-1, 1)
    t = o + p - torch.arange(k, dtype=torch.int64, device=device).view(1, -1) * d
    q = torch.div(t, s, rounding_mode="floor")
    exists = (t >= 0) & (q * s == t) & (q < n)
    return torch.where(exists, q, torch.zeros_like(q)), exists


def taps_exist(H, W, KH, KW, stride=1, padding=0, output_padding=0, dilation=1):
    """[OH, OW, KH, KW] bool: tap (kh, kw) of output pixel (oh, ow) exists"""
    (sh, sw), (ph, pw), (oph, opw), (dh, dw) = pair(stride), pair(padding), pair(output_padding), pair(dilation)
    eh, ew = axis_taps(H, KH, sh, ph, dh, oph)[1], axis_taps(W, KW, sw, pw, dw, opw)[1]
    return eh.view(-1, 1, KH, 1) & ew.view(1, -1, 1, KW)


def gathered_codes(x_codes, x_scales, w_codes, w_scales, stride=1, padding=0, output_padding=0, dilation=1):
    """(A [M, K'], SA [M, K' / 32], Wp [Cout, K'], SWp [Cout, K' / 32]) of x_codes [B, H, W, C] / w_codes [Cout, KH, KW, C]"""
    (sh, sw), (ph, pw), (oph, opw), (dh, dw) = pair(stride), pair(padding), pair(output_padding), pair(dilation)
    (B, H, W, C), (Cout, KH, KW, _) = x_codes.shape, w_codes.shape
    dev = x_codes.device
    Cp = -(-C // BLOCK) * BLOCK
    nb = Cp // BLOCK
    ih, eh = axis_taps(H, KH, sh, ph, dh, oph, dev)
    iw, ew = axis_taps(W, KW, sw, pw, dw, opw, dev)
    OH, OW = ih.shape[0], iw.shape[0]
    exists = (eh.view(OH, 1, KH, 1) & ew.view(1, OW, 1, KW)).expand(B, OH, OW, KH, KW).reshape(-1)
    b = torch.arange(B, dtype=torch.int64, device=dev).view(B, 1, 1, 1, 1)
    px = ((b * H + ih.view(1, OH, 1, KH, 1)) * W + iw.view(1, 1, OW, 1, KW)).reshape(-1)
    px = torch.where(exists, px, torch.zeros_like(px))
    xc = F.pad(x_codes, (0, Cp - C)).reshape(-1, Cp)                              # zero codes up to Cp
    A = torch.where(exists.view(-1, 1), xc[px], torch.zeros((), dtype=torch.uint8, device=dev))
    SA = torch.where(exists.view(-1, 1), x_scales.reshape(-1, nb)[px], torch.full((), 127, dtype=torch.uint8, device=dev))
    M = B * OH * OW
    Wp = F.pad(w_codes, (0, Cp - C)).reshape(Cout, KH * KW * Cp).contiguous()
    return A.view(M, KH * KW * Cp).contiguous(), SA.view(M, KH * KW * nb).contiguous(), Wp, w_scales.reshape(Cout, KH * KW * nb).contiguous()


def conv_transpose64(x_vals, w_vals, bias, stride=1, padding=0, output_padding=0, dilation=1):
    """float64 F.conv_transpose2d of channels-last value tensors x [B, H, W, C], w [Cout, KH, KW, C] -> [B, OH, OW, Cout]"""
    y = F.conv_transpose2d(x_vals.permute(0, 3, 1, 2), w_vals.permute(3, 0, 1, 2), None if bias is None else bias.cpu().double(),
                           pair(stride), pair(padding), pair(output_padding), 1, pair(dilation))
    return y.permute(0, 2, 3, 1).contiguous()
