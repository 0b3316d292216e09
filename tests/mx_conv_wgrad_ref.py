"""Test helper of the convolution's weight gradient on MX codes: the gathered operands of the definition, built in pure torch on
whatever device the codes are on, from integer index arithmetic alone.  ``mx_conv2d_weight_grad`` is defined as ``mx_matmul`` on
``G [Cout, K']`` and ``X' [KH KW C, K']`` with ``Bp = 32 ceil(B / 32)``, ``K' = OH OW Bp`` and ``k' = (oh OW + ow) Bp + b``:

    G[n, k'] = dyt[oh, ow, n, b]        X'[(kh KW + kw) C + c, k'] = xt[oh sh - ph + kh dh, ow sw - pw + kw dw, c, b]

the zero code where ``b >= B`` or the tap lies outside the image; the scale byte of a block that does not exist (a tap outside the
image) is 127."""
import torch
import torch.nn.functional as F

BLOCK = 32


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_size(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def axis_taps(n, k, s, p, d, device="cpu"):
    """(index [out, k] int64, inside [out, k] bool): the input position tap j of output position o reads, and whether it is inside"""
    o = torch.arange(out_size(n, k, s, p, d), dtype=torch.int64, device=device).view(-1, 1)
    i = o * s - p + torch.arange(k, dtype=torch.int64, device=device).view(1, -1) * d
    inside = (i >= 0) & (i < n)
    return torch.where(inside, i, torch.zeros_like(i)), inside


def gathered_codes(dyt_codes, dyt_scales, xt_codes, xt_scales, kernel_size, stride=1, padding=0, dilation=1):
    """(G [Cout, K'], SG [Cout, K' / 32], X' [KH KW C, K'], SX' [KH KW C, K' / 32]) of dyt_codes [OH, OW, Cout, B] / xt_codes
    [H, W, C, B]"""
    (KH, KW), (sh, sw), (ph, pw), (dh, dw) = pair(kernel_size), pair(stride), pair(padding), pair(dilation)
    (OH, OW, Cout, B), (H, W, C, _) = dyt_codes.shape, xt_codes.shape
    dev = xt_codes.device
    Bp = -(-B // BLOCK) * BLOCK
    nb = Bp // BLOCK
    ih, eh = axis_taps(H, KH, sh, ph, dh, dev)
    iw, ew = axis_taps(W, KW, sw, pw, dw, dev)
    assert (ih.shape[0], iw.shape[0]) == (OH, OW), "dyt is not the gradient of this convolution"
    Gc = F.pad(dyt_codes, (0, Bp - B)).permute(2, 0, 1, 3).reshape(Cout, OH * OW * Bp).contiguous()       # zero codes up to Bp
    SG = dyt_scales.permute(2, 0, 1, 3).reshape(Cout, OH * OW * nb).contiguous()
    inside = (eh.view(OH, KH, 1, 1) & ew.view(1, 1, OW, KW)).view(OH, KH, OW, KW, 1, 1)
    rows, cols = ih.view(OH, KH, 1, 1), iw.view(1, 1, OW, KW)
    xc = F.pad(xt_codes, (0, Bp - B))[rows, cols]                                                         # [OH, KH, OW, KW, C, Bp]
    xs = xt_scales[rows, cols]                                                                            # [OH, KH, OW, KW, C, nb]
    Xc = torch.where(inside, xc, torch.zeros((), dtype=torch.uint8, device=dev))
    SX = torch.where(inside, xs, torch.full((), 127, dtype=torch.uint8, device=dev))
    Xc = Xc.permute(1, 3, 4, 0, 2, 5).reshape(KH * KW * C, OH * OW * Bp).contiguous()
    SX = SX.permute(1, 3, 4, 0, 2, 5).reshape(KH * KW * C, OH * OW * nb).contiguous()
    return Gc, SG, Xc, SX


def taps_reading(H, W, KH, KW, stride=1, padding=0, dilation=1):
    """[H, W, KH, KW] bool, written as the scatter of the definition (independent of the gather above): some output pixel reads
    input pixel (ih, iw) through tap (kh, kw)"""
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(padding), pair(dilation)
    out = torch.zeros(H, W, KH, KW, dtype=torch.bool)
    for oh in range(out_size(H, KH, sh, ph, dh)):
        for kh in range(KH):
            ih = oh * sh - ph + kh * dh
            if not 0 <= ih < H:
                continue
            for ow in range(out_size(W, KW, sw, pw, dw)):
                for kw in range(KW):
                    iw = ow * sw - pw + kw * dw
                    if 0 <= iw < W:
                        out[ih, iw, kh, kw] = True
    return out


def wgrad64(dy_vals, x_vals, kernel_size, stride=1, padding=0, dilation=1):
    """float64 ``torch.nn.grad.conv2d_weight`` of batch-last value tensors dy [OH, OW, Cout, B], x [H, W, C, B] -> [Cout, KH, KW, C]"""
    KH, KW = pair(kernel_size)
    dy, x = dy_vals.permute(3, 2, 0, 1).contiguous(), x_vals.permute(3, 2, 0, 1).contiguous()
    dw = torch.nn.grad.conv2d_weight(x, (dy.shape[1], x.shape[1], KH, KW), dy, pair(stride), pair(padding), pair(dilation))
    return dw.permute(0, 2, 3, 1).contiguous()
