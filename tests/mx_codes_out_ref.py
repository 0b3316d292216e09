"""Test helper of the MX products that write MX codes (``mx_matmul(..., out_fmt=)``, ``mx_conv2d(..., out_fmt=)``): the composition they
are defined as -- the float32 product, the activation, ``quantize_with_mx`` along the last axis -- on whatever device the codes are on,
and seeded operands with a wide spread of block scales."""
import torch
import torch.nn as nn

from qsparse_amd.mx_conv import MXConv2d, mx_conv2d
from qsparse_amd.mx_gemm import MXLinear, mx_matmul
from qsparse_amd.quantize import MX_FORMATS, quantize_with_mx

FORMATS = list(MX_FORMATS)


def relu(y):
    """NaN stays NaN, everything else that is not positive becomes +0"""
    return torch.where(y > 0, y, torch.where(y != y, y, torch.zeros_like(y)))


def quantized(y, out_fmt, act):
    _, codes, scales = quantize_with_mx(relu(y) if act == "relu" else y, out_fmt, -1, return_codes=True)
    return codes, scales


def matmul_composition(ac, asc, fa, bc, bsc, fb, bias, out_fmt, act):
    return quantized(mx_matmul(ac, asc, fa, bc, bsc, fb, bias), out_fmt, act)


def conv_composition(xc, xs, fx, wc, ws, fw, bias, stride, padding, dilation, out_fmt, act):
    return quantized(mx_conv2d(xc, xs, fx, wc, ws, fw, bias, stride, padding, dilation), out_fmt, act)


def operand(g, shape, fmt, device="cpu", spread=12):
    """(codes, scales) of a seeded randn tensor whose rows (all but the last axis) are scaled by 2^[-spread, spread]"""
    x = torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-spread, spread + 1, tuple(shape[:-1]) + (1,), generator=g).float())
    _, codes, scales = quantize_with_mx(x.to(device), fmt, -1, return_codes=True)
    return codes, scales


def same(got, want):
    return all(g.shape == w.shape and g.dtype == torch.uint8 and torch.equal(g, w) for g, w in zip(got, want))


def linear_chain(device, out_fmt="mxfp4_e2m1", seed=3):
    """(fused chain, first layer plain, second layer, x): 48 -> 70 -> 9 features"""
    g = torch.Generator().manual_seed(seed)
    w1, w2 = operand(g, (70, 48), "mxfp8_e4m3", device, 2), operand(g, (9, 70), "mxfp6_e3m2", device, 2)
    b1, b2 = torch.randn(70, generator=g).to(device), torch.randn(9, generator=g).to(device)
    first = MXLinear(*w1, "mxfp8_e4m3", b1, "mxfp8_e5m2", out_fmt=out_fmt, act="relu")
    plain = MXLinear(*w1, "mxfp8_e4m3", b1, "mxfp8_e5m2")
    second = MXLinear(*w2, "mxfp6_e3m2", b2, act_fmt=out_fmt)
    return nn.Sequential(first, second), plain, second, torch.randn(2, 5, 48, generator=g).to(device)


def conv_chain(device, out_fmt="mxfp8_e4m3", seed=4):
    """(fused chain, first layer plain, second layer, x): 3x3, stride 2, padding 1, C = 40 -> 48 -> 8"""
    g = torch.Generator().manual_seed(seed)
    w1, w2 = operand(g, (48, 3, 3, 40), "mxfp4_e2m1", device, 2), operand(g, (8, 3, 3, 48), "mxfp8_e4m3", device, 2)
    b1, b2 = torch.randn(48, generator=g).to(device), torch.randn(8, generator=g).to(device)
    first = MXConv2d(*w1, "mxfp4_e2m1", b1, 2, 1, 1, "mxfp6_e2m3", out_fmt=out_fmt, act="relu")
    plain = MXConv2d(*w1, "mxfp4_e2m1", b1, 2, 1, 1, "mxfp6_e2m3")
    second = MXConv2d(*w2, "mxfp8_e4m3", b2, 2, 1, 1, act_fmt=out_fmt)
    return nn.Sequential(first, second), plain, second, torch.randn(2, 40, 13, 11, generator=g).to(device)
