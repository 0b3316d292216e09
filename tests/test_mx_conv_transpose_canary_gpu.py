"""Out-of-bounds check for the transposed convolution on MX codes, in the manner of tests/test_mx_conv_canary_gpu.py: the five
operands and the output of every call are carved out of larger allocations whose margins hold a byte pattern; after the launch the
margins must be intact (y: nothing written past it; the inputs: unchanged) and the body equal the float64 transposed convolution.
Margins on both sides also mean that a read past an operand -- a tap of a row past M, a pixel left of the first image or below the
last one, a piece past C -- would pick up the pattern instead of zeros and show in the result.  M and Cout that are no multiples of
the tile (128), Cout % 4 != 0 (the scalar stores of the epilogue), crops and output paddings are where the clamped fetch and the
store would reach too far."""
import ctypes

import pytest
import torch

import mx_conv_transpose_ref as T
import mx_gemm_ref as G
from mx_guard import guarded as _guarded, intact as _intact
from qsparse_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


CASES = [  # B, H, W, C, Cout, (KH, KW), stride, padding, output_padding, dilation, byte offset of the code bases, expected route
    (3, 5, 4, 48, 130, (3, 3), (2, 2), (1, 1), (1, 1), (1, 1), 0, _hip.MX_CONV_ROUTE_VEC),        # M = 240, N = 130, Cp = 64
    (2, 3, 4, 16, 3, (3, 2), (2, 3), (2, 1), (1, 2), (1, 2), 0, _hip.MX_CONV_ROUTE_VEC),          # Cout = 3; a crop and an output padding
    (2, 4, 5, 40, 131, (3, 3), (1, 2), (2, 1), (0, 1), (1, 1), 0, _hip.MX_CONV_ROUTE_PLAIN),      # C % 16 != 0, N % 4 != 0
    (1, 3, 4, 3, 7, (2, 2), (3, 3), (0, 0), (2, 2), (1, 1), 3, _hip.MX_CONV_ROUTE_PLAIN),         # holes, at an odd base
    (2, 5, 4, 48, 21, (3, 3), (2, 2), (1, 1), (1, 1), (1, 1), 1, _hip.MX_CONV_ROUTE_PLAIN),       # VEC-eligible but for the base
]


@pytest.mark.parametrize("fx,fw", [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp8_e5m2"), ("mxfp6_e3m2", "mxfp6_e3m2")])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_margins_survive_every_route(fx, fw, out_dtype):
    lib = _hip.load()
    osz = torch.empty(0, dtype=out_dtype).element_size()
    for B, H, W, C, Cout, (KH, KW), stride, padding, out_pad, dilation, off, route in CASES:
        g = torch.Generator().manual_seed(H * 1000 + C + Cout)
        Kp = KH * KW * (-(-C // 32) * 32)
        rx, rw = G.scale_windows(Kp, fx, fw)
        G.assert_exact_class(Kp, fx, fw, rx, rw)
        ops = G.exact_operand(g, B * H * W, C, fx, rx) + G.exact_operand(g, Cout * KH * KW, C, fw, rw)
        bias = torch.randint(-16, 16, (Cout,), generator=g).float()
        guarded = []
        for t in ops:
            raw, body = _guarded(t.numel(), off)
            body.copy_(t.reshape(-1).to(DEV))
            guarded.append((raw, body, t.numel(), off))
        braw, bbody = _guarded(Cout * 4)
        bbody.copy_(bias.view(torch.uint8).to(DEV))
        OH = T.out_size(H, KH, stride[0], padding[0], dilation[0], out_pad[0])
        OW = T.out_size(W, KW, stride[1], padding[1], dilation[1], out_pad[1])
        assert (B * OH * OW) % 128 != 0 and Cout % 128 != 0
        ynum = B * OH * OW * Cout
        yoff = osz if off else 0                                                # y needs its element's alignment, nothing more
        yraw, ybody = _guarded(ynum * osz, yoff)
        a = _hip.MxConvTranspose2dArgs()
        a.struct_size = ctypes.sizeof(a)
        a.x_format, a.w_format = _hip.MX_FORMATS.index(fx), _hip.MX_FORMATS.index(fw)
        a.x_codes, a.x_scales, a.w_codes, a.w_scales = (b.data_ptr() for _, b, _, _ in guarded)
        a.bias, a.y, a.ydt = bbody.data_ptr(), ybody.data_ptr(), _hip._DT[out_dtype]
        a.B, a.H, a.W, a.C, a.Cout, a.KH, a.KW = B, H, W, C, Cout, KH, KW
        (a.stride_h, a.stride_w), (a.pad_h, a.pad_w), (a.dil_h, a.dil_w), (a.out_pad_h, a.out_pad_w) = stride, padding, dilation, out_pad
        a.stream = _hip._stream(ybody)
        what = (fx, fw, out_dtype, B, H, W, C, Cout, KH, KW, off)
        assert lib.qs_mx_conv_transpose2d_route(ctypes.byref(a)) == route, what
        assert lib.qs_mx_conv_transpose2d_v(ctypes.byref(a)) == 0, what
        torch.cuda.synchronize()
        assert _intact(yraw, ynum * osz, yoff), ("y", what)
        for name, (raw, body, n, o), t in zip(("x_codes", "x_scales", "w_codes", "w_scales"), guarded, ops):
            assert _intact(raw, n, o) and torch.equal(body.cpu(), t.reshape(-1)), (name, what)
        assert _intact(braw, Cout * 4), ("bias", what)
        xv = G.values(ops[0], ops[1], fx).view(B, H, W, C)
        wv = G.values(ops[2], ops[3], fw).view(Cout, KH, KW, C)
        want = T.conv_transpose64(xv, wv, bias, stride, padding, out_pad, dilation).to(out_dtype)
        assert G.same(ybody.clone().view(out_dtype).view(B, OH, OW, Cout), want), what
