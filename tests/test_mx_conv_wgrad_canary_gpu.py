"""Out-of-bounds check for the convolution's weight gradient on MX codes, in the manner of tests/test_mx_conv_transpose_canary_gpu.py:
the four operands, the output and the split-K workspace of every call are carved out of larger allocations whose margins hold a
byte pattern; after the launch the margins must be intact (dW and the workspace: nothing written past them; the inputs: unchanged)
and the body equal the float64 weight gradient.  The workspace is given S' * Cout * KH KW C * 4 bytes exactly.  Margins on both
sides also mean that a read past an operand -- a row past Cout or KH KW C, a tap outside the image, a piece past B, the steps past
K' of the last slice -- would pick up the pattern instead of zeros and show in the result."""
import ctypes

import pytest
import torch

import mx_conv_wgrad_ref as R
import mx_gemm_ref as G
from mx_guard import PAD, PATTERN, guarded as _guarded, intact as _intact
from qsparse_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


CASES = [  # B, H, W, C, Cout, (KH, KW), stride, padding, dilation, byte offset of the code bases, split_k, expected route
    (48, 5, 4, 10, 130, (3, 3), (1, 1), (1, 1), (1, 1), 0, 1, _hip.MX_CONV_ROUTE_VEC),         # M = 130, N = 90; a partial batch block
    (48, 5, 4, 10, 130, (3, 3), (1, 1), (1, 1), (1, 1), 0, 3, _hip.MX_CONV_ROUTE_VEC),         # 10 steps in slices of 4, 4, 2
    (16, 6, 5, 3, 7, (3, 2), (2, 1), (2, 1), (1, 2), 0, 2, _hip.MX_CONV_ROUTE_VEC),            # N = 18, M = 7; padding 2, dilation 2
    (20, 5, 4, 15, 131, (3, 3), (1, 2), (1, 0), (1, 1), 0, 1, _hip.MX_CONV_ROUTE_PLAIN),       # B % 16 != 0, N % 4 != 0
    (20, 5, 4, 15, 131, (3, 3), (1, 2), (1, 0), (1, 1), 0, 2, _hip.MX_CONV_ROUTE_PLAIN),       # ... split: scalar stores to the workspace
    (5, 4, 4, 3, 7, (2, 2), (1, 1), (0, 0), (1, 1), 3, 2, _hip.MX_CONV_ROUTE_PLAIN),           # a small batch at an odd base
    (32, 5, 4, 16, 21, (3, 3), (1, 1), (1, 1), (1, 1), 1, 2, _hip.MX_CONV_ROUTE_PLAIN),        # VEC-eligible but for the base
]


@pytest.mark.parametrize("fg,fx", [("mxfp8_e5m2", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp8_e5m2"), ("mxfp6_e3m2", "mxfp6_e3m2")])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_margins_survive_every_route(fg, fx, out_dtype):
    lib = _hip.load()
    osz = torch.empty(0, dtype=out_dtype).element_size()
    for B, H, W, C, Cout, (KH, KW), stride, padding, dilation, off, split_k, route in CASES:
        g = torch.Generator().manual_seed(H * 1000 + C + Cout)
        OH, OW = (R.out_size(n, k, s, p, d) for n, k, s, p, d in zip((H, W), (KH, KW), stride, padding, dilation))
        Bp = -(-B // 32) * 32
        Kp, N = OH * OW * Bp, KH * KW * C
        rg, rx = G.scale_windows(Kp, fg, fx)
        G.assert_exact_class(Kp, fg, fx, rg, rx)
        ops = G.exact_operand(g, OH * OW * Cout, B, fg, rg) + G.exact_operand(g, H * W * C, B, fx, rx)
        guarded = []
        for t in ops:
            raw, body = _guarded(t.numel(), off)
            body.copy_(t.reshape(-1).to(DEV))
            guarded.append((raw, body, t.numel(), off))
        steps = -(-Kp // 128)
        per = -(-steps // split_k)
        slices = -(-steps // per)
        assert slices == split_k and Cout % 128 != 0 and N % 128 != 0
        planned, nbytes = _hip.mx_conv_wgrad_plan(Cout, N, Kp, split_k)
        assert planned == slices and nbytes == (slices * Cout * N * 4 if slices > 1 else 0)
        wraw, wbody = _guarded(max(nbytes, 16))
        ynum = Cout * N
        yoff = osz if off else 0                                                # dW needs its element's alignment, nothing more
        yraw, ybody = _guarded(ynum * osz, yoff)
        a = _hip.MxConv2dWgradArgs()
        a.struct_size = ctypes.sizeof(a)
        a.dy_format, a.x_format = _hip.MX_FORMATS.index(fg), _hip.MX_FORMATS.index(fx)
        a.dyt_codes, a.dyt_scales, a.xt_codes, a.xt_scales = (b.data_ptr() for _, b, _, _ in guarded)
        a.dw, a.ydt, a.split_k = ybody.data_ptr(), _hip._DT[out_dtype], split_k
        a.B, a.H, a.W, a.C, a.Cout, a.OH, a.OW, a.KH, a.KW = B, H, W, C, Cout, OH, OW, KH, KW
        (a.stride_h, a.stride_w), (a.pad_h, a.pad_w), (a.dil_h, a.dil_w) = stride, padding, dilation
        a.workspace, a.workspace_bytes = (wbody.data_ptr(), nbytes) if slices > 1 else (None, 0)
        a.stream = _hip._stream(ybody)
        what = (fg, fx, out_dtype, B, H, W, C, Cout, KH, KW, off, split_k)
        assert lib.qs_mx_conv2d_wgrad_route(ctypes.byref(a)) == route, what
        if slices > 1:                                                          # one byte short: refused, nothing enqueued
            a.workspace_bytes = nbytes - 1
            assert lib.qs_mx_conv2d_wgrad_v(ctypes.byref(a)) == -4, what
            a.workspace_bytes = nbytes
        assert lib.qs_mx_conv2d_wgrad_v(ctypes.byref(a)) == 0, what
        torch.cuda.synchronize()
        assert _intact(yraw, ynum * osz, yoff), ("dw", what)
        assert bool((wraw[:PAD] == PATTERN).all()) and bool((wraw[PAD + nbytes:] == PATTERN).all()), ("workspace", what)
        for name, (raw, body, n, o), t in zip(("dyt_codes", "dyt_scales", "xt_codes", "xt_scales"), guarded, ops):
            assert _intact(raw, n, o) and torch.equal(body.cpu(), t.reshape(-1)), (name, what)
        gv = G.values(ops[0], ops[1], fg).view(OH, OW, Cout, B)
        xv = G.values(ops[2], ops[3], fx).view(H, W, C, B)
        want = R.wgrad64(gv, xv, (KH, KW), stride, padding, dilation).to(out_dtype)
        assert G.same(ybody.clone().view(out_dtype).view(Cout, KH, KW, C), want), what
