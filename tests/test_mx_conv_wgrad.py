"""The weight gradient of a convolution on MX codes, ``mx_conv2d_train`` and ``MXTrainConv2d`` on the CPU, and what of the C ABI
answers without a GPU: the float64 definition against ``torch.nn.grad.conv2d_weight``, the NaN pattern of 0xFF scale bytes, every
argument error, the two-way quantizer's pairs as the products' operands, the autograd function against the composition of the
public calls, the layer, ``qs_mx_conv2d_wgrad_plan`` and the layout of ``qs_mx_conv2d_wgrad_args``."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn as nn

import mx_conv_wgrad_ref as R
import mx_gemm_ref as G
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_conv import MXConv2d, mx_conv2d
from qsparse_amd.mx_conv_train import MXTrainConv2d, mx_conv2d_train, mx_conv2d_weight_grad
from qsparse_amd.mx_conv_transpose import mx_conv2d_input_grad
from qsparse_amd.mx_gemm import mx_matmul, mx_quantize_2way
from qsparse_amd.quantize import quantize_with_mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("mxfp8_e5m2", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp6_e2m3", "mxfp8_e5m2"), ("mxfp8_e4m3", "mxfp4_e2m1")]
# B, H, W, C, Cout, (KH, KW), stride, padding, dilation
GEOMETRIES = [
    (5, 8, 7, 3, 6, (3, 3), 2, 1, 1),                     # stride 2 with a remainder row, B = 5, C = 3
    (32, 7, 6, 8, 5, (3, 2), 1, (2, 0), 2),               # dilation 2, asymmetric padding
    (48, 5, 6, 4, 9, (2, 3), (1, 2), (0, 2), (1, 1)),     # a partial second batch block
    (5, 3, 3, 3, 4, (2, 2), 1, 3, 1),                     # padding beyond the kernel's reach
]


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def out_hw(H, W, ks, stride, padding, dilation):
    (sh, sw), (ph, pw), (dh, dw) = R.pair(stride), R.pair(padding), R.pair(dilation)
    return R.out_size(H, ks[0], sh, ph, dh), R.out_size(W, ks[1], sw, pw, dw)


def batch_blocked(t, fmt):
    B, H, W, C = t.shape
    _, _, cc, cs = mx_quantize_2way(t.reshape(B, -1), None, fmt)
    return cc.view(H, W, C, B), cs.view(H, W, C, -1)


def quantized_case(g, case, fg, fx):
    B, H, W, C, Cout, ks, stride, padding, dilation = case
    OH, OW = out_hw(H, W, ks, stride, padding, dilation)
    x, dy = torch.randn(B, H, W, C, generator=g), torch.randn(B, OH, OW, Cout, generator=g)
    return batch_blocked(dy, fg) + batch_blocked(x, fx)


@pytest.mark.parametrize("fg,fx", PAIRS)
def test_cpu_path_equals_conv2d_weight_in_float64(fg, fx):
    """to within one float32 ulp of the sum of the absolute products (the float64 sums differ in order only; the result is float32)"""
    g = torch.Generator().manual_seed(1)
    for case in GEOMETRIES:
        ks, geom = case[5], case[6:]
        ops = quantized_case(g, case, fg, fx)
        gv, xv = G.values(ops[0], ops[1], fg), G.values(ops[2], ops[3], fx)
        want, S = R.wgrad64(gv, xv, ks, *geom), R.wgrad64(gv.abs(), xv.abs(), ks, *geom)
        for split_k in (1, 3, "auto"):
            dw = mx_conv2d_weight_grad(*ops[:2], fg, *ops[2:], fx, ks, *geom, split_k=split_k)
            assert dw.shape == (case[4], ks[0], ks[1], case[3]) and dw.dtype == torch.float32 and dw.is_contiguous()
            assert G.within(dw, want, G.ulp(S, torch.float32))[0], (case, split_k)
        # the same sum as the matrix product of the gathered operands
        Gc, SG, Xc, SX = R.gathered_codes(*ops, ks, *geom)
        assert G.within(mx_matmul(Gc, SG, fg, Xc, SX, fx).view_as(dw), want, G.ulp(S, torch.float32))[0], case
        for dt in (torch.bfloat16, torch.float16):
            assert G.within(mx_conv2d_weight_grad(*ops[:2], fg, *ops[2:], fx, ks, *geom, dt), want, G.ulp(want, dt))[0], (case, dt)


def test_ff_scale_bytes_give_nan_exactly_where_the_definition_says():
    g = torch.Generator().manual_seed(2)
    fg, fx = "mxfp8_e5m2", "mxfp8_e4m3"
    case = (40, 5, 6, 8, 10, (3, 3), 2, 1, 1)
    ks, geom = case[5], case[6:]
    base = quantized_case(g, case, fg, fx)
    reads = R.taps_reading(5, 6, 3, 3, *geom)
    gc, gs, xc, xs = (t.clone() for t in base)
    xs[2, 3, 5, 1] = 255                                    # the second batch block at pixel (2, 3), channel 5
    nan = torch.zeros(10, 3, 3, 8, dtype=torch.bool)
    nan[:, :, :, 5] = reads[2, 3]
    assert reads[2, 3].nonzero().tolist() == [[1, 0], [1, 2]]
    assert torch.equal(mx_conv2d_weight_grad(gc, gs, fg, xc, xs, fx, ks, *geom).isnan(), nan)
    gc, gs, xc, xs = (t.clone() for t in base)
    gs[1, 2, 7, 0] = 255                                    # channel 7 at one output pixel: dW[7] everywhere, also against padding
    nan = torch.zeros(10, 3, 3, 8, dtype=torch.bool)
    nan[7] = True
    assert torch.equal(mx_conv2d_weight_grad(gc, gs, fg, xc, xs, fx, ks, *geom).isnan(), nan)
    # a pixel no tap reads: stride 2 without padding skips the last row of a 4-row image (OH = 1 for k = 3)
    case = (8, 4, 3, 2, 3, (3, 3), 2, 0, 1)
    gc, gs, xc, xs = quantized_case(g, case, fg, fx)
    xs[3, 1, 0, 0] = 255
    assert not R.taps_reading(4, 3, 3, 3, 2, 0, 1)[3].any()
    assert not mx_conv2d_weight_grad(gc, gs, fg, xc, xs, fx, (3, 3), 2, 0, 1).isnan().any()


def test_argument_errors():
    g = torch.Generator().manual_seed(3)
    f = "mxfp8_e4m3"
    gc, gs, xc, xs = quantized_case(g, (5, 6, 6, 3, 4, (3, 3), 1, 1, 1), f, f)
    call = lambda *a, **k: mx_conv2d_weight_grad(*a, **k)
    ok = (gc, gs, f, xc, xs, f, (3, 3), 1, 1, 1)
    assert call(*ok).shape == (4, 3, 3, 3)
    with pytest.raises(ValueError, match="unknown MX format"):
        call(gc, gs, "fp8", xc, xs, f, 3, 1, 1)
    with pytest.raises(TypeError, match="must be uint8"):
        call(gc.float(), gs, f, xc, xs, f, 3, 1, 1)
    with pytest.raises(TypeError, match="must be a tensor"):
        call(gc, None, f, xc, xs, f, 3, 1, 1)
    with pytest.raises(ValueError, match="needs 4 dimensions"):
        call(gc.view(36, 4, 5), gs.view(36, 4, 1), f, xc, xs, f, 3, 1, 1)
    with pytest.raises(ValueError, match="the batch"):
        call(gc, gs[..., :0], f, xc, xs, f, 3, 1, 1)
    with pytest.raises(ValueError, match="disagree on B"):
        call(gc[..., :4].contiguous(), gs, f, xc, xs, f, 3, 1, 1)
    with pytest.raises(ValueError, match="B, H, W >= 1"):
        call(gc[..., :0], gs[..., :0], f, xc[..., :0], xs[..., :0], f, 3, 1, 1)
    with pytest.raises(ValueError, match="not the gradient"):
        call(gc, gs, f, xc, xs, f, 3, 2, 1)
    with pytest.raises(ValueError, match="not the gradient"):
        call(gc, gs, f, xc, xs, f, (3, 5), 1, 1)
    with pytest.raises(TypeError, match="out_dtype"):
        call(*ok, torch.float64)
    with pytest.raises(ValueError, match="kernel_size must be >= 1"):
        call(gc, gs, f, xc, xs, f, 0, 1, 1)
    with pytest.raises(ValueError, match="stride must be >= 1"):
        call(gc, gs, f, xc, xs, f, 3, 0, 1)
    with pytest.raises(ValueError, match="padding must be"):
        call(gc, gs, f, xc, xs, f, 3, 1, "same")
    with pytest.raises(TypeError, match="dilation must be"):
        call(gc, gs, f, xc, xs, f, 3, 1, 1, 1.0)
    for bad, exc in ((0, ValueError), ("best", ValueError), (2.0, TypeError), (True, TypeError)):
        with pytest.raises(exc, match="split_k"):
            call(*ok, split_k=bad)
    x, w = torch.randn(2, 3, 5, 5), torch.randn(4, 3, 3, 3)
    with pytest.raises(ValueError, match="must be \\[B, C, H, W\\]"):
        mx_conv2d_train(x[:, :2], w)
    with pytest.raises(ValueError, match="weight must be"):
        mx_conv2d_train(x, w[0])
    with pytest.raises(ValueError, match="bias has shape"):
        mx_conv2d_train(x, w, torch.zeros(3))
    with pytest.raises(TypeError, match="must be one of"):
        mx_conv2d_train(x.double(), w)
    with pytest.raises(ValueError, match="B, Cout, C, KH, KW >= 1"):
        mx_conv2d_train(x[:0], w)
    with pytest.raises(ValueError, match="wgrad_split_k"):
        mx_conv2d_train(x, w, wgrad_split_k=0)
    with pytest.raises(ValueError, match="unknown rounding"):
        mx_conv2d_train(x, w, grad_rounding="up")
    with pytest.raises(ValueError, match="does not fit"):
        mx_conv2d_train(x, w, dilation=3)


@pytest.mark.parametrize("fmt", ["mxfp8_e4m3", "mxfp4_e2m1"])
@pytest.mark.parametrize("shape", [(5, 4, 3, 64), (48, 3, 2, 32), (33, 4, 3, 20)])
def test_two_way_pairs_are_the_products_operands(fmt, shape):
    """for a channels-last x [B, H, W, C]: the column pair of mx_quantize_2way(x.view(B, -1)) is the one-way quantizer on
    x.permute(1, 2, 3, 0); the row pair is the forward operand (blocks along C) when C % 32 == 0"""
    B, H, W, C = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(4)) * 3
    rc, rs, cc, cs = mx_quantize_2way(x.view(B, -1), fmt, fmt)
    _, tc, ts = quantize_with_mx(x.permute(1, 2, 3, 0).contiguous(), fmt, -1, return_codes=True)
    assert torch.equal(cc.view(H, W, C, B), tc) and torch.equal(cs.view(H, W, C, -1), ts)
    _, fc, fs = quantize_with_mx(x, fmt, -1, return_codes=True)
    if C % 32 == 0:
        assert torch.equal(rc.view(B, H, W, C), fc) and torch.equal(rs.view(B, H, W, -1), fs)
    else:
        assert rs.shape[1] == -(-H * W * C // 32) and not torch.equal(rc.view(B, H, W, C), fc)         # blocks straddle the pixels


def composed(x, w, b, dy, s, p, d, fx, fw, fg, rounding="nearest", seed=0, step=0):
    """y, dx, dW, db of mx_conv2d_train as the composition of the public calls on channels-last tensors"""
    q = lambda t, f, **k: quantize_with_mx(t.contiguous(), f, -1, return_codes=True, **k)[1:]
    sr = lambda stream: dict(rounding=rounding, seed=seed, step=torch.tensor([step]), stream=stream) if rounding == "stochastic" else {}
    xl, dyl = x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
    y = mx_conv2d(*q(xl, fx), fx, *q(w.permute(0, 2, 3, 1), fw), fw, None if b is None else b.float(), s, p, d, x.dtype)
    dx = mx_conv2d_input_grad(*q(dyl, fg, **sr(0)), fg, *q(w.permute(1, 2, 3, 0), fw), fw, x.shape[2:], s, p, d, x.dtype)
    dw = mx_conv2d_weight_grad(*q(dyl.permute(1, 2, 3, 0), fg, **sr(1)), fg, *q(xl.permute(1, 2, 3, 0), fx), fx, w.shape[2:], s, p, d, w.dtype)
    return y.permute(0, 3, 1, 2), dx.permute(0, 3, 1, 2), dw.permute(0, 3, 1, 2), dyl.contiguous().sum((0, 1, 2), dtype=torch.float32)


@pytest.mark.parametrize("C,Cout", [(32, 64), (3, 20)])
@pytest.mark.parametrize("channels_last", [True, False])
def test_mx_conv2d_train_is_the_composition_of_the_public_calls(C, Cout, channels_last):
    g = torch.Generator().manual_seed(5)
    fx, fw, fg = "mxfp8_e4m3", "mxfp6_e2m3", "mxfp8_e5m2"
    B, H, W, s, p, d = 5, 7, 6, 2, 1, 1
    x = torch.randn(B, C, H, W, generator=g)
    x = x.contiguous(memory_format=torch.channels_last) if channels_last else x
    w, b = torch.randn(Cout, C, 3, 3, generator=g) / (9 * C) ** 0.5, torch.randn(Cout, generator=g)
    xg, wg, bg = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = mx_conv2d_train(xg, wg, bg, s, p, d, fx, fw, fg)
    assert y.shape == (B, Cout, 4, 3) and y.is_contiguous(memory_format=torch.channels_last)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    want = composed(x, w, b, dy, s, p, d, fx, fw, fg)
    for got, ref, name in zip((y, xg.grad, wg.grad, bg.grad), want, ("y", "dx", "dW", "db")):
        assert got.shape == ref.shape and torch.equal(got.detach(), ref), name
    # gradients nobody asks for are None
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        ts = [t.clone().requires_grad_(n) for t, n in zip((x, w, b), need)]
        mx_conv2d_train(*ts, s, p, d, fx, fw, fg).backward(dy)
        for t, n, ref in zip(ts, need, want[1:]):
            assert (t.grad is None) == (not n) and (not n or torch.equal(t.grad, ref))
    assert not mx_conv2d_train(x, w, b, s, p, d).requires_grad
    # stochastic rounding: the two forms of dy at step 7, the step advanced by one; y is the nearest mode's
    step = torch.tensor([7])
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ys = mx_conv2d_train(xg, wg, None, s, p, d, fx, fw, "mxfp4_e2m1", "stochastic", 21, step)
    ys.backward(dy)
    assert int(step) == 8
    want = composed(x, w, None, dy, s, p, d, fx, fw, "mxfp4_e2m1", "stochastic", 21, 7)
    assert torch.equal(ys.detach(), want[0]) and torch.equal(xg.grad, want[1]) and torch.equal(wg.grad, want[2])
    nearest = composed(x, w, None, dy, s, p, d, fx, fw, "mxfp4_e2m1")
    assert torch.equal(want[0], nearest[0]) and not torch.equal(want[1], nearest[1]) and not torch.equal(want[2], nearest[2])


def test_mxtrainconv2d():
    torch.manual_seed(6)
    conv = nn.Conv2d(32, 24, (3, 2), stride=(2, 1), padding=(1, 0), dilation=(1, 2))
    layer = MXTrainConv2d.from_conv(conv, w_fmt="mxfp4_e2m1")
    assert isinstance(layer, nn.Conv2d) and list(layer.state_dict()) == list(conv.state_dict()) == ["weight", "bias"]
    assert layer.weight is conv.weight and layer.bias is conv.bias and layer.weight.data_ptr() == conv.weight.data_ptr()
    assert not hasattr(layer, "sr_seed") and not hasattr(layer, "sr_step")
    assert "w_fmt='mxfp4_e2m1'" in repr(layer) and "x_fmt='mxfp8_e4m3'" in repr(layer) and "grad_fmt='mxfp8_e5m2'" in repr(layer)
    assert "wgrad_split_k" not in repr(layer) and "wgrad_split_k=4" in repr(MXTrainConv2d(4, 4, 3, wgrad_split_k=4))
    x = torch.randn(5, 32, 9, 8)
    y = layer(x)
    assert torch.equal(y, mx_conv2d_train(x, conv.weight, conv.bias, (2, 1), (1, 0), (1, 2), w_fmt="mxfp4_e2m1"))
    y.sum().backward()
    assert conv.weight.grad is not None and conv.weight.grad.shape == conv.weight.shape and conv.bias.grad is not None
    inf = layer.to_inference()
    assert isinstance(inf, MXConv2d) and inf.weight_fmt == "mxfp4_e2m1" and inf.act_fmt == "mxfp8_e4m3"
    with torch.no_grad():
        assert torch.equal(inf(x), layer(x))               # bit for bit: the same codes, the same product
    own = MXTrainConv2d(32, 24, 3, bias=False)
    assert list(own.state_dict()) == ["weight"] and own.bias is None and own(x).shape == (5, 24, 7, 6)
    sr = MXTrainConv2d(8, 8, 3, grad_rounding="stochastic", seed=5)
    assert sr.sr_seed == 5 and int(sr.sr_step) == 0 and list(sr.state_dict()) == ["weight", "bias"] and "stochastic" in repr(sr)
    sr(torch.randn(2, 8, 5, 5)).sum().backward()
    assert int(sr.sr_step) == 1
    shared = MXTrainConv2d.from_conv(nn.Conv2d(8, 8, 3), grad_rounding="stochastic")
    assert int(shared.sr_step) == 0 and isinstance(shared.sr_seed, int)
    # the refusals
    with pytest.raises(ValueError, match="supports groups == 1 only, the layer has groups=2"):
        MXTrainConv2d(8, 8, 3, groups=2)
    with pytest.raises(ValueError, match="supports zero padding only, the layer has padding_mode='reflect'"):
        MXTrainConv2d.from_conv(nn.Conv2d(8, 8, 3, padding=1, padding_mode="reflect"))
    with pytest.raises(ValueError, match="needs the padding as numbers, the layer has padding='same'"):
        MXTrainConv2d.from_conv(nn.Conv2d(8, 8, 3, padding="same"))
    with pytest.raises(TypeError, match="needs an nn.Conv2d"):
        MXTrainConv2d.from_conv(nn.Linear(3, 3))
    with pytest.raises(ValueError, match="unknown MX format"):
        MXTrainConv2d(8, 8, 3, grad_fmt="fp8")
    with pytest.raises(ValueError, match="wgrad_split_k"):
        MXTrainConv2d(8, 8, 3, wgrad_split_k="all")


def plan(M, N, K, S):
    slices, nbytes = ctypes.c_int32(-1), ctypes.c_uint64(1)
    st = _hip.load().qs_mx_conv2d_wgrad_plan(M, N, K, S, ctypes.byref(slices), ctypes.byref(nbytes))
    return st, slices.value, nbytes.value


def test_plan_without_a_gpu():
    for K, S in ((2304, 1), (2304, 2), (2304, 7), (2304, 18), (2304, 100), (5184, 3), (5184, 40), (130, 5)):
        steps = -(-K // 128)
        per = -(-steps // S)
        want = -(-steps // per)
        assert plan(136, 360, K, S) == (0, want, want * 136 * 360 * 4 if want > 1 else 0), (K, S)
        assert _hip.mx_conv_wgrad_plan(136, 360, K, S) == (want, want * 136 * 360 * 4 if want > 1 else 0)
    assert plan(64, 576, 31 * 128, 0)[:2] == (0, 1)                       # fewer than 32 steps: never split
    st, slices, nbytes = plan(64, 576, 9 * 9 * 64, 0)                    # B 64, 9 x 9 output, Cout 64, 3x3 x 64: 41 steps, 5 tiles
    assert st == 0 and 1 < slices <= 41 // 8 and nbytes == slices * 64 * 576 * 4
    assert plan(2048, 2048, 1 << 20, 0)[:2] == (0, 1)                    # 256 tiles: never split
    assert plan(0, 576, 4096, 0) == (0, 1, 0) and plan(64, 0, 4096, 4) == (0, 1, 0)
    for bad in ((-1, 8, 128, 1), (8, -1, 128, 1), (8, 8, -1, 1), (8, 8, 128, -1), (8, 8, 0, 1)):
        assert plan(*bad)[0] == -2, bad
    assert _hip.load().qs_mx_conv2d_wgrad_plan(8, 8, 256, 2, None, None) == 0


def test_entry_points_validate_without_a_gpu(tmp_path):
    lib = _hip.load()
    assert lib.qs_mx_conv2d_wgrad_v(None) == -2 and lib.qs_mx_conv2d_wgrad_route(None) == -2
    a = _hip.MxConv2dWgradArgs()
    a.struct_size = 2
    assert lib.qs_mx_conv2d_wgrad_route(ctypes.byref(a)) == -2

    def fresh(**over):
        a = _hip.MxConv2dWgradArgs()
        a.struct_size = ctypes.sizeof(a)
        a.dyt_codes, a.dyt_scales, a.xt_codes, a.xt_scales, a.dw = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
        a.B, a.H, a.W, a.C, a.Cout, a.OH, a.OW, a.KH, a.KW = 64, 9, 9, 64, 64, 9, 9, 3, 3
        a.stride_h = a.stride_w = a.dil_h = a.dil_w = a.pad_h = a.pad_w = 1
        a.split_k = 1
        for k, v in over.items():
            setattr(a, k, v)
        return a

    route = lambda **over: lib.qs_mx_conv2d_wgrad_route(ctypes.byref(fresh(**over)))
    assert route() == _hip.MX_CONV_ROUTE_VEC
    assert route(B=40, OH=9) == _hip.MX_CONV_ROUTE_PLAIN and route(xt_codes=0x3001) == _hip.MX_CONV_ROUTE_PLAIN
    assert route(dyt_codes=0x1008) == _hip.MX_CONV_ROUTE_PLAIN
    for null in ("dyt_codes", "dyt_scales", "xt_codes", "xt_scales", "dw"):
        assert route(**{null: None}) == -2, null
    for field, v in (("dy_format", 5), ("x_format", -1), ("B", 0), ("B", -1), ("Cout", -1), ("C", -1), ("H", 0), ("W", 0), ("KH", 0), ("KW", 0),
                     ("stride_h", 0), ("stride_w", 0), ("dil_h", 0), ("dil_w", 0), ("pad_h", -1), ("pad_w", -1), ("split_k", -1),
                     ("OH", 8), ("OW", 10), ("OH", 0), ("KH", 12), ("B", 2 ** 31), ("Cout", 2 ** 31), ("C", 2 ** 31), ("H", 2 ** 31),
                     ("pad_w", 2 ** 31 - 4)):
        assert route(**{field: v}) == -2, (field, v)
    assert route(ydt=7) == -1 and route(dw=0x5002) == -3 and route(dw=0x5002, ydt=1) == _hip.MX_CONV_ROUTE_VEC
    assert route(Cout=0) == 0 and route(C=0) == 0                        # an empty problem: nothing to do
    assert lib.qs_mx_conv2d_wgrad_v(ctypes.byref(fresh(Cout=0))) == 0
    assert route(Cout=0, B=0) == -2                                       # B == 0 is an error first
    # the workspace of a split product: 41 steps in 5 slices
    need = 5 * 64 * 576 * 4
    assert route(split_k=5) == -2                                         # NULL
    assert route(split_k=5, workspace=0x6008, workspace_bytes=need) == -3
    assert route(split_k=5, workspace=0x6000, workspace_bytes=need - 1) == -4
    assert route(split_k=5, workspace=0x6000, workspace_bytes=need) == _hip.MX_CONV_ROUTE_VEC
    # their precedence: NULL, then the alignment, then the size, then the grid of tiles x slices
    assert route(split_k=5, workspace_bytes=need - 1) == -2 and route(split_k=5, workspace=0x6008, workspace_bytes=need - 1) == -3
    big = dict(split_k=5, Cout=2 ** 21, C=2 ** 20, workspace=0x6000)      # 2^14 x 9 2^13 tiles fit a grid, five times as many do not
    assert route(**big, workspace_bytes=5 * 2 ** 21 * 9 * 2 ** 20 * 4 - 1) == -4 and route(**big, workspace_bytes=5 * 2 ** 21 * 9 * 2 ** 20 * 4) == -2
    assert route(split_k=0) == -2 and route(split_k=0, workspace=0x6000, workspace_bytes=need) == _hip.MX_CONV_ROUTE_VEC      # auto: <= 5 slices
    assert route(split_k=1, workspace=0x6008) == _hip.MX_CONV_ROUTE_VEC   # not looked at when S' == 1
    # 64-bit overflow of a product of extents; more work-groups than a grid holds
    assert route(H=2 ** 31 - 3, W=2 ** 31 - 3, OH=2 ** 31 - 3, OW=2 ** 31 - 3, Cout=2 ** 20, C=2 ** 20) == -2
    assert route(Cout=2 ** 31 - 1, C=2 ** 31 - 1) == -2
    # the struct layout against the header
    fields = [f for f, _ in _hip.MxConv2dWgradArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\nprintf("%%zu", sizeof(qs_mx_conv2d_wgrad_args));\n%s\nreturn 0; }\n'
                   % (os.path.join(ROOT, "include", "qsparse_hip.h"),
                      "\n".join(f'printf(" %zu", offsetof(qs_mx_conv2d_wgrad_args, {f}));' for f in fields)))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(src)], check=True)
    size, *offsets = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(_hip.MxConv2dWgradArgs)
    assert [int(o) for o in offsets] == [getattr(_hip.MxConv2dWgradArgs, f).offset for f in fields]
    assert fields[0] == "struct_size"
