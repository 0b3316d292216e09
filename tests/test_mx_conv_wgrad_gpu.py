"""The weight gradient of a convolution on MX codes on the GPU: the batch-blocked implicit-GEMM kernel (qs_mx_conv2d_wgrad_v) with the
route of every call asserted -- bit-identical to ``mx_matmul(..., split_k=S')`` on the host-gathered operands
(tests/mx_conv_wgrad_ref.py), S' read from ``_hip.mx_conv_wgrad_last_split``; the slicing, 0xFF scale bytes, the derived bound of
the float64 reference, ``mx_conv2d_train`` against its CPU path, the layer under autocast, stochastic rounding, a side stream and a
graph capture of a whole forward + backward.

The general-class bound is test_mx_conv_gpu.py's with K' = OH OW Bp as the contraction length:
|y32 - y64| <= 2 K' 2^-23 S + ulp_ydt(y64), S = the sum of the absolute products in float64.  A split sum adds its S' partials after
at most ceil(K' / 128 / S') steps each: fewer roundings than the K' the bound allows for."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mx_conv_wgrad_ref as R
import mx_gemm_ref as G
import mx_sr_ref as S
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_conv_train import MXTrainConv2d, mx_conv2d_train, mx_conv2d_weight_grad
from qsparse_amd.mx_gemm import mx_matmul, mx_quantize_2way
from qsparse_amd.quantize import quantize_with_mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
PAIRS = [("mxfp8_e5m2", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp6_e2m3", "mxfp8_e5m2"), ("mxfp8_e4m3", "mxfp4_e2m1"),
         ("mxfp6_e3m2", "mxfp6_e2m3")]
VEC, PLAIN = _hip.MX_CONV_ROUTE_VEC, _hip.MX_CONV_ROUTE_PLAIN
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# B, H, W, C, Cout, (KH, KW), stride, padding, dilation, route
MAIN = (48, 6, 6, 40, 136, (3, 3), 1, 1, 1, VEC)          # a partial batch block; M = 136 (two tiles), N = 360 (three, ragged); 18 steps
MAIN_PLAIN = (20, 6, 6, 40, 136, (3, 3), 1, 1, 1, PLAIN)
AUTO = (64, 9, 9, 64, 64, (3, 3), 1, 1, 1, VEC)           # 9 x 9 output: 41 steps (a partial last one), 5 tiles
GEOMETRIES = [
    (32, 8, 7, 16, 9, (3, 3), 2, 1, 1, VEC),              # stride 2 with a remainder row: (8 + 2 - 3) % 2 == 1
    (32, 7, 7, 16, 9, (3, 3), 1, 2, 2, VEC),              # dilation 2
    (48, 5, 4, 40, 17, (1, 1), 1, 0, 1, VEC),             # 1x1: still the implicit kernel
    (16, 6, 5, 8, 9, (5, 3), 1, (2, 0), 1, VEC),          # 5x3 with pad (2, 0)
    (16, 3, 3, 8, 9, (2, 2), 1, 3, 1, VEC),               # padding beyond the kernel's reach: output pixels of pure padding
    (40, 6, 6, 3, 20, (3, 3), 1, 1, 1, PLAIN),            # C = 3
    (32, 6, 6, 40, 1, (3, 3), 1, 1, 1, VEC),              # Cout = 1
]


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def offset_by_one(t):
    """the same bytes on the device at a base one byte past a 16-byte boundary (a slice of a larger allocation)"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() and view.is_contiguous()
    return view


def out_hw(case):
    B, H, W, C, Cout, (KH, KW), stride, padding, dilation, route = case
    (sh, sw), (ph, pw), (dh, dw) = R.pair(stride), R.pair(padding), R.pair(dilation)
    return R.out_size(H, KH, sh, ph, dh), R.out_size(W, KW, sw, pw, dw)


def wgrad(ops, fg, fx, route, ks, stride=1, padding=0, dilation=1, dt=torch.float32, split_k="auto"):
    dw = mx_conv2d_weight_grad(ops[0], ops[1], fg, ops[2], ops[3], fx, ks, stride, padding, dilation, dt, split_k)
    assert _hip.mx_conv_wgrad_last_route == route, (_hip.mx_conv_wgrad_last_route, route)
    assert dw.is_cuda and dw.dtype == dt and dw.is_contiguous()
    return dw


def batch_blocked(t, fmt):
    """the column pair of the two-way quantizer on a channels-last t [B, H, W, C] seen as [B, H W C]: codes [H, W, C, B]"""
    B, H, W, C = t.shape
    _, _, cc, cs = mx_quantize_2way(t.reshape(B, -1).to(DEV), None, fmt)
    return cc.view(H, W, C, B), cs.view(H, W, C, -1)


def quantized_case(g, case, fg, fx):
    """(dyt_codes, dyt_scales, xt_codes, xt_scales) as the GPU quantizer writes them, from randn tensors"""
    B, H, W, C, Cout = case[:5]
    OH, OW = out_hw(case)
    x, dy = torch.randn(B, H, W, C, generator=g), torch.randn(B, OH, OW, Cout, generator=g) / (B * OH * OW) ** 0.5
    return batch_blocked(dy, fg) + batch_blocked(x, fx)


def exact_case(g, case, fg, fx):
    """operands of the exact class for the contraction length K' = OH OW Bp (CPU tensors)"""
    B, H, W, C, Cout = case[:5]
    OH, OW = out_hw(case)
    Kp = OH * OW * (-(-B // 32) * 32)
    rg, rx = G.scale_windows(Kp, fg, fx)
    G.assert_exact_class(Kp, fg, fx, rg, rx)
    gc, gs = G.exact_operand(g, OH * OW * Cout, B, fg, rg)
    xc, xs = G.exact_operand(g, H * W * C, B, fx, rx)
    nb = xs.shape[-1]
    return gc.view(OH, OW, Cout, B), gs.view(OH, OW, Cout, nb), xc.view(H, W, C, B), xs.view(H, W, C, nb)


def expected_split(steps, S):
    per = -(-steps // S)
    return -(-steps // per)


def check_against_gathered(g, case, fg, fx, dtypes=(torch.float32,), shift=False, split_k="auto"):
    B, H, W, C, Cout, ks, stride, padding, dilation, route = case
    ops = quantized_case(g, case, fg, fx)
    Gc, SG, Xc, SX = R.gathered_codes(*ops, ks, stride, padding, dilation)
    if shift:                                              # code bases one byte past a 16-byte boundary: the byte-load kernel
        assert route == VEC
        ops, route = (offset_by_one(ops[0]), ops[1], offset_by_one(ops[2]), ops[3]), PLAIN
    for dt in dtypes:
        dw = wgrad(ops, fg, fx, route, ks, stride, padding, dilation, dt, split_k)
        slices = _hip.mx_conv_wgrad_last_split
        want = mx_matmul(Gc, SG, fg, Xc, SX, fx, None, dt, split_k=slices)
        assert _hip.mx_gemm_last_route == _hip.MX_GEMM_ROUTE_VEC and _hip.mx_gemm_last_split == slices     # K' % 32 == 0, fresh operands
        assert dw.shape == (Cout, ks[0], ks[1], C)
        assert G.same(dw.reshape(Cout, -1), want), (case, fg, fx, dt, shift, slices)
    return slices


@pytest.mark.parametrize("fg,fx", ALL_PAIRS)
def test_bit_identical_to_matmul_on_gathered_operands_every_format_pair(fg, fx):
    g = torch.Generator().manual_seed(200 + G.FMTS.index(fg) * 5 + G.FMTS.index(fx))
    check_against_gathered(g, MAIN, fg, fx)
    check_against_gathered(g, MAIN_PLAIN, fg, fx)
    check_against_gathered(g, MAIN, fg, fx, shift=True)


@pytest.mark.parametrize("fg,fx", PAIRS)
def test_bit_identical_in_every_output_dtype(fg, fx):
    g = torch.Generator().manual_seed(250 + G.FMTS.index(fg) * 5 + G.FMTS.index(fx))
    check_against_gathered(g, MAIN, fg, fx, DTYPES)
    check_against_gathered(g, MAIN, fg, fx, DTYPES, split_k=3)


@pytest.mark.parametrize("fg,fx", PAIRS)
def test_bit_identical_to_matmul_on_gathered_operands_every_geometry(fg, fx):
    g = torch.Generator().manual_seed(300 + G.FMTS.index(fg) * 5 + G.FMTS.index(fx))
    assert out_hw(GEOMETRIES[0]) == (4, 4) and out_hw(GEOMETRIES[4]) == (8, 8)
    for case in GEOMETRIES:
        check_against_gathered(g, case, fg, fx)
        check_against_gathered(g, case, fg, fx, split_k=2)


@pytest.mark.parametrize("split_k", [1, 2, 3, 7])
def test_requested_slices_follow_the_formula(split_k):
    g = torch.Generator().manual_seed(40 + split_k)
    for case, steps in ((MAIN, 6 * 6 * 64 // 128), (MAIN_PLAIN, 6 * 6 * 32 // 128)):        # Bp = 64: 18 steps; Bp = 32: 9
        got = check_against_gathered(g, case, "mxfp8_e5m2", "mxfp8_e4m3", DTYPES, split_k=split_k)
        assert got == expected_split(steps, split_k), (steps, got)
    assert expected_split(18, 7) == 6 and expected_split(9, 7) == 5                         # 7 divides neither


def test_auto_splits_a_long_contraction_over_few_tiles():
    g = torch.Generator().manual_seed(41)
    assert out_hw(AUTO) == (9, 9)
    got = check_against_gathered(g, AUTO, "mxfp8_e5m2", "mxfp8_e4m3", DTYPES)
    assert got > 1
    assert check_against_gathered(g, MAIN, "mxfp8_e5m2", "mxfp8_e4m3") == 1          # 18 steps: fewer than 32, never split


def test_two_runs_give_the_same_bits():
    g = torch.Generator().manual_seed(42)
    ops = quantized_case(g, AUTO, "mxfp4_e2m1", "mxfp8_e4m3")
    a = wgrad(ops, "mxfp4_e2m1", "mxfp8_e4m3", VEC, (3, 3), 1, 1, 1)
    assert _hip.mx_conv_wgrad_last_split > 1
    b = wgrad(ops, "mxfp4_e2m1", "mxfp8_e4m3", VEC, (3, 3), 1, 1, 1)
    assert G.same(a, b)


@pytest.mark.parametrize("fg,fx", PAIRS)
def test_ff_scale_bytes_give_nan_exactly_where_the_definition_says(fg, fx):
    g = torch.Generator().manual_seed(7)
    # B, H, W, C, Cout; 3x3, stride 2, padding 1: the corner pixel (0, 0) is read through tap (1, 1) only
    for case in ((64, 5, 6, 8, 130, (3, 3), 2, 1, 1, VEC), (40, 5, 6, 8, 20, (3, 3), 2, 1, 1, PLAIN)):
        B, H, W, C, Cout, ks, stride, padding, dilation, route = case
        base = exact_case(g, case, fg, fx)
        reads = R.taps_reading(H, W, 3, 3, stride, padding, dilation)                 # [H, W, KH, KW]
        for which, split_k in (("x", 1), ("x", 2), ("dy", 1), ("dy", 3)):
            gc, gs, xc, xs = (t.clone() for t in base)
            nan = torch.zeros(Cout, 3, 3, C, dtype=torch.bool)
            if which == "x":                                                          # block 1 of the batch at pixel (2, 3), channel 5
                ih, iw, c, blk = 2, 3, 5, 1
                xs[ih, iw, c, blk] = 255
                xc[ih, iw, c, 32 * blk:] = 0                                          # (as the quantizer writes such a block)
                nan[:, :, :, c] = reads[ih, iw]
                assert 0 < int(reads[ih, iw].sum()) < 9
            else:                                                                     # channel 7 at one output pixel: dW[7] everywhere
                gs[1, 2, 7, 0] = 255
                gc[1, 2, 7, :32] = 0
                nan[7] = True
            dw = wgrad(tuple(t.to(DEV) for t in (gc, gs, xc, xs)), fg, fx, route, ks, stride, padding, dilation, split_k=split_k)
            assert torch.equal(dw.isnan().cpu(), nan), (which, split_k)
            # everything else is still the float64 weight gradient
            clean = R.wgrad64(torch.nan_to_num(G.values(gc, gs, fg)), torch.nan_to_num(G.values(xc, xs, fx)), ks, stride, padding, dilation)
            assert torch.equal(dw.cpu().double()[~nan], clean[~nan]), (which, split_k)
    assert reads[0, 0].nonzero().tolist() == [[1, 1]]


@pytest.mark.parametrize("fg,fx", PAIRS)
def test_general_class_within_the_derived_bound(fg, fx):
    g = torch.Generator().manual_seed(500 + G.FMTS.index(fg) * 5 + G.FMTS.index(fx))
    case = (48, 9, 8, 40, 72, (3, 3), 2, 1, 1, VEC)                       # 5 x 4 output, K' = 20 * 64 = 1280
    ks, geom = case[5], case[6:9]
    Kp = 5 * 4 * 64
    dev = quantized_case(g, case, fg, fx)
    gv, xv = G.values(dev[0], dev[1], fg), G.values(dev[2], dev[3], fx)
    y64, S_ = R.wgrad64(gv, xv, ks, *geom), R.wgrad64(gv.abs(), xv.abs(), ks, *geom)
    for dt, split_k in ((torch.float32, 1), (torch.bfloat16, 1), (torch.float32, 4), (torch.float16, "auto")):
        dw = wgrad(dev, fg, fx, VEC, ks, *geom, dt, split_k)
        ok, ratio = G.within(dw, y64, 2 * Kp * 2.0 ** -23 * S_ + G.ulp(y64, dt))
        print(fg, fx, dt, split_k, "largest |err| / bound", ratio)
        assert ok, (dt, split_k, ratio)


def float64_step(x, w, bias, dy, geom, fx, fw, fg):
    """(y, dx, dW, S_y, S_dx, S_dW) of the definition of mx_conv2d_train in float64 on the CPU, from the public quantizers' codes:
    NCHW value tensors, S the sums of the absolute products"""
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous()
    nchw = lambda v: v.permute(0, 3, 1, 2)
    val = lambda t, f, dim: G.values(*(u.movedim(dim, -1) for u in quantize_with_mx(t, f, dim, return_codes=True)[1:]), f).movedim(-1, dim)
    xl, dyl, wl = cl(x.float().cpu()), cl(dy.float().cpu()), cl(w.float().cpu())
    x_c, x_b = nchw(val(xl, fx, 3)), nchw(val(xl, fx, 0))
    g_n, g_b = nchw(val(dyl, fg, 3)), nchw(val(dyl, fg, 0))
    w_c, w_n = nchw(val(wl, fw, 3)), nchw(val(wl, fw, 0))
    conv = lambda a, b: F.conv2d(a, b, None, *geom)
    out = []
    for f in (lambda t: t, torch.abs):
        xv = f(x_c).clone().requires_grad_(True)
        wv = torch.zeros_like(w_c).requires_grad_(True)
        y = conv(f(x_c), f(w_c))
        dx = torch.autograd.grad(conv(xv, f(w_n)), xv, f(g_n))[0]
        dw = torch.autograd.grad(conv(f(x_b), wv), wv, f(g_b))[0]
        out += [y, dx, dw]
    out[0] = out[0] + bias.double().cpu().view(1, -1, 1, 1)
    return out


@pytest.mark.parametrize("fx,fw,fg", [("mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp4_e2m1", "mxfp4_e2m1", "mxfp4_e2m1"),
                                      ("mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e3m2")])
def test_mx_conv2d_train_on_the_gpu_against_the_cpu(fx, fw, fg):
    g = torch.Generator().manual_seed(600)
    # (B, C, Cout, H, W, k, stride, padding, dilation, channels_last, dtype): multiples of 32 (one two-way call) and not
    for B, C, Cout, H, W, k, s, p, d, cl, dtype in ((48, 32, 64, 9, 8, 3, 2, 1, 1, True, torch.float32),
                                                    (40, 20, 36, 7, 7, 3, 1, 1, 1, False, torch.bfloat16),
                                                    (33, 3, 5, 8, 8, (5, 3), 1, (2, 0), 2, True, torch.float32)):
        geom = (R.pair(s), R.pair(p), R.pair(d))
        KH, KW = R.pair(k)
        x = (torch.randn(B, C, H, W, generator=g) * 2).to(dtype)
        w = torch.randn(Cout, C, KH, KW, generator=g) / (C * KH * KW) ** 0.5
        bias = torch.randn(Cout, generator=g)
        OH, OW = R.out_size(H, KH, geom[0][0], geom[1][0], geom[2][0]), R.out_size(W, KW, geom[0][1], geom[1][1], geom[2][1])
        dy = (torch.randn(B, Cout, OH, OW, generator=g) / (OH * OW)).to(dtype)
        res = {}
        for dev in ("cpu", DEV):
            xin = x.clone().to(dev).contiguous(memory_format=torch.channels_last) if cl else x.clone().to(dev).contiguous()
            xin.requires_grad_(True)                                     # (clones: on the CPU `.to` hands back the tensor itself)
            wd, bd = w.clone().to(dev).requires_grad_(True), bias.clone().to(dev).requires_grad_(True)
            y = mx_conv2d_train(xin, wd, bd, s, p, d, fx, fw, fg)
            assert y.shape == (B, Cout, OH, OW) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
            y.backward(dy.to(dev))
            assert xin.grad.dtype == dtype and wd.grad.dtype == torch.float32 and wd.grad.shape == w.shape
            res[dev] = (y.detach(), xin.grad, wd.grad, bd.grad)
        assert _hip.mx_conv_wgrad_last_route == (VEC if B % 16 == 0 else PLAIN)
        y64, dx64, dw64, Sy, Sdx, Sdw = float64_step(x, w, bias, dy, geom, fx, fw, fg)
        pad32 = lambda n: -(-n // 32) * 32
        terms = (KH * KW * pad32(C), KH * KW * pad32(Cout), OH * OW * pad32(B))
        for name, i, ref, S_, K_, dt in (("y", 0, y64, Sy, terms[0], dtype), ("dx", 1, dx64, Sdx, terms[1], dtype),
                                         ("dW", 2, dw64, Sdw, terms[2], torch.float32)):
            bound = 2 * K_ * 2.0 ** -23 * S_ + G.ulp(ref, dt) + (2.0 ** -23 * bias.abs().double().view(1, -1, 1, 1) if i == 0 else 0)
            ok, ratio = G.within(res[DEV][i], ref, bound)
            print(fx, fw, fg, (B, C, Cout), name, "largest |err| / bound", ratio)
            assert ok, (name, ratio)
            assert G.within(res["cpu"][i], ref, bound)[0], name
        assert torch.allclose(res[DEV][3].cpu(), dy.float().sum((0, 2, 3)), rtol=1e-5, atol=1e-6)
        assert torch.allclose(res["cpu"][3], dy.float().sum((0, 2, 3)), rtol=1e-5, atol=1e-6)


def test_mxtrainconv2d_forward_and_backward_under_bf16_autocast():
    torch.manual_seed(3)
    layer = MXTrainConv2d(32, 48, 3, stride=1, padding=1, w_fmt="mxfp4_e2m1").to(DEV)
    x = torch.randn(32, 32, 7, 7, device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = layer(x)
    assert y.dtype == torch.bfloat16 and y.shape == (32, 48, 7, 7) and y.is_contiguous(memory_format=torch.channels_last)
    dy = torch.randn_like(y)
    y.backward(dy)
    assert x.grad.dtype == torch.float32 and layer.weight.grad.dtype == torch.float32 and layer.bias.grad.dtype == torch.float32
    # the same call on the cast input, outside autocast
    xb = x.detach().bfloat16().requires_grad_(True)
    w2, b2 = layer.weight.detach().clone().requires_grad_(True), layer.bias.detach().clone().requires_grad_(True)
    y2 = mx_conv2d_train(xb, w2, b2, 1, 1, 1, "mxfp8_e4m3", "mxfp4_e2m1", "mxfp8_e5m2")
    y2.backward(dy)
    assert torch.equal(y, y2) and torch.equal(x.grad, xb.grad.float()) and torch.equal(layer.weight.grad, w2.grad)
    assert torch.equal(layer.bias.grad, b2.grad)
    ref = F.conv2d(x.detach(), layer.weight.detach(), layer.bias.detach(), 1, 1)
    assert float((y.float() - ref).norm() / ref.norm()) < 0.2                     # FP4 weights: the quantization error, not the kernel's
    inf = layer.to_inference(out_dtype=torch.bfloat16)
    with torch.no_grad():
        assert torch.equal(inf(xb.detach()), y)


@pytest.mark.parametrize("Cout", [32, 20])
def test_stochastic_rounding_rounds_the_two_forms_of_dy_and_nothing_else(Cout):
    FX, FW, FG, seed = "mxfp8_e4m3", "mxfp8_e4m3", "mxfp4_e2m1", 1234
    g = torch.Generator().manual_seed(0)
    B, C, H, W = 16, 8, 5, 4
    x = (torch.randn(B, C, H, W, generator=g) * 2).to(DEV)
    w = (torch.randn(Cout, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(DEV)
    dy = (torch.randn(B, Cout, H, W, generator=g) / Cout).to(DEV)
    step = torch.tensor([3], device=DEV)
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = mx_conv2d_train(xg, wg, None, 1, 1, 1, FX, FW, FG, "stochastic", seed, step)
    y.backward(dy)
    assert int(step) == 4
    xn, wn = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yn = mx_conv2d_train(xn, wn, None, 1, 1, 1, FX, FW, FG)
    yn.backward(dy)
    assert torch.equal(y, yn) and not torch.equal(xg.grad, xn.grad) and not torch.equal(wg.grad, wn.grad)
    # the codes of dy: the Cout form on stream 0, the B form on stream 1, at step 3 -- the element-by-element reference's
    dyl = dy.permute(0, 2, 3, 1).contiguous().cpu()
    _, r_codes, r_scales = S.reference(dyl, FG, -1, torch.float32, seed, 3, 0)
    _, c_codes, c_scales = S.reference(dyl.reshape(B, -1).t().contiguous(), FG, -1, torch.float32, seed, 3, 1)
    c_codes, c_scales = c_codes.view(H, W, Cout, B), c_scales.view(H, W, Cout, -1)
    from qsparse_amd.mx_conv_transpose import mx_conv2d_input_grad
    with torch.no_grad():
        wt = quantize_with_mx(w.permute(1, 2, 3, 0).contiguous(), FW, -1, return_codes=True)[1:]
        xt = batch_blocked(x.permute(0, 2, 3, 1).contiguous().cpu(), FX)
    dx = mx_conv2d_input_grad(r_codes.to(DEV), r_scales.to(DEV), FG, wt[0], wt[1], FW, (H, W), 1, 1, 1)
    dw = mx_conv2d_weight_grad(c_codes.to(DEV), c_scales.to(DEV), FG, xt[0], xt[1], FX, (3, 3), 1, 1, 1)
    assert torch.equal(xg.grad, dx.permute(0, 3, 1, 2)) and torch.equal(wg.grad, dw.permute(0, 3, 1, 2))


def test_non_default_stream():
    g = torch.Generator().manual_seed(5)
    fg, fx = "mxfp8_e4m3", "mxfp4_e2m1"
    for split_k in (1, 3):
        ops = exact_case(g, MAIN, fg, fx)
        dev = tuple(t.to(DEV) for t in ops)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dw = wgrad(dev, fg, fx, VEC, (3, 3), 1, 1, 1, split_k=split_k)
        s.synchronize()
        assert G.same(dw, R.wgrad64(G.values(ops[0], ops[1], fg), G.values(ops[2], ops[3], fx), (3, 3), 1, 1, 1).float())


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
def test_graph_capture_of_a_whole_step_replays(rounding):
    """forward + backward of one MXTrainConv2d under torch.cuda.graph (a single layer: no parallel branches): nearest rounding
    replays bit for bit; with stochastic rounding the captured add_ advances the step and two replays differ"""
    g = torch.Generator().manual_seed(11)
    B, C, Cout = 64, 32, 64
    xs_ = [torch.randn(B, C, 9, 9, generator=g).bfloat16().to(DEV).contiguous(memory_format=torch.channels_last) for _ in range(2)]
    t = torch.randn(B, Cout, 9, 9, generator=g).bfloat16().to(DEV)
    torch.manual_seed(0)
    init = MXTrainConv2d(C, Cout, 3, padding=1, grad_fmt="mxfp4_e2m1", grad_rounding=rounding, seed=99).to(DEV)

    def step(layer, x):
        xin = x.detach().requires_grad_(True)
        y = layer(xin)
        for p in layer.parameters():
            p.grad = None
        y.backward(((y - t) / y.numel()).detach())
        return y.detach(), xin.grad

    layer = copy.deepcopy(init)
    static_x = xs_[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(layer, static_x)
    torch.cuda.current_stream().wait_stream(side)
    assert _hip.mx_conv_wgrad_last_split > 1               # 9 x 9 x 64: 41 steps, the split product and its workspace are captured
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                          # (a host synchronisation or a foreign allocation on the path would fail the capture)
        static_y, static_dx = step(layer, static_x)
    grads = []
    for i, x in enumerate(xs_ + xs_[:1]):
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eager = copy.deepcopy(init)
        if rounding == "stochastic":
            assert int(layer.sr_step) == 2 + i             # the warm-up plus the replays
            eager.sr_step.fill_(1 + i)
        y, dx = step(eager, x)
        assert torch.equal(static_y, y) and torch.equal(static_dx, dx) and torch.equal(layer.weight.grad, eager.weight.grad), i
        assert torch.equal(layer.bias.grad, eager.bias.grad)
        grads.append(layer.weight.grad.clone())
    assert torch.equal(grads[0], grads[2]) == (rounding == "nearest")      # the same input twice
