"""Transposed convolutions on MX codes on the GPU: the fractionally-strided implicit-GEMM kernel (qs_mx_conv_transpose2d_v) with the
route of every call asserted -- bit-identical to ``mx_matmul`` on the host-gathered operands (tests/mx_conv_transpose_ref.py), the
outputs no tap reaches, 0xFF scale bytes, quantizer-produced operands and the input gradient of a convolution within the derived
bound of the float64 reference, the layer, a side stream and a graph capture.

The general-class bound is test_mx_conv_gpu.py's with K' = KH KW Cp as the contraction length:
|y32 - y64| <= 2 K' 2^-23 S + ulp_ydt(y64) (+ 2^-23 |bias|), S = the sum of the absolute products in float64; used for K' >= 512."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mx_conv_transpose_ref as T
import mx_gemm_ref as G
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_conv_transpose import MXConvTranspose2d, mx_conv2d_input_grad, mx_conv_transpose2d
from qsparse_amd.mx_gemm import mx_matmul
from qsparse_amd.quantize import MXQuantizer, quantize_with_mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
PAIRS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp6_e2m3", "mxfp8_e5m2"), ("mxfp8_e4m3", "mxfp4_e2m1"),
         ("mxfp6_e3m2", "mxfp8_e4m3")]
GEMM, VEC, PLAIN = _hip.MX_CONV_ROUTE_GEMM, _hip.MX_CONV_ROUTE_VEC, _hip.MX_CONV_ROUTE_PLAIN
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# B, H, W, C, Cout, (KH, KW), stride, padding, output_padding, dilation, route
MAIN = (2, 5, 4, 48, 40, (3, 3), 2, 1, 1, 1, VEC)         # 10 x 8: M = 160 (two M tiles), K' = 576 (a partial last step)
MAIN_PLAIN = (2, 5, 4, 20, 40, (3, 3), 2, 1, 1, 1, PLAIN)
GEOMETRIES = [
    (2, 4, 3, 48, 17, (3, 2), (2, 3), (1, 0), 0, (2, 1), VEC),         # unequal strides and dilations
    (2, 6, 6, 32, 20, (3, 3), 2, 3, 0, 1, VEC),                        # p > d (k - 1): a crop, 7 x 7
    (2, 4, 5, 64, 9, (1, 3), 2, (0, 1), 0, 1, VEC),                    # KH == 1
    (2, 5, 4, 40, 9, (3, 1), 2, (1, 0), 0, 1, PLAIN),                  # KW == 1
    (2, 9, 7, 64, 17, (1, 1), 2, 0, 0, 1, VEC),                        # 1x1 with holes: not the GEMM route
    (3, 1, 1, 160, 130, (3, 3), 2, 0, 0, 1, VEC),                      # H == W == 1; Cp = 160: a 128-step straddles taps
    (2, 3, 4, 16, 33, (2, 2), (3, 2), 0, (2, 1), 1, VEC),              # op == s - 1
    (2, 5, 4, 3, 6, (3, 3), 2, 1, 1, 1, PLAIN),
    (2, 9, 7, 64, 17, (1, 1), 1, 0, 0, 1, GEMM),
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


def convt(ops, fx, fw, route, bias=None, stride=1, padding=0, out_pad=0, dilation=1, dt=torch.float32):
    y = mx_conv_transpose2d(ops[0], ops[1], fx, ops[2], ops[3], fw, bias, stride, padding, out_pad, dilation, dt)
    assert _hip.mx_conv_transpose_last_route == route, (_hip.mx_conv_transpose_last_route, route)
    assert y.is_cuda and y.dtype == dt and y.is_contiguous()
    return y


def quantized_case(g, B, H, W, C, Cout, KH, KW, fx, fw):
    """codes and scales as the GPU quantizer writes them, from randn activations and randn / sqrt(fan_in) weights"""
    x, w = torch.randn(B, H, W, C, generator=g), torch.randn(Cout, KH, KW, C, generator=g) / (KH * KW * C) ** 0.5
    _, xc, xs = quantize_with_mx(x.to(DEV), fx, -1, return_codes=True)
    _, wc, ws = quantize_with_mx(w.to(DEV), fw, -1, return_codes=True)
    return xc, xs, wc, ws


def exact_case(g, B, H, W, C, Cout, KH, KW, fx, fw):
    """operands of the exact class for the contraction length K' = KH KW Cp (CPU tensors)"""
    Kp = KH * KW * (-(-C // 32) * 32)
    rx, rw = G.scale_windows(Kp, fx, fw)
    G.assert_exact_class(Kp, fx, fw, rx, rw)
    xc, xs = G.exact_operand(g, B * H * W, C, fx, rx)
    wc, ws = G.exact_operand(g, Cout * KH * KW, C, fw, rw)
    nb = xs.shape[-1]
    return xc.view(B, H, W, C), xs.view(B, H, W, nb), wc.view(Cout, KH, KW, C), ws.view(Cout, KH, KW, nb)


def reached(n, k, s, p, d, op):
    """[out, n] bool, written as the scatter of the definition (independent of the helper's gather): input position i of the axis
    feeds output position i s - p + j d for every tap j"""
    out = torch.zeros(T.out_size(n, k, s, p, d, op), n, dtype=torch.bool)
    for i in range(n):
        for j in range(k):
            o = i * s - p + j * d
            if 0 <= o < out.shape[0]:
                out[o, i] = True
    return out


def check_against_gathered(g, case, fx, fw, dtypes=DTYPES, shift=False):
    B, H, W, C, Cout, (KH, KW), stride, padding, out_pad, dilation, route = case
    ops = quantized_case(g, B, H, W, C, Cout, KH, KW, fx, fw)
    A, SA, Wp, SWp = T.gathered_codes(*ops, stride, padding, out_pad, dilation)
    if shift:                                              # code bases one byte past a 16-byte boundary: the byte-load kernel
        assert route == VEC
        ops, route = (offset_by_one(ops[0]), ops[1], offset_by_one(ops[2]), ops[3]), PLAIN
    bias = torch.randn(Cout, generator=g).to(DEV)
    (sh, sw), (ph, pw), (oph, opw), (dh, dw) = T.pair(stride), T.pair(padding), T.pair(out_pad), T.pair(dilation)
    shape = (B, T.out_size(H, KH, sh, ph, dh, oph), T.out_size(W, KW, sw, pw, dw, opw), Cout)
    for dt in dtypes:
        for b in (None, bias):
            y = convt(ops, fx, fw, route, b, stride, padding, out_pad, dilation, dt)
            want = mx_matmul(A, SA, fx, Wp, SWp, fw, b, dt)
            assert _hip.mx_gemm_last_route == _hip.MX_GEMM_ROUTE_VEC and _hip.mx_gemm_last_split == 1      # K' % 32 == 0, fresh operands
            assert y.shape == shape
            assert G.same(y.reshape(-1, Cout), want), (case, fx, fw, dt, b is not None, shift)


@pytest.mark.parametrize("fx,fw", ALL_PAIRS)
def test_bit_identical_to_matmul_on_gathered_operands_every_format_pair(fx, fw):
    g = torch.Generator().manual_seed(200 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    assert T.out_size(5, 3, 2, 1, 1, 1) == 10 and T.out_size(4, 3, 2, 1, 1, 1) == 8
    check_against_gathered(g, MAIN, fx, fw)
    check_against_gathered(g, MAIN_PLAIN, fx, fw)
    check_against_gathered(g, MAIN, fx, fw, shift=True)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_bit_identical_to_matmul_on_gathered_operands_every_geometry(fx, fw):
    g = torch.Generator().manual_seed(300 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    assert T.out_size(6, 3, 2, 3, 1, 0) == 7
    for case in GEOMETRIES:
        check_against_gathered(g, case, fx, fw)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_outputs_that_no_tap_reaches_are_the_bias_or_plus_zero(fx, fw):
    """a stride larger than the kernel (k = 2, s = 3, p = 0): every third row and column of y has no tap"""
    g = torch.Generator().manual_seed(8)
    for C, route in ((32, VEC), (20, PLAIN)):
        B, H, W, Cout = 2, 4, 3, 9
        ops = exact_case(g, B, H, W, C, Cout, 2, 2, fx, fw)
        dev = tuple(t.to(DEV) for t in ops)
        bias = torch.randint(1, 16, (Cout,), generator=g).float() * torch.tensor([1.0, -1.0, 1.0] * 3)
        hit = reached(H, 2, 3, 0, 1, 0).any(1).view(-1, 1) & reached(W, 2, 3, 0, 1, 0).any(1).view(1, -1)      # [OH, OW]
        assert hit.shape == (11, 8) and int((~hit).sum()) == 11 * 8 - 8 * 6
        for dt in DTYPES:
            y0, yb = convt(dev, fx, fw, route, None, 3, 0, 0, 1, dt).cpu(), convt(dev, fx, fw, route, bias.to(DEV), 3, 0, 0, 1, dt).cpu()
            assert bool((y0[:, ~hit] == 0).all()) and not bool(torch.signbit(y0[:, ~hit]).any())          # +0.0
            assert torch.equal(yb[:, ~hit], bias.to(dt).expand(B, int((~hit).sum()), Cout))
            y64 = T.conv_transpose64(G.values(ops[0], ops[1], fx), G.values(ops[2], ops[3], fw), bias, 3, 0, 0, 1)
            assert G.same(yb, y64.to(dt))                                                                 # the rest: the exact class


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_ff_scale_bytes_give_nan_exactly_where_a_tap_reads_them(fx, fw):
    g = torch.Generator().manual_seed(7)
    for B, H, W, C, Cout, route in ((2, 5, 4, 64, 130, VEC), (2, 4, 5, 40, 20, PLAIN)):
        stride, padding, out_pad = (2, 3), (1, 2), (1, 0)
        pb, ph_, pw_, blk = 1, 3, 1, 1                                    # the activation block: pixel (1, 3, 1), channels 32..
        base = exact_case(g, B, H, W, C, Cout, 3, 3, fx, fw)
        rh, rw = reached(H, 3, 2, 1, 1, 1), reached(W, 3, 3, 2, 1, 0)     # [OH, H], [OW, W]
        for which in ("x", "w"):
            xc, xs, wc, ws = (t.clone() for t in base)
            nan = torch.zeros(B, rh.shape[0], rw.shape[0], Cout, dtype=torch.bool)
            if which == "x":                                              # exactly the outputs with an existing tap on that pixel
                xs[pb, ph_, pw_, blk] = 255
                xc[pb, ph_, pw_, 32 * blk:] = 0                           # (as the quantizer writes such a block)
                nan[pb] = (rh[:, ph_].view(-1, 1) & rw[:, pw_].view(1, -1)).unsqueeze(-1)
                assert 0 < int(nan[pb, ..., 0].sum()) < nan[pb, ..., 0].numel()
            else:                                                         # channel n at every output pixel, also where no tap exists
                ws[7, 2, 0, 0] = 255
                wc[7, 2, 0, :32] = 0
                nan[..., 7] = True
                at = T.taps_exist(H, W, 3, 3, stride, padding, out_pad, 1)[:, :, 2, 0]
                assert 0 < int(at.sum()) < at.numel()                     # at most pixels that tap does not exist: the block meets zero codes
            y = convt(tuple(t.to(DEV) for t in (xc, xs, wc, ws)), fx, fw, route, None, stride, padding, out_pad, 1)
            assert torch.equal(y.isnan().cpu(), nan), which
            # everything else is still the float64 transposed convolution
            clean = T.conv_transpose64(torch.nan_to_num(G.values(xc, xs, fx)), torch.nan_to_num(G.values(wc, ws, fw)), None, stride,
                                       padding, out_pad, 1)
            assert torch.equal(y.cpu().double()[~nan], clean[~nan]), which


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_general_class_within_the_derived_bound(fx, fw):
    g = torch.Generator().manual_seed(500 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    B, H, W, C, Cout, KH, KW = 2, 5, 4, 96, 40, 3, 3                      # K' = 9 * 96 = 864
    geom = (2, 1, 1, 1)
    dev = quantized_case(g, B, H, W, C, Cout, KH, KW, fx, fw)
    xv, wv = G.values(dev[0], dev[1], fx), G.values(dev[2], dev[3], fw)
    bias = torch.randn(Cout, generator=g)
    S = T.conv_transpose64(xv.abs(), wv.abs(), None, *geom)
    for dt, b in ((torch.float32, None), (torch.bfloat16, bias), (torch.float32, bias), (torch.float16, None)):
        y64 = T.conv_transpose64(xv, wv, b, *geom)
        y = convt(dev, fx, fw, VEC, None if b is None else b.to(DEV), *geom, dt)
        bound = 2 * KH * KW * C * 2.0 ** -23 * S + G.ulp(y64, dt) + (0 if b is None else 2.0 ** -23 * b.abs().double())
        ok, ratio = G.within(y, y64, bound)
        print(fx, fw, dt, "largest |err| / bound", ratio)
        assert ok, (dt, ratio)


@pytest.mark.parametrize("fy,fw", PAIRS)
def test_input_grad_of_a_convolution(fy, fw):
    """x [2, 8, 8, 32], Cout = 96, 3x3, s = 2, p = 1: dy is 4 x 4, the derived output padding 1, K' = 864"""
    g = torch.Generator().manual_seed(600 + G.FMTS.index(fy) * 5 + G.FMTS.index(fw))
    B, H, W, Cin, Cout, K = 2, 8, 8, 32, 96, 3
    dy, w = torch.randn(B, 4, 4, Cout, generator=g), torch.randn(Cin, K, K, Cout, generator=g) / (K * K * Cout) ** 0.5
    _, dyc, dys = quantize_with_mx(dy.to(DEV), fy, -1, return_codes=True)
    _, wtc, wts = quantize_with_mx(w.to(DEV), fw, -1, return_codes=True)
    dyv, wv = G.values(dyc, dys, fy), G.values(wtc, wts, fw)               # float64, on the CPU
    x = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, wv.permute(3, 0, 1, 2), None, 2, 1)
    assert y.shape == (B, Cout, 4, 4)
    dx64 = torch.autograd.grad(y, x, dyv.permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
    S = torch.autograd.grad(F.conv2d(x, wv.abs().permute(3, 0, 1, 2), None, 2, 1), x, dyv.abs().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
    for dt in DTYPES:
        dx = mx_conv2d_input_grad(dyc, dys, fy, wtc, wts, fw, (H, W), 2, 1, 1, dt)
        assert _hip.mx_conv_transpose_last_route == VEC and dx.shape == (B, H, W, Cin) and dx.dtype == dt
        ok, ratio = G.within(dx, dx64, 2 * K * K * Cout * 2.0 ** -23 * S + G.ulp(dx64, dt))
        print(fy, fw, dt, "largest |err| / bound", ratio)
        assert ok, (dt, ratio)
        assert G.same(dx, convt((dyc, dys, wtc, wts), fy, fw, VEC, None, 2, 1, 1, 1, dt))
    with pytest.raises(ValueError, match="not the gradient"):
        mx_conv2d_input_grad(dyc, dys, fy, wtc, wts, fw, (9, 8), 2, 1)


@pytest.mark.parametrize("wfmt,afmt", [("mxfp4_e2m1", "mxfp8_e4m3"), ("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4_e2m1")])
def test_mxconvtranspose2d_on_the_gpu_against_the_cpu(wfmt, afmt):
    torch.manual_seed(2)
    C, Cout = 64, 24
    layer = qs.quantize(nn.ConvTranspose2d(C, Cout, 3, stride=2, padding=1, output_padding=1), bits=G.WIDTH[wfmt], timeout=1,
                        callback=MXQuantizer(wfmt, block_dim=0)).train()
    layer(torch.randn(2, C, 5, 4)), layer(torch.randn(2, C, 5, 4))
    cpu = MXConvTranspose2d.from_quantized(layer.eval(), afmt)
    gpu = MXConvTranspose2d.from_quantized(layer, afmt).to(DEV)
    assert gpu.weight_codes.is_cuda and torch.equal(gpu.weight_codes.cpu(), cpu.weight_codes) and torch.equal(gpu.weight_scales.cpu(), cpu.weight_scales)
    exported = MXConvTranspose2d.from_exported(qs.export_integer(nn.Sequential(layer))["0"].weight, layer.bias.detach(), 2, 1, 1, 1, afmt)
    for name in ("weight_codes", "weight_scales", "bias"):
        assert torch.equal(getattr(exported, name), getattr(cpu, name)), name
    x = torch.randn(3, C, 5, 4) * 2
    Kp = 9 * C                                                           # 576
    for xin, od in ((x.bfloat16().contiguous(memory_format=torch.channels_last), torch.bfloat16), (x, torch.float32)):
        gpu.out_dtype = cpu.out_dtype = od
        yg = gpu(xin.to(DEV))
        assert _hip.mx_conv_transpose_last_route == VEC and yg.shape == (3, Cout, 10, 8) and yg.dtype == od and not yg.requires_grad
        assert yg.is_contiguous(memory_format=torch.channels_last)
        _, xc, xs = quantize_with_mx(xin.permute(0, 2, 3, 1), afmt, -1, return_codes=True)
        xv, wv = G.values(xc.contiguous(), xs.contiguous(), afmt), G.values(cpu.weight_codes, cpu.weight_scales, wfmt)
        y64 = T.conv_transpose64(xv, wv, cpu.bias, 2, 1, 1, 1)
        S = T.conv_transpose64(xv.abs(), wv.abs(), None, 2, 1, 1, 1)
        bound = 2 * Kp * 2.0 ** -23 * S + G.ulp(y64, od) + 2.0 ** -23 * cpu.bias.abs().double()
        ok, ratio = G.within(yg.permute(0, 2, 3, 1), y64, bound)
        print(wfmt, afmt, od, "largest |err| / bound", ratio)
        assert ok and G.within(cpu(xin).permute(0, 2, 3, 1), y64, bound)[0]
    from_gpu_layer = MXConvTranspose2d.from_quantized(layer.to(DEV), afmt)                               # built on the device
    assert torch.equal(from_gpu_layer.weight_codes.cpu(), cpu.weight_codes) and torch.equal(from_gpu_layer(x.to(DEV)), yg)
    with pytest.raises(RuntimeError, match="requires grad"):
        gpu(x.to(DEV).requires_grad_(True))
    # the exact class: the two devices give the same bits
    g = torch.Generator().manual_seed(3)
    xc, xs, wc, ws = exact_case(g, 2, 5, 4, C, Cout, 3, 3, afmt, wfmt)
    ec = MXConvTranspose2d(wc, ws, wfmt, torch.randint(-8, 8, (Cout,), generator=g).float(), 2, 1, 1, 1, afmt)
    xe = G.values(xc, xs, afmt).float().permute(0, 3, 1, 2)               # quantizes back to an exact-class tensor's values
    assert torch.equal(copy.deepcopy(ec).to(DEV)(xe.to(DEV)).cpu(), ec(xe))
    with pytest.raises(ValueError, match="is on"):
        mx_conv_transpose2d(xc.to(DEV), xs.to(DEV), afmt, wc, ws, wfmt)


def test_non_default_stream():
    g = torch.Generator().manual_seed(5)
    fx, fw = "mxfp8_e4m3", "mxfp4_e2m1"
    ops = exact_case(g, 2, 5, 4, 64, 136, 3, 3, fx, fw)
    dev = tuple(t.to(DEV) for t in ops)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = convt(dev, fx, fw, VEC, None, 2, 1, 1, 1)
    s.synchronize()
    assert G.same(y, T.conv_transpose64(G.values(ops[0], ops[1], fx), G.values(ops[2], ops[3], fw), None, 2, 1, 1, 1).float())


def test_graph_capture_of_quantize_then_conv_transpose_replays_bit_for_bit():
    g = torch.Generator().manual_seed(11)
    fx, fw = "mxfp8_e4m3", "mxfp4_e2m1"
    B, H, W, C, Cout = 4, 7, 7, 64, 96
    _, wc, ws = quantize_with_mx((torch.randn(Cout, 3, 3, C, generator=g) / (9 * C) ** 0.5).to(DEV), fw, -1, return_codes=True)
    bias = torch.randn(Cout, generator=g).to(DEV)
    xs_ = [torch.randn(B, C, H, W, generator=g).bfloat16().to(DEV).contiguous(memory_format=torch.channels_last) for _ in range(3)]

    def step(x):
        _, xc, xsc = quantize_with_mx(x.permute(0, 2, 3, 1), fx, -1, return_codes=True)
        return mx_conv_transpose2d(xc, xsc, fx, wc, ws, fw, bias, 2, 1, 1, 1, torch.bfloat16)

    eager = [step(x).clone() for x in xs_]
    static_x = xs_[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # (a host synchronisation or a foreign allocation on the path would fail the capture)
        static_y = step(static_x)
    for x, want in zip(xs_, eager):
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_y, want)
