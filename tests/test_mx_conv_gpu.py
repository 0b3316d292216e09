"""Convolutions on MX codes on the GPU: the implicit-GEMM kernel (qs_mx_conv2d_v) with the route of every call asserted --
bit-identical to ``mx_matmul`` on the host-built im2col operands (tests/mx_conv_ref.py), bit for bit against the float64 convolution
on the exact class, within the derived bound on quantizer-produced inputs, plus the checks a transposed or skipped tap cannot pass.

The general-class bound is test_mx_gemm_gpu.py's with K' = KH KW Cp as the contraction length:
|y32 - y64| <= 2 K' 2^-23 S + ulp_ydt(y64) (+ 2^-23 |bias|), S = the sum of the absolute products in float64; used for K' >= 512."""
import pytest
import torch
import torch.nn as nn

import mx_conv_ref as R
import mx_gemm_ref as G
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_conv import MXConv2d, mx_conv2d
from qsparse_amd.mx_gemm import mx_matmul
from qsparse_amd.quantize import MXQuantizer, quantize_with_mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
PAIRS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp6_e2m3", "mxfp8_e5m2"), ("mxfp8_e4m3", "mxfp4_e2m1"),
         ("mxfp6_e3m2", "mxfp8_e4m3")]
GEMM, VEC, PLAIN = _hip.MX_CONV_ROUTE_GEMM, _hip.MX_CONV_ROUTE_VEC, _hip.MX_CONV_ROUTE_PLAIN
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# B, H, W, C, Cout, (KH, KW), stride, padding, dilation, route
CASES = [
    (3, 9, 7, 64, 130, (3, 3), 1, 1, 1, VEC),             # M = 189 and N = 130 both cross a tile edge
    (2, 9, 7, 160, 17, (3, 3), 2, 1, 1, VEC),             # Cp = 160: a 128-step straddles taps
    (2, 8, 8, 48, 40, (3, 2), (2, 1), (2, 0), 1, VEC),    # Cp = 64: a short last block per tap
    (2, 8, 8, 16, 33, (5, 5), 1, 2, 1, VEC),              # every second piece is channel padding
    (2, 11, 10, 32, 20, (3, 3), 1, 2, 2, VEC),            # dilation
    (2, 6, 5, 3, 16, (3, 3), 1, 1, 1, PLAIN),             # a stem
    (1, 7, 7, 20, 1, (1, 1), 1, 0, 1, PLAIN),
    (2, 7, 9, 40, 130, (3, 3), 1, 1, 1, PLAIN),
    (2, 9, 7, 64, 17, (1, 1), 1, 0, 1, GEMM),
    (2, 9, 7, 64, 17, (1, 1), 2, 0, 1, VEC),              # a strided 1x1 is not the GEMM route
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


def conv(ops, fx, fw, route, bias=None, stride=1, padding=0, dilation=1, dt=torch.float32):
    y = mx_conv2d(ops[0], ops[1], fx, ops[2], ops[3], fw, bias, stride, padding, dilation, dt)
    assert _hip.mx_conv_last_route == route, (_hip.mx_conv_last_route, route)
    assert y.is_cuda and y.dtype == dt and y.is_contiguous()
    return y


def quantized_case(g, B, H, W, C, Cout, KH, KW, fx, fw):
    """codes and scales as the GPU quantizer writes them, from randn activations and randn / sqrt(fan_in) weights"""
    x, w = torch.randn(B, H, W, C, generator=g), torch.randn(Cout, KH, KW, C, generator=g) / (KH * KW * C) ** 0.5
    _, xc, xs = quantize_with_mx(x.to(DEV), fx, -1, return_codes=True)
    _, wc, ws = quantize_with_mx(w.to(DEV), fw, -1, return_codes=True)
    return xc, xs, wc, ws


def exact_conv_case(g, B, H, W, C, Cout, KH, KW, fx, fw):
    """conv operands of the exact class for the contraction length K' = KH KW Cp (CPU tensors)"""
    Kp = KH * KW * (-(-C // 32) * 32)
    rx, rw = G.scale_windows(Kp, fx, fw)
    G.assert_exact_class(Kp, fx, fw, rx, rw)
    xc, xs = G.exact_operand(g, B * H * W, C, fx, rx)
    wc, ws = G.exact_operand(g, Cout * KH * KW, C, fw, rw)
    nb = xs.shape[-1]
    return xc.view(B, H, W, C), xs.view(B, H, W, nb), wc.view(Cout, KH, KW, C), ws.view(Cout, KH, KW, nb)


def check_against_im2col(g, case, fx, fw, dtypes=DTYPES, shift=False):
    B, H, W, C, Cout, (KH, KW), stride, padding, dilation, route = case
    ops = quantized_case(g, B, H, W, C, Cout, KH, KW, fx, fw)
    A, SA, Wp, SWp = R.im2col_codes(*ops, KH, KW, stride, padding, dilation)
    if shift:                                              # code bases one byte past a 16-byte boundary: the byte-load kernel
        ops, route = (offset_by_one(ops[0]), ops[1], offset_by_one(ops[2]), ops[3]), PLAIN
    bias = torch.randn(Cout, generator=g).to(DEV)
    for dt in dtypes:
        for b in (None, bias):
            y = conv(ops, fx, fw, route, b, stride, padding, dilation, dt)
            want = mx_matmul(A, SA, fx, Wp, SWp, fw, b, dt)
            assert _hip.mx_gemm_last_route == _hip.MX_GEMM_ROUTE_VEC and _hip.mx_gemm_last_split == 1      # K' % 32 == 0, fresh operands
            assert y.shape == (B, R.out_size(H, KH, R.pair(stride)[0], R.pair(padding)[0], R.pair(dilation)[0]),
                               R.out_size(W, KW, R.pair(stride)[1], R.pair(padding)[1], R.pair(dilation)[1]), Cout)
            assert G.same(y.reshape(-1, Cout), want), (case, fx, fw, dt, b is not None, shift)


@pytest.mark.parametrize("fx,fw", ALL_PAIRS)
def test_bit_identical_to_matmul_on_im2col_every_format_pair(fx, fw):
    g = torch.Generator().manual_seed(200 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    check_against_im2col(g, CASES[0], fx, fw)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_bit_identical_to_matmul_on_im2col_every_geometry(fx, fw):
    g = torch.Generator().manual_seed(300 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    for case in CASES[1:]:
        check_against_im2col(g, case, fx, fw)
    check_against_im2col(g, CASES[0], fx, fw, (torch.float32,), shift=True)
    check_against_im2col(g, CASES[2], fx, fw, (torch.bfloat16,), shift=True)


# B, H, W, C, Cout, (KH, KW), stride, padding, dilation, route: the last two are dilated, the second of them with OH == OW == 1
EXACT_GEOMETRIES = ((2, 9, 7, 32, 130, (3, 3), 1, 1, 1, VEC), (2, 9, 7, 40, 20, (3, 3), 1, 1, 1, PLAIN), (2, 9, 7, 64, 17, (1, 1), 2, 0, 1, VEC),
                    (2, 11, 10, 32, 20, (3, 3), 1, 2, 2, VEC), (2, 9, 9, 32, 17, (3, 3), 1, 1, 5, VEC))


def check_against_conv64(g, geometry, fx, fw):
    """the comparison that does not pass through mx_matmul: exact-class operands against torch's float64 convolution of their values"""
    B, H, W, C, Cout, (KH, KW), stride, padding, dilation, route = geometry
    ops = exact_conv_case(g, B, H, W, C, Cout, KH, KW, fx, fw)
    bias = torch.randint(-16, 16, (Cout,), generator=g).float()
    y64 = R.conv64(G.values(ops[0], ops[1], fx), G.values(ops[2], ops[3], fw), bias, stride, padding, dilation)
    dev = tuple(t.to(DEV) for t in ops)
    for dt in DTYPES:
        y = conv(dev, fx, fw, route, bias.to(DEV), stride, padding, dilation, dt)
        assert G.same(y, y64.to(dt)), (geometry, dt)
        assert torch.equal(y.cpu(), mx_conv2d(*ops[:2], fx, *ops[2:], fw, bias, stride, padding, dilation, dt))      # the CPU path


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_exact_class_bit_for_bit_against_the_float64_convolution(fx, fw):
    g = torch.Generator().manual_seed(400 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    for geometry in EXACT_GEOMETRIES:
        check_against_conv64(g, geometry, fx, fw)


@pytest.mark.parametrize("fx,fw", ALL_PAIRS)
def test_exact_class_against_the_float64_convolution_every_format_pair(fx, fw):
    check_against_conv64(torch.Generator().manual_seed(450 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw)), EXACT_GEOMETRIES[0], fx, fw)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_general_class_within_the_derived_bound(fx, fw):
    g = torch.Generator().manual_seed(500 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    B, H, W, C, Cout, KH, KW = 2, 9, 7, 64, 40, 3, 3                      # K' = 576
    dev = quantized_case(g, B, H, W, C, Cout, KH, KW, fx, fw)
    xv, wv = G.values(dev[0], dev[1], fx), G.values(dev[2], dev[3], fw)
    bias = torch.randn(Cout, generator=g)
    S = R.conv64(xv.abs(), wv.abs(), None, 1, 1, 1)
    for dt, b in ((torch.float32, None), (torch.bfloat16, bias), (torch.float32, bias), (torch.float16, None)):
        y64 = R.conv64(xv, wv, b, 1, 1, 1)
        y = conv(dev, fx, fw, VEC, None if b is None else b.to(DEV), 1, 1, 1, dt)
        bound = 2 * KH * KW * C * 2.0 ** -23 * S + G.ulp(y64, dt) + (0 if b is None else 2.0 ** -23 * b.abs().double())
        ok, ratio = G.within(y, y64, bound)
        print(fx, fw, dt, "largest |err| / bound", ratio)
        assert ok, (dt, ratio)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_one_hot_weight_returns_the_shifted_strided_input_channel(fx, fw):
    """w = 1.0 at one (kh, kw, c): y[b, oh, ow, n] = x[b, oh sh - ph + kh dh, ow sw - pw + kw dw, c], zero in the padding -- a swap of h
    with w or of kh with kw cannot pass on a non-square image with unequal strides and paddings"""
    g = torch.Generator().manual_seed(6)
    B, H, W, C, Cout, KH, KW = 2, 9, 6, 48, 5, 3, 2
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation = (2, 1), (2, 1), (2, 1)
    xc, xs = G.exact_operand(g, B * H * W, C, fx, 3)
    xc, xs = xc.view(B, H, W, C), xs.view(B, H, W, 2)
    one = int((G.table(fw)[: 1 << G.WIDTH[fw]] == 1.0).nonzero()[0])
    wc, ws = torch.zeros(Cout, KH, KW, C, dtype=torch.uint8), torch.full((Cout, KH, KW, 2), 127, dtype=torch.uint8)
    hot = [(0, 1, 37), (2, 0, 5), (1, 1, 0), (2, 1, 47), (0, 0, 33)]      # (kh, kw, c) of channel n
    for n, (kh, kw, c) in enumerate(hot):
        wc[n, kh, kw, c] = one
    y = conv((xc.to(DEV), xs.to(DEV), wc.to(DEV), ws.to(DEV)), fx, fw, VEC, None, stride, padding, dilation).cpu().double()
    xv = G.values(xc, xs, fx)
    OH, OW = R.out_size(H, KH, sh, ph, dh), R.out_size(W, KW, sw, pw, dw)
    assert y.shape == (B, OH, OW, Cout) and OH != OW
    want = torch.zeros(B, OH, OW, Cout, dtype=torch.float64)
    for n, (kh, kw, c) in enumerate(hot):
        for oh in range(OH):
            for ow in range(OW):
                ih, iw = oh * sh - ph + kh * dh, ow * sw - pw + kw * dw
                if 0 <= ih < H and 0 <= iw < W:
                    want[:, oh, ow, n] = xv[:, ih, iw, c]
    assert torch.equal(y, want) and (want == 0).any() and (want != 0).any()


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_ff_scale_bytes_give_nan_exactly_where_the_window_reads_them(fx, fw):
    g = torch.Generator().manual_seed(7)
    for B, H, W, C, Cout, route in ((2, 9, 7, 64, 130, VEC), (2, 7, 9, 40, 20, PLAIN)):
        stride, padding = (2, 1), (1, 2)
        xc, xs, wc, ws = exact_conv_case(g, B, H, W, C, Cout, 3, 3, fx, fw)
        pb, ph_, pw_, blk = 1, 4, 0, 1                                    # the activation block: pixel (1, 4, 0), channels 32..
        xs[pb, ph_, pw_, blk], ws[7, 2, 0, 0] = 255, 255
        xc[pb, ph_, pw_, 32 * blk:] = 0                                   # (as the quantizer writes such a block)
        wc[7, 2, 0, :32] = 0
        y = conv(tuple(t.to(DEV) for t in (xc, xs, wc, ws)), fx, fw, route, None, stride, padding, 1)
        nan = torch.zeros(y.shape, dtype=torch.bool)
        nan[..., 7] = True
        for oh in range(y.shape[1]):
            for ow in range(y.shape[2]):
                if 0 <= ph_ - (oh * stride[0] - padding[0]) < 3 and 0 <= pw_ - (ow * stride[1] - padding[1]) < 3:
                    nan[pb, oh, ow, :] = True
        assert torch.equal(y.isnan().cpu(), nan) and 0 < int(nan[..., 0].sum()) < nan[..., 0].numel()
        # everything else is still the float64 convolution
        clean = R.conv64(torch.nan_to_num(G.values(xc, xs, fx)), torch.nan_to_num(G.values(wc, ws, fw)), None, stride, padding, 1)
        assert torch.equal(y.cpu().double()[~nan], clean[~nan])


@pytest.mark.parametrize("wfmt,afmt", [("mxfp4_e2m1", "mxfp8_e4m3"), ("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4_e2m1")])
def test_mxconv2d_on_the_gpu_against_the_cpu(wfmt, afmt):
    torch.manual_seed(2)
    C, Cout = 64, 24
    layer = qs.quantize(nn.Conv2d(C, Cout, 3, stride=2, padding=1), bits=G.WIDTH[wfmt], timeout=1, callback=MXQuantizer(wfmt, block_dim=1)).train()
    layer(torch.randn(2, C, 9, 7)), layer(torch.randn(2, C, 9, 7))
    cpu = MXConv2d.from_quantized(layer.eval(), afmt)
    gpu = MXConv2d.from_quantized(layer, afmt).to(DEV)
    assert gpu.weight_codes.is_cuda and torch.equal(gpu.weight_codes.cpu(), cpu.weight_codes) and torch.equal(gpu.weight_scales.cpu(), cpu.weight_scales)
    x = torch.randn(3, C, 9, 7) * 2
    Kp = 9 * C                                                           # 576
    for xin, od in ((x.bfloat16().contiguous(memory_format=torch.channels_last), torch.bfloat16), (x, torch.float32)):
        gpu.out_dtype = cpu.out_dtype = od
        yg = gpu(xin.to(DEV))
        assert _hip.mx_conv_last_route == VEC and yg.shape == (3, Cout, 5, 4) and yg.dtype == od and not yg.requires_grad
        assert yg.is_contiguous(memory_format=torch.channels_last)
        _, xc, xs = quantize_with_mx(xin.permute(0, 2, 3, 1), afmt, -1, return_codes=True)
        xv, wv = G.values(xc.contiguous(), xs.contiguous(), afmt), G.values(cpu.weight_codes, cpu.weight_scales, wfmt)
        y64 = R.conv64(xv, wv, cpu.bias, 2, 1, 1)
        S = R.conv64(xv.abs(), wv.abs(), None, 2, 1, 1)
        bound = 2 * Kp * 2.0 ** -23 * S + G.ulp(y64, od) + 2.0 ** -23 * cpu.bias.abs().double()
        ok, ratio = G.within(yg.permute(0, 2, 3, 1), y64, bound)
        print(wfmt, afmt, od, "largest |err| / bound", ratio)
        assert ok and G.within(cpu(xin).permute(0, 2, 3, 1), y64, bound)[0]
    from_gpu_layer = MXConv2d.from_quantized(layer.to(DEV), afmt)                                        # built on the device
    assert torch.equal(from_gpu_layer.weight_codes.cpu(), cpu.weight_codes) and torch.equal(from_gpu_layer(x.to(DEV)), yg)
    with pytest.raises(RuntimeError, match="requires grad"):
        gpu(x.to(DEV).requires_grad_(True))
    # the exact class: the two devices give the same bits
    g = torch.Generator().manual_seed(3)
    xc, xs, wc, ws = exact_conv_case(g, 2, 9, 7, C, Cout, 3, 3, afmt, wfmt)
    ec = MXConv2d(wc, ws, wfmt, torch.randint(-8, 8, (Cout,), generator=g).float(), 2, 1, 1, afmt)
    xe = G.values(xc, xs, afmt).float().permute(0, 3, 1, 2)               # quantizes back to an exact-class tensor's values
    assert torch.equal(copy_to(ec, DEV)(xe.to(DEV)).cpu(), ec(xe))
    with pytest.raises(ValueError, match="is on"):
        mx_conv2d(xc.to(DEV), xs.to(DEV), afmt, wc, ws, wfmt)


def copy_to(module, device):
    import copy
    return copy.deepcopy(module).to(device)


def test_non_default_stream():
    g = torch.Generator().manual_seed(5)
    fx, fw = "mxfp8_e4m3", "mxfp4_e2m1"
    ops = exact_conv_case(g, 2, 9, 7, 64, 136, 3, 3, fx, fw)
    dev = tuple(t.to(DEV) for t in ops)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = conv(dev, fx, fw, VEC, None, 1, 1, 1)
    s.synchronize()
    assert G.same(y, R.conv64(G.values(ops[0], ops[1], fx), G.values(ops[2], ops[3], fw), None, 1, 1, 1).float())


def test_graph_capture_of_quantize_then_conv_replays_bit_for_bit():
    g = torch.Generator().manual_seed(11)
    fx, fw = "mxfp8_e4m3", "mxfp4_e2m1"
    B, H, W, C, Cout = 4, 14, 14, 64, 96
    _, wc, ws = quantize_with_mx((torch.randn(Cout, 3, 3, C, generator=g) / (9 * C) ** 0.5).to(DEV), fw, -1, return_codes=True)
    bias = torch.randn(Cout, generator=g).to(DEV)
    xs_ = [torch.randn(B, C, H, W, generator=g).bfloat16().to(DEV).contiguous(memory_format=torch.channels_last) for _ in range(3)]

    def step(x):
        _, xc, xsc = quantize_with_mx(x.permute(0, 2, 3, 1), fx, -1, return_codes=True)
        return mx_conv2d(xc, xsc, fx, wc, ws, fw, bias, 1, 1, 1, torch.bfloat16)

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
