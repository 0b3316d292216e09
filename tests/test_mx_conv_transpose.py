"""Transposed convolutions on MX codes, CPU side: the ATen path of ``mx_conv_transpose2d`` against ``mx_matmul`` on the gathered
operands of tests/mx_conv_transpose_ref.py and against the float64 ``F.conv_transpose2d`` of the de-quantized tensors, the input
gradient wrapper against autograd, the layer ``MXConvTranspose2d``, and the entry point's declaration / binding / validation (no
GPU needed for any of it)."""
import copy
import ctypes
import os
import subprocess

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp6_e2m3", "mxfp8_e5m2"), ("mxfp8_e4m3", "mxfp4_e2m1"),
         ("mxfp6_e3m2", "mxfp8_e4m3")]
BITS = {f: G.WIDTH[f] for f in G.FMTS}
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# B, H, W, C, Cout, (KH, KW), stride, padding, output_padding, dilation
GEOMS = [
    (2, 5, 4, 48, 7, (3, 3), 2, 1, 1, 1),                 # the shape of the main GPU test, fewer channels out
    (1, 4, 3, 40, 5, (3, 2), (2, 3), (1, 0), 0, (2, 1)),  # unequal strides and dilations
    (1, 6, 6, 32, 4, (3, 3), 2, 3, 0, 1),                 # p > d (k - 1): a crop, 7 x 7
    (2, 4, 5, 20, 3, (1, 3), 2, (0, 1), 0, 1),            # KH == 1
    (2, 5, 4, 33, 3, (3, 1), 2, (1, 0), 0, 1),            # KW == 1
    (2, 4, 3, 64, 6, (1, 1), 2, 0, 0, 1),                 # 1x1 with holes
    (3, 1, 1, 16, 5, (3, 3), 2, 0, 0, 1),                 # H == W == 1
    (1, 3, 4, 32, 4, (2, 2), (3, 2), 0, (2, 1), 1),       # op == s - 1
    (2, 4, 3, 64, 6, (1, 1), 1, 0, 0, 1),                 # what the GPU forwards to the matrix product
]


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def exact_case(g, B, H, W, C, Cout, KH, KW, fx, fw):
    """operands of the exact class for the contraction length K' = KH KW Cp"""
    Kp = KH * KW * (-(-C // 32) * 32)
    rx, rw = G.scale_windows(Kp, fx, fw)
    G.assert_exact_class(Kp, fx, fw, rx, rw)
    xc, xs = G.exact_operand(g, B * H * W, C, fx, rx)
    wc, ws = G.exact_operand(g, Cout * KH * KW, C, fw, rw)
    nb = xs.shape[-1]
    return xc.view(B, H, W, C), xs.view(B, H, W, nb), wc.view(Cout, KH, KW, C), ws.view(Cout, KH, KW, nb)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_cpu_path_equals_gathered_matmul_and_float64_conv_transpose_on_the_exact_class(fx, fw):
    g = torch.Generator().manual_seed(G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    for B, H, W, C, Cout, (KH, KW), stride, padding, out_pad, dilation in GEOMS:
        xc, xs, wc, ws = exact_case(g, B, H, W, C, Cout, KH, KW, fx, fw)
        bias = torch.randint(-16, 16, (Cout,), generator=g).float()
        A, SA, Wp, SWp = T.gathered_codes(xc, xs, wc, ws, stride, padding, out_pad, dilation)
        y64 = T.conv_transpose64(G.values(xc, xs, fx), G.values(wc, ws, fw), bias, stride, padding, out_pad, dilation)
        for dt in DTYPES:
            got = mx_conv_transpose2d(xc, xs, fx, wc, ws, fw, bias, stride, padding, out_pad, dilation, dt)
            assert got.dtype == dt and got.is_contiguous() and got.shape == y64.shape, (H, W, C, dt)
            # every order of summation is exact on this class: equality with both forms of the definition
            assert torch.equal(got.reshape(-1, Cout), mx_matmul(A, SA, fx, Wp, SWp, fw, bias, dt)), (H, W, C, dt)
            assert torch.equal(got, y64.to(dt)), (H, W, C, dt)
        assert torch.equal(mx_conv_transpose2d(xc, xs, fx, wc, ws, fw, None, stride, padding, out_pad, dilation),
                           T.conv_transpose64(G.values(xc, xs, fx), G.values(wc, ws, fw), None, stride, padding, out_pad, dilation).float())


@pytest.mark.parametrize("fx,fw", PAIRS[:3])
def test_cpu_path_on_quantizer_inputs_and_nan_blocks(fx, fw):
    """general operands: the two float64 summations (the convolution's and the matmul's) differ by their order only: K' 2^-52 S each"""
    g = torch.Generator().manual_seed(2)
    B, H, W, C, Cout, KH, KW = 2, 5, 4, 40, 9, 3, 3
    geom = dict(stride=(2, 1), padding=(1, 0), output_padding=(1, 0), dilation=1)
    x, w = torch.randn(B, H, W, C, generator=g), torch.randn(Cout, KH, KW, C, generator=g) / (C * 9) ** 0.5
    _, xc, xs = quantize_with_mx(x, fx, -1, return_codes=True)
    _, wc, ws = quantize_with_mx(w, fw, -1, return_codes=True)
    bias = torch.randn(Cout, generator=g)
    A, SA, Wp, SWp = T.gathered_codes(xc, xs, wc, ws, **geom)
    _, y64, S = G.reference(A, SA, fx, Wp, SWp, fw, bias)
    for dt in DTYPES:
        got = mx_conv_transpose2d(xc, xs, fx, wc, ws, fw, bias, out_dtype=dt, **geom)
        ok, ratio = G.within(got.reshape(-1, Cout), y64, A.shape[1] * 2.0 ** -52 * S + G.ulp(y64, dt))
        print(fx, fw, dt, "largest |err| / bound", ratio)
        assert ok, (dt, ratio)
    # 0xFF: the outputs with an existing tap on the pixel, and the whole output channel -- also where no tap exists
    xs[1, 3, 2, 1], ws[4, 0, 2, 0] = 255, 255
    got = mx_conv_transpose2d(xc, xs, fx, wc, ws, fw, bias, **geom)
    A, SA, Wp, SWp = T.gathered_codes(xc, xs, wc, ws, **geom)
    want_nan = G.reference(A, SA, fx, Wp, SWp, fw, bias)[1].isnan().view(got.shape)
    nan = torch.zeros_like(want_nan)
    nan[..., 4] = True
    for oh in range(got.shape[1]):
        for ow in range(got.shape[2]):
            th, tw = oh + 1 - 3 * 2, ow + 0 - 2 * 1            # kh = oh + ph - ih sh, kw = ow + pw - iw sw at dilation 1
            if 0 <= th < KH and 0 <= tw < KW:
                nan[1, oh, ow, :] = True
    assert torch.equal(want_nan, nan) and torch.equal(got.isnan(), nan) and 0 < int(nan[1, ..., 0].sum()) < nan[1, ..., 0].numel()


@pytest.mark.parametrize("fy,fw", PAIRS[:3])
def test_input_grad_against_autograd(fy, fw):
    g = torch.Generator().manual_seed(3)
    # B, H, W, Cin, Cout, (KH, KW), stride, padding, dilation: the first two leave rows of x that no window reaches
    for B, H, W, Cin, Cout, (KH, KW), stride, padding, dilation in ((2, 8, 8, 5, 40, (3, 3), 2, 1, 1), (1, 9, 6, 4, 32, (2, 3), (3, 2), (0, 1), 1),
                                                                      (2, 7, 7, 3, 33, (3, 3), 1, 2, 2), (1, 5, 6, 6, 64, (1, 1), 1, 0, 1)):
        OH, OW = (_hip.mx_conv_out_size(n, k, s, p, d) for n, k, s, p, d in zip((H, W), (KH, KW), T.pair(stride), T.pair(padding), T.pair(dilation)))
        dy, w = torch.randn(B, OH, OW, Cout, generator=g), torch.randn(Cin, KH, KW, Cout, generator=g) / (KH * KW * Cout) ** 0.5
        _, dyc, dys = quantize_with_mx(dy, fy, -1, return_codes=True)
        _, wtc, wts = quantize_with_mx(w, fw, -1, return_codes=True)
        dyv, wv = G.values(dyc, dys, fy), G.values(wtc, wts, fw)
        x = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, wv.permute(3, 0, 1, 2), None, T.pair(stride), T.pair(padding), T.pair(dilation))
        (dx64,) = torch.autograd.grad(y, x, dyv.permute(0, 3, 1, 2))
        S = torch.autograd.grad(F.conv2d(x, wv.abs().permute(3, 0, 1, 2), None, T.pair(stride), T.pair(padding), T.pair(dilation)), x,
                                dyv.abs().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
        dx64 = dx64.permute(0, 2, 3, 1)
        Kp = KH * KW * (-(-Cout // 32) * 32)
        for dt in DTYPES:
            dx = mx_conv2d_input_grad(dyc, dys, fy, wtc, wts, fw, (H, W), stride, padding, dilation, dt)
            assert dx.shape == (B, H, W, Cin) and dx.dtype == dt
            ok, ratio = G.within(dx, dx64, 2 * Kp * 2.0 ** -52 * S + G.ulp(dx64, dt))      # two float64 summations in different orders
            assert ok, (H, W, dt, ratio)
    with pytest.raises(ValueError, match="not the gradient"):
        mx_conv2d_input_grad(dyc, dys, fy, wtc, wts, fw, (6, 6))
    with pytest.raises(ValueError, match="input_size"):
        mx_conv2d_input_grad(dyc, dys, fy, wtc, wts, fw, (5, 0))
    with pytest.raises(ValueError, match="dy_scales has shape"):
        mx_conv2d_input_grad(dyc, dys[..., :1], fy, wtc, wts, fw, (5, 6))
    with pytest.raises(ValueError, match="disagree on C"):
        mx_conv2d_input_grad(dyc, dys, fy, wtc[..., :32].contiguous(), wts[..., :1].contiguous(), fw, (5, 6))
    assert qs.mx_conv2d_input_grad is mx_conv2d_input_grad


def test_arguments_are_checked_before_anything_runs():
    g = torch.Generator().manual_seed(0)
    xc, xs, wc, ws = exact_case(g, 2, 5, 5, 40, 3, 3, 3, "mxfp8_e4m3", "mxfp4_e2m1")
    ok = lambda **kw: mx_conv_transpose2d(**{**dict(x_codes=xc, x_scales=xs, x_fmt="mxfp8_e4m3", w_codes=wc, w_scales=ws, w_fmt="mxfp4_e2m1"), **kw})
    assert ok().shape == (2, 7, 7, 3) and ok(padding=1, stride=(2, 1), output_padding=(1, 0)).shape == (2, 10, 5, 3)
    with pytest.raises(ValueError, match="unknown MX format"):
        ok(w_fmt="mxfp5")
    with pytest.raises(TypeError, match="uint8"):
        ok(x_codes=xc.float())
    with pytest.raises(TypeError, match="must be a tensor"):
        ok(w_scales=None)
    with pytest.raises(ValueError, match="4 dimensions"):
        ok(x_codes=xc[0], x_scales=xs[0])
    with pytest.raises(ValueError, match="x_scales has shape"):
        ok(x_scales=xs[..., :1])
    with pytest.raises(ValueError, match="disagree on C"):
        ok(w_codes=wc[..., :32].contiguous(), w_scales=ws[..., :1].contiguous())
    with pytest.raises(ValueError, match="needs C, H, W, KH, KW >= 1"):
        ok(x_codes=xc[:, :0], x_scales=xs[:, :0])
    with pytest.raises(TypeError, match="float32"):
        ok(bias=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="bias has shape"):
        ok(bias=torch.zeros(4))
    with pytest.raises(TypeError, match="out_dtype"):
        ok(out_dtype=torch.float64)
    with pytest.raises(ValueError, match="string"):
        ok(padding="same")
    with pytest.raises(TypeError, match="stride"):
        ok(stride=2.0)
    with pytest.raises(ValueError, match="stride"):
        ok(stride=0)
    with pytest.raises(ValueError, match="padding"):
        ok(padding=(1, -1))
    with pytest.raises(ValueError, match="dilation"):
        ok(dilation=(1, 2, 3))
    with pytest.raises(ValueError, match="output_padding"):
        ok(output_padding=-1)
    with pytest.raises(ValueError, match="smaller than either stride or dilation"):
        ok(output_padding=1)
    with pytest.raises(ValueError, match="smaller than either stride or dilation"):
        ok(stride=(2, 3), dilation=(3, 1), output_padding=(2, 3))
    assert ok(stride=(2, 3), dilation=(3, 1), output_padding=(2, 2)).shape == (2, 17, 17, 3)       # op < max(s, d)
    with pytest.raises(ValueError, match="crops the whole output"):
        ok(padding=4)                                                                              # 4 - 8 + 2 + 1 < 1
    empty = ok(x_codes=xc[:0], x_scales=xs[:0], bias=torch.zeros(3))
    assert empty.shape == (0, 7, 7, 3) and empty.dtype == torch.float32
    assert qs.mx_conv_transpose2d is mx_conv_transpose2d and qs.MXConvTranspose2d is MXConvTranspose2d


def _quantized_deconv(fmt, block_dim=0, seed=0, **kw):
    torch.manual_seed(seed)
    deconv = nn.ConvTranspose2d(40, 24, 3, **{**dict(stride=2, padding=1, output_padding=1), **kw})
    layer = qs.quantize(deconv, bits=BITS[fmt], timeout=1, callback=MXQuantizer(fmt, block_dim=block_dim)).train()
    layer(torch.randn(2, 40, 5, 4)), layer(torch.randn(2, 40, 5, 4))
    return layer.eval()


@pytest.mark.parametrize("wfmt,afmt", [("mxfp4_e2m1", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp6_e3m2"), ("mxfp8_e4m3", "mxfp4_e2m1")])
def test_mxconvtranspose2d_from_quantized(wfmt, afmt):
    layer = _quantized_deconv(wfmt)
    ex = qs.export_integer(nn.Sequential(layer))["0"].weight
    m = MXConvTranspose2d.from_quantized(layer, afmt)
    assert (m.weight_fmt, m.act_fmt, m.out_dtype) == (wfmt, afmt, torch.float32)
    assert (m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.output_padding, m.dilation) == \
        (40, 24, (3, 3), (2, 2), (1, 1), (1, 1), (1, 1))
    assert m.weight_codes.shape == (24, 3, 3, 40) and m.weight_scales.shape == (24, 3, 3, 2)
    assert torch.equal(m.weight_codes, ex.codes.permute(1, 2, 3, 0)) and torch.equal(m.weight_scales, ex.block_scale.permute(1, 2, 3, 0))
    assert m.weight_codes.is_contiguous() and m.bias.dtype == torch.float32 and torch.equal(m.bias, layer.bias.detach())
    x = torch.randn(2, 40, 5, 4, generator=torch.Generator().manual_seed(4)) * 3
    for xin in (x, x.contiguous(memory_format=torch.channels_last), x.bfloat16()):
        y = m(xin)
        assert y.shape == (2, 24, 10, 8) and y.dtype == torch.float32 and not y.requires_grad
        assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(m(x), m(x.contiguous(memory_format=torch.channels_last)))
    # the simulated layer on the quantized input computes the same transposed convolution in float32
    xq, xc, xs = quantize_with_mx(x.permute(0, 2, 3, 1), afmt, -1, return_codes=True)
    A, SA, Wp, SWp = T.gathered_codes(xc.contiguous(), xs.contiguous(), m.weight_codes, m.weight_scales, 2, 1, 1, 1)
    _, y64, S = G.reference(A, SA, afmt, Wp, SWp, wfmt, m.bias)
    Kp = A.shape[1]
    assert G.within(m(x).permute(0, 2, 3, 1).reshape(-1, 24), y64, Kp * 2.0 ** -52 * S + G.ulp(y64, torch.float32))[0]
    with torch.no_grad():
        sim = layer(xq.permute(0, 3, 1, 2))
    assert G.within(sim.permute(0, 2, 3, 1).reshape(-1, 24), y64,
                    2 * Kp * 2.0 ** -23 * S + 2.0 ** -23 * m.bias.abs().double() + G.ulp(y64, torch.float32))[0]
    assert torch.equal(G.values(m.weight_codes, m.weight_scales, wfmt).float(), layer.weight.detach().permute(1, 2, 3, 0))


def test_mxconvtranspose2d_constructors_refusals_and_state_dict():
    layer = _quantized_deconv("mxfp6_e3m2")
    ex = qs.export_integer(nn.Sequential(layer))["0"]
    a = MXConvTranspose2d.from_quantized(layer, "mxfp8_e4m3")
    b = MXConvTranspose2d.from_exported(ex.weight, layer.bias.detach(), 2, 1, 1, 1, "mxfp8_e4m3")
    x = torch.randn(2, 40, 5, 4)
    assert torch.equal(a(x), b(x)) and set(a.state_dict()) == {"weight_codes", "weight_scales", "bias"}
    assert torch.equal(a.weight_codes, b.weight_codes) and torch.equal(a.weight_scales, b.weight_scales) and torch.equal(a.bias, b.bias)
    assert not list(a.parameters()) and "weight_fmt='mxfp6_e3m2'" in repr(a) and "output_padding=(1, 1)" in repr(a)
    nobias = MXConvTranspose2d.from_exported(ex.weight, None, act_fmt="mxfp4_e2m1", out_dtype=torch.bfloat16)
    assert nobias.bias is None and set(nobias.state_dict()) == {"weight_codes", "weight_scales"}
    assert nobias(x).shape == (2, 24, 7, 6) and nobias(x).dtype == torch.bfloat16
    other = MXConvTranspose2d.from_quantized(_quantized_deconv("mxfp6_e3m2", seed=9), "mxfp8_e4m3")
    assert not torch.equal(other(x), a(x))
    other.load_state_dict(copy.deepcopy(a.state_dict()))
    assert torch.equal(other(x), a(x))
    # refusals: inference only, groups, padding modes, the block axis, layers that are not MX
    with pytest.raises(RuntimeError, match="requires grad"):
        a(x.clone().requires_grad_(True))
    with torch.no_grad():
        assert not a(x.clone().requires_grad_(True)).requires_grad
    with pytest.raises(ValueError, match="groups"):
        MXConvTranspose2d.from_quantized(_quantized_deconv("mxfp8_e4m3", groups=2), "mxfp8_e4m3")
    odd = _quantized_deconv("mxfp8_e4m3")
    odd.padding_mode = "reflect"           # (nn.ConvTranspose2d itself accepts zeros only; a subclass might not)
    with pytest.raises(ValueError, match="padding_mode"):
        MXConvTranspose2d.from_quantized(odd, "mxfp8_e4m3")
    for dim in (1, -1):
        along = _quantized_deconv("mxfp8_e4m3", block_dim=dim)
        with pytest.raises(ValueError, match=r"MXQuantizer\(fmt, block_dim=0\)"):
            MXConvTranspose2d.from_quantized(along, "mxfp8_e4m3")
        with pytest.raises(ValueError, match=r"MXQuantizer\(fmt, block_dim=0\)"):
            MXConvTranspose2d.from_exported(qs.export_integer(nn.Sequential(along))["0"].weight, None)
    scaler = qs.quantize(nn.ConvTranspose2d(40, 24, 3), bits=8, timeout=1).train()
    scaler(x), scaler(x)
    with pytest.raises(ValueError, match="MXQuantizer"):
        MXConvTranspose2d.from_quantized(scaler, "mxfp8_e4m3")
    with pytest.raises(ValueError, match="kind"):
        MXConvTranspose2d.from_exported(qs.export_integer(nn.Sequential(scaler))["0"].weight, None)
    conv = qs.quantize(nn.Conv2d(40, 24, 3), bits=8, timeout=1, callback=MXQuantizer("mxfp8_e4m3", block_dim=0)).train()
    conv(torch.randn(2, 40, 5, 4)), conv(torch.randn(2, 40, 5, 4))
    with pytest.raises(ValueError, match="nn.ConvTranspose2d"):
        MXConvTranspose2d.from_quantized(conv, "mxfp8_e4m3")
    lin = qs.quantize(nn.Linear(70, 12), bits=8, timeout=1, callback=MXQuantizer("mxfp8_e4m3", block_dim=0)).train()
    lin(torch.randn(3, 70)), lin(torch.randn(3, 70))
    with pytest.raises(ValueError, match="4-d"):
        MXConvTranspose2d.from_exported(qs.export_integer(nn.Sequential(lin))["0"].weight, None)
    fresh = qs.quantize(nn.ConvTranspose2d(40, 24, 3), bits=8, timeout=5, callback=MXQuantizer("mxfp8_e4m3", block_dim=0))
    with pytest.raises(ValueError, match="timeout"):
        MXConvTranspose2d.from_quantized(fresh, "mxfp8_e4m3")
    with pytest.raises(ValueError, match="unknown MX format"):
        MXConvTranspose2d.from_quantized(layer, "mxfp3")
    with pytest.raises(TypeError, match="out_dtype"):
        MXConvTranspose2d.from_quantized(layer, "mxfp8_e4m3", torch.float64)
    with pytest.raises(ValueError, match="bias has shape"):
        MXConvTranspose2d.from_exported(ex.weight, torch.zeros(40))
    with pytest.raises(ValueError, match=r"\[B, 40, H, W\]"):
        a(torch.randn(2, 39, 5, 4))


def _args(**kw):
    a = _hip.MxConvTranspose2dArgs()
    a.struct_size = ctypes.sizeof(a)
    a.x_codes, a.x_scales, a.w_codes, a.w_scales, a.y = 1024, 2048, 4096, 8192, 16384
    a.B, a.H, a.W, a.C, a.Cout, a.KH, a.KW = 2, 5, 4, 64, 5, 3, 3
    a.stride_h = a.stride_w = 2
    a.dil_h = a.dil_w = 1
    a.pad_h = a.pad_w = 1
    a.out_pad_h = a.out_pad_w = 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_entry_point_is_declared_bound_and_validates_without_a_gpu(tmp_path):
    lib = _hip.load()
    VEC, PLAIN, GEMM = _hip.MX_CONV_ROUTE_VEC, _hip.MX_CONV_ROUTE_PLAIN, _hip.MX_CONV_ROUTE_GEMM
    assert lib.qs_version() == _hip.ABI_VERSION == 28 and lib.qs_abi_floor() == 25     # symbols were added, the version stays
    assert "qs_mx_conv_transpose2d_v" in _hip.SIGNATURES and "qs_mx_conv_transpose2d_route" in _hip.SIGNATURES
    assert lib.qs_mx_conv_transpose2d_v(None) == -2 and lib.qs_mx_conv_transpose2d_route(None) == -2     # a null descriptor
    v = lambda **kw: lib.qs_mx_conv_transpose2d_v(ctypes.byref(_args(**kw)))
    route = lambda **kw: lib.qs_mx_conv_transpose2d_route(ctypes.byref(_args(**kw)))
    blank = _hip.MxConvTranspose2dArgs()
    blank.struct_size = ctypes.sizeof(blank)
    assert lib.qs_mx_conv_transpose2d_route(ctypes.byref(blank)) == -2           # no tensors
    for null in ("x_codes", "x_scales", "w_codes", "w_scales", "y"):
        assert route(**{null: None}) == -2 and v(**{null: None}) == -2
    assert route(x_format=5) == -2 and route(w_format=-1) == -2                  # unknown format
    assert route(ydt=7) == -1                                                    # unknown dtype
    assert route(y=16386) == -3 and v(y=16386) == -3                             # y not aligned to a float32
    assert route(y=16386, ydt=1) == VEC                                          # ... but to a bf16
    assert route(bias=6) == -3                                                   # bias not aligned to a float32
    for bad in (dict(C=0), dict(C=-1), dict(KH=0), dict(KW=0), dict(H=0), dict(W=0), dict(B=-1), dict(Cout=-1), dict(stride_h=0),
                dict(stride_w=0), dict(dil_h=0), dict(dil_w=-1), dict(pad_h=-1), dict(pad_w=-1), dict(out_pad_h=-1), dict(out_pad_w=-1)):
        assert route(**bad) == -2, bad
    # the output padding: < max(stride, dilation) of its axis
    assert route(out_pad_h=2) == -2 and route(out_pad_w=2) == -2
    assert route(out_pad_h=2, dil_h=3) == VEC and route(out_pad_w=2, stride_w=3) == VEC
    assert route(out_pad_h=3, dil_h=3) == -2 and route(stride_h=1, stride_w=1) == -2
    assert route(out_pad_h=0, out_pad_w=0) == VEC
    # an output extent < 1: (5 - 1) 2 - 2 p + 2 + 1 + 1 = 12 - 2 p
    assert route(pad_h=5) == VEC and route(pad_h=6) == -2 and route(pad_w=5) == -2 and v(pad_h=6) == -2
    # extents the kernel's 32-bit coordinates cannot hold: H, C + 32, oh + ph, (KH - 1) dh
    assert route(H=2 ** 31) == -2 and route(C=2 ** 31 - 16) == -2
    assert route(H=2 ** 30 + 1) == -2 and route(H=2 ** 29, stride_h=3) == VEC
    assert route(dil_h=2 ** 30 + 1) == -2 and route(KH=2, dil_h=2 ** 30 + 1) == VEC
    assert route(B=0) == 0 and route(Cout=0) == 0 and v(B=0) == 0 and v(Cout=0) == 0      # an empty problem: accepted, nothing enqueued
    assert v(B=0, ydt=7) == -1 and v(B=0, C=0) == -2 and v(B=0, out_pad_h=2) == -2        # ... after the checks
    short = _hip.MxConvTranspose2dArgs()
    short.struct_size = 2
    assert lib.qs_mx_conv_transpose2d_route(ctypes.byref(short)) == -2           # a descriptor too short to carry its own size
    assert route(struct_size=_hip.MxConvTranspose2dArgs.KH.offset) == -2         # ... or one that ends before the kernel size (KH = 0)
    assert route(struct_size=_hip.MxConvTranspose2dArgs.out_pad_h.offset) == VEC           # ... before the output padding: read as zero
    # the route the call would take, decided by the launching code itself
    assert route() == VEC
    assert route(C=16) == VEC and route(C=48) == VEC
    assert route(C=40) == PLAIN and route(C=3) == PLAIN                          # C % 16 != 0
    assert route(x_codes=1025) == PLAIN and route(w_codes=4097) == PLAIN
    assert route(x_scales=2049, w_scales=8193) == VEC                            # scale bytes: any address
    one = dict(KH=1, KW=1, pad_h=0, pad_w=0, stride_h=1, stride_w=1, out_pad_h=0, out_pad_w=0)
    assert route(**one) == GEMM
    assert route(**one, x_codes=1025) == GEMM                                    # (the matmul picks its own kernel for the base)
    assert route(**one, dil_h=3) == GEMM                                         # the dilation of a 1x1 kernel moves nothing
    assert route(**{**one, "dil_h": 3, "out_pad_h": 1}) == VEC                   # ... but an output padding adds a row
    assert route(**{**one, "stride_w": 2}) == VEC                                # a strided 1x1 leaves holes
    assert route(**{**one, "pad_h": 1}) == VEC                                   # a crop
    assert route(**one, C=48) == VEC and route(**one, C=20) == PLAIN             # C % 32 != 0
    # the ctypes mirror against the header's own layout
    fields = [f for f, _ in _hip.MxConvTranspose2dArgs._fields_]
    assert fields[-3:] == ["out_pad_h", "out_pad_w", "stream"] and fields[:-3] == [f for f, _ in _hip.MxConv2dArgs._fields_][:-1]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu", sizeof(qs_mx_conv_transpose2d_args));\n%s\nreturn 0; }\n'
                   % (os.path.join(ROOT, "include", "qsparse_hip.h"), "\n".join(f'printf(" %zu", offsetof(qs_mx_conv_transpose2d_args, {f}));' for f in fields)))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(src)], check=True)
    size, *offs = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(_hip.MxConvTranspose2dArgs)
    assert [int(o) for o in offs] == [getattr(_hip.MxConvTranspose2dArgs, f).offset for f in fields]
