"""The MX products that write MX codes, without a GPU: the CPU definition of ``mx_matmul(..., out_fmt=)`` / ``mx_conv2d(..., out_fmt=)``,
their refusals, the argument checks of ``qs_mx_matmul_q_v`` / ``qs_mx_conv2d_q_v`` (nothing is enqueued by a refused call), the layout
of their descriptors against the header, and chains of ``MXLinear`` / ``MXConv2d`` that pass ``MXActivation`` between them."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn as nn

import mx_codes_out_ref as R
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_conv import MXConv2d, mx_conv2d
from qsparse_amd.mx_conv_train import MXTrainConv2d
from qsparse_amd.mx_gemm import MXActivation, MXLinear, MXTrainLinear, mx_matmul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4, FP4 = "mxfp8_e4m3", "mxfp4_e2m1"


def _gemm_ops(seed=0, lead=(2, 3), N=70, K=40, fa=E4, fb="mxfp6_e2m3"):
    g = torch.Generator().manual_seed(seed)
    return R.operand(g, lead + (K,), fa) + (fa,) + R.operand(g, (N, K), fb) + (fb,), torch.randn(N, generator=g)


def _conv_ops(seed=1, C=40, Cout=33, fx=E4, fw=FP4):
    g = torch.Generator().manual_seed(seed)
    return R.operand(g, (2, 5, 6, C), fx) + (fx,) + R.operand(g, (Cout, 3, 3, C), fw) + (fw,), torch.randn(Cout, generator=g)


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("out_fmt", R.FORMATS)
def test_cpu_matmul_is_the_composition(out_fmt, act):
    ops, bias = _gemm_ops()
    got = mx_matmul(*ops, bias, out_fmt=out_fmt, act=act)
    assert isinstance(got, tuple) and got[0].shape == (2, 3, 70) and got[1].shape == (2, 3, 3)
    assert R.same(got, R.quantized(mx_matmul(*ops, bias, torch.float32), out_fmt, act))
    assert R.same(mx_matmul(*ops, out_fmt=out_fmt, act=act), R.quantized(mx_matmul(*ops), out_fmt, act))
    if act == "relu":       # (about half the sums are negative: the activation is not a no-op here)
        assert not R.same(got, mx_matmul(*ops, bias, out_fmt=out_fmt))


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("out_fmt", R.FORMATS)
def test_cpu_conv_is_the_composition(out_fmt, act):
    ops, bias = _conv_ops()
    geo = ((2, 1), (1, 0), (1, 2))
    got = mx_conv2d(*ops, bias, *geo, out_fmt=out_fmt, act=act)
    want = R.quantized(mx_conv2d(*ops, bias, *geo), out_fmt, act)
    assert got[0].shape == want[0].shape and got[0].shape[-1] == 33 and got[1].shape[-1] == 2
    assert R.same(got, want)


def test_special_values_follow_the_quantizer():
    """a NaN row, a ReLU that empties every block, and -0 under the ReLU, on the CPU definition"""
    ops, _ = _gemm_ops(N=33)
    ac, asc, fa, bc, bsc, fb = ops
    asc = asc.clone()
    asc[0, 0, 0] = 255                                              # row (0, 0) of A: NaN in every output of that row
    codes, scales = mx_matmul(ac, asc, fa, bc, bsc, fb, out_fmt=E4, act="relu")
    assert (scales[0, 0] == 255).all() and (codes[0, 0] == 0).all() and (scales[0, 1] != 255).all()
    codes, scales = mx_matmul(*ops, torch.full((33,), -1e30), out_fmt=E4, act="relu")
    assert not codes.any() and not scales.any()
    codes, scales = mx_matmul(*ops, torch.full((33,), -1e30), out_fmt=E4)
    assert (codes >> 7).all()                                       # without it: every sign bit set


def test_refusals():
    ops, bias = _gemm_ops()
    cops, cbias = _conv_ops()
    with pytest.raises(ValueError, match="needs out_fmt"):
        mx_matmul(*ops, bias, act="relu")
    with pytest.raises(ValueError, match="needs out_fmt"):
        mx_conv2d(*cops, cbias, act="relu")
    for bad in ("gelu", "ReLU", 1):
        with pytest.raises(ValueError, match="unknown act"):
            mx_matmul(*ops, bias, out_fmt=E4, act=bad)
        with pytest.raises(ValueError, match="unknown act"):
            mx_conv2d(*cops, cbias, out_fmt=E4, act=bad)
    with pytest.raises(ValueError, match="unknown MX format"):
        mx_matmul(*ops, bias, out_fmt="fp8")
    with pytest.raises(ValueError, match="unknown MX format"):
        mx_conv2d(*cops, cbias, out_fmt="fp8")
    with pytest.raises(ValueError, match="out_dtype"):
        mx_matmul(*ops, bias, torch.bfloat16, out_fmt=E4)
    with pytest.raises(ValueError, match="out_dtype"):
        mx_conv2d(*cops, cbias, out_dtype=torch.float16, out_fmt=E4)
    for split in (2, "auto"):
        with pytest.raises(ValueError, match="split_k"):
            mx_matmul(*ops, bias, split_k=split, out_fmt=E4)
    with pytest.raises(ValueError, match="needs out_fmt"):
        MXLinear(ops[3], ops[4], ops[5], act="relu")
    with pytest.raises(ValueError, match="out_dtype"):
        MXConv2d(cops[3], cops[4], cops[5], out_dtype=torch.bfloat16, out_fmt=E4)


def _matmul_q_args(**over):
    a = _hip.MxMatmulQArgs()
    a.struct_size = ctypes.sizeof(a)
    a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.out_codes, a.out_scales = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    a.M, a.N, a.K = 5, 33, 256
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _conv_q_args(**over):
    a = _hip.MxConv2dQArgs()
    a.struct_size = ctypes.sizeof(a)
    a.x_codes, a.x_scales, a.w_codes, a.w_scales, a.out_codes, a.out_scales = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    a.B, a.H, a.W, a.C, a.Cout, a.KH, a.KW = 2, 13, 11, 48, 33, 3, 3
    a.stride_h = a.stride_w = a.dil_h = a.dil_w = 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_c_entry_points_refuse_before_anything_is_enqueued():
    """every call here returns from the argument checks: safe on a host without a GPU"""
    lib = _hip.load()
    ARG, ALIGN = -2, -3
    for make, v, route in ((_matmul_q_args, lib.qs_mx_matmul_q_v, lib.qs_mx_matmul_q_route),
                           (_conv_q_args, lib.qs_mx_conv2d_q_v, lib.qs_mx_conv2d_q_route)):
        first = "a_codes" if make is _matmul_q_args else "x_codes"
        second = "b_codes" if make is _matmul_q_args else "w_codes"
        assert v(None) == ARG and route(None) == ARG
        short = make()
        short.struct_size = 2
        assert v(ctypes.byref(short)) == ARG
        refused = [make(out_codes=None), make(out_scales=None), make(out_format=5), make(out_format=-1), make(act=2), make(act=-1),
                   make(**{first: None}), make(**{first[0] + "_format": 7}),
                   make(out_codes=0x10000), make(out_codes=0x10000 - 1), make(out_codes=0x30000 + 100)]        # shares bytes with an input
        for a in refused:
            assert v(ctypes.byref(a)) == ARG and route(ctypes.byref(a)) == ARG
        a = make(bias=0x70002)
        assert v(ctypes.byref(a)) == ALIGN and route(ctypes.byref(a)) == ALIGN
        a = make(bias=0x70002, act=3)                                # the QS_ERR_ARG checks come before the alignment's
        assert v(ctypes.byref(a)) == ARG
        assert route(ctypes.byref(make(**{second: 0x30001}))) == (_hip.MX_GEMM_ROUTE_PLAIN if make is _matmul_q_args else _hip.MX_CONV_ROUTE_PLAIN)
        assert route(ctypes.byref(make(out_codes=0x50001, bias=0x70004, act=1, out_format=4))) == (
            _hip.MX_GEMM_ROUTE_VEC if make is _matmul_q_args else _hip.MX_CONV_ROUTE_VEC)
    # an empty product enqueues nothing and succeeds; K == 0 of a non-empty one is refused
    assert lib.qs_mx_matmul_q_v(ctypes.byref(_matmul_q_args(M=0))) == 0 and lib.qs_mx_matmul_q_v(ctypes.byref(_matmul_q_args(N=0))) == 0
    assert lib.qs_mx_matmul_q_v(ctypes.byref(_matmul_q_args(K=0))) == ARG and lib.qs_mx_matmul_q_v(ctypes.byref(_matmul_q_args(M=-1))) == ARG
    assert lib.qs_mx_conv2d_q_v(ctypes.byref(_conv_q_args(B=0))) == 0 and lib.qs_mx_conv2d_q_v(ctypes.byref(_conv_q_args(Cout=0))) == 0
    assert lib.qs_mx_conv2d_q_v(ctypes.byref(_conv_q_args(KH=14))) == ARG                       # the kernel does not fit the image
    assert lib.qs_mx_conv2d_q_route(ctypes.byref(_conv_q_args(KH=1, KW=1, C=64))) == _hip.MX_CONV_ROUTE_GEMM
    assert lib.qs_mx_conv2d_q_route(ctypes.byref(_conv_q_args(KH=1, KW=1, C=64, out_codes=0x10000))) == ARG


def test_descriptors_have_the_headers_layout(tmp_path):
    pairs = {"qs_mx_matmul_q_args": _hip.MxMatmulQArgs, "qs_mx_conv2d_q_args": _hip.MxConv2dQArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "qsparse_hip.h")}"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append(f'printf("{cname} %zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {fname}));' for fname, _ in ct._fields_]
        lines.append('printf("\\n");')
    lines += ['printf("%d %d\\n", QS_MX_ACT_NONE, QS_MX_ACT_RELU);', 'return 0; }']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    for line, (cname, ct) in zip(out, pairs.items()):
        name, size, *offsets = line.split()
        assert name == cname and int(size) == ctypes.sizeof(ct)
        assert [int(o) for o in offsets] == [getattr(ct, f).offset for f, _ in ct._fields_], cname
        assert "y" not in dict(ct._fields_) and "ydt" not in dict(ct._fields_)
    assert out[2].split() == [str(_hip.MX_ACTS.index(None)), str(_hip.MX_ACTS.index("relu"))]


@pytest.mark.parametrize("chain", [R.linear_chain, R.conv_chain])
def test_layer_chain_equals_the_layers_with_a_float_relu_between(chain):
    fused, plain, second, x = chain("cpu")
    mid = fused[0](x)
    assert isinstance(mid, MXActivation) and mid.fmt == fused[0].out_fmt and mid.codes.dtype == mid.scales.dtype == torch.uint8
    want = second(R.relu(plain(x)))
    got = fused(x)
    assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, want) and bool(got.isfinite().all())
    assert "out_fmt=" in repr(fused[0]) and "act='relu'" in repr(fused[0]) and "out_fmt" not in repr(second)
    # what the first layer hands out IS the second one's quantized input, in the NCHW view for a convolution
    _, codes, scales = qs.quantize_with_mx(R.relu(plain(x)), mid.fmt, 1 if x.dim() == 4 else -1, return_codes=True)
    deq = mid.dequantize()
    assert deq.shape == plain(x).shape and torch.equal(deq, qs.quantize_with_mx(R.relu(plain(x)), mid.fmt, 1 if x.dim() == 4 else -1))
    if x.dim() == 4:
        assert mid.channels_last and torch.equal(mid.codes, codes.permute(0, 2, 3, 1)) and torch.equal(mid.scales, scales.permute(0, 2, 3, 1))
        with pytest.raises(ValueError, match="MXActivation with codes"):
            second(MXActivation(mid.codes[..., :40], mid.scales, mid.fmt, True))
        with pytest.raises(ValueError, match="channels_last=True"):
            second(MXActivation(mid.codes, mid.scales, mid.fmt))
        with pytest.raises(ValueError, match="channels_last=True"):
            R.linear_chain("cpu")[2](mid)
    else:
        assert torch.equal(mid.codes, codes) and torch.equal(mid.scales, scales)


def test_constructors_pass_the_keywords_on():
    lin = MXTrainLinear(48, 16).to_inference(out_fmt=FP4, act="relu")
    conv = MXTrainConv2d(40, 16, 3).to_inference(out_fmt=E4)
    assert (lin.out_fmt, lin.act, conv.out_fmt, conv.act) == (FP4, "relu", E4, None)
    assert isinstance(lin(torch.randn(3, 48)), MXActivation) and isinstance(conv(torch.randn(1, 40, 5, 5)), MXActivation)
    assert qs.MXActivation is MXActivation
    layer = qs.quantize(nn.Linear(64, 8), bits=8, timeout=1, callback=qs.MXQuantizer(E4, block_dim=1)).train()
    layer(torch.randn(2, 64)), layer(torch.randn(2, 64))
    layer.eval()
    built = MXLinear.from_quantized(layer, out_fmt="mxfp6_e2m3", act="relu")
    assert (built.out_fmt, built.act) == ("mxfp6_e2m3", "relu") and built(torch.randn(2, 64)).fmt == "mxfp6_e2m3"
