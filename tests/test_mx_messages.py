"""The wording of the argument errors the products on MX codes share, and what the two training layers show and count: the operand
check is one function behind three wordings (matmul; convolution, "(the channels)"; weight gradient, "(the batch)"), the bias,
``out_dtype`` and ``wgrad_split_k`` checks are one each, and ``MXTrainLinear`` / ``MXTrainConv2d`` take their options, their ``repr`` tail
and their stochastic-rounding counter from one mixin.  Every string below is the literal text; CPU tensors only."""
import re

import pytest
import torch
import torch.nn as nn

from qsparse_amd.mx_conv import mx_conv2d
from qsparse_amd.mx_conv_train import MXTrainConv2d, mx_conv2d_train, mx_conv2d_weight_grad
from qsparse_amd.mx_gemm import MXTrainLinear, mx_linear, mx_matmul

F8 = "mxfp8_e4m3"
RETURNS = "the bytes quantize_with_mx(..., return_codes=True) returns"


def u8(*shape, device="cpu"):
    return torch.zeros(shape, dtype=torch.uint8, device=device)


def raises(kind, text, fn, *args, **kw):
    with pytest.raises(kind, match="^" + re.escape(text) + "$"):
        fn(*args, **kw)


def test_matmul_operand_messages():
    a, sa, b, sb = u8(4, 64), u8(4, 2), u8(8, 64), u8(8, 2)
    mm = lambda a=a, sa=sa, b=b, sb=sb: mx_matmul(a, sa, F8, b, sb, F8)
    assert mm().shape == (4, 8)
    raises(TypeError, "a_codes must be a tensor, got list", mm, a=[1])
    raises(TypeError, "b_scales must be a tensor, got NoneType", mm, sb=None)
    raises(TypeError, f"a_scales must be uint8 ({RETURNS}), got torch.float32", mm, sa=sa.float())
    raises(TypeError, f"b_codes must be uint8 ({RETURNS}), got torch.int8", mm, b=b.to(torch.int8))
    raises(ValueError, "a_codes needs at least one dimension [..., K], got shape ()", mm, a=u8(), sa=u8())
    raises(ValueError, "b_codes needs 2 dimensions [N, K], got shape (64,)", mm, b=u8(64), sb=u8(2))
    raises(ValueError, "b_codes must be [N, K], got shape (2, 8, 64)", mm, b=u8(2, 8, 64), sb=u8(2, 8, 2))
    raises(ValueError, "a_scales has shape (4, 3), expected (4, 2): one E8M0 byte per block of 32 along the last dimension of a_codes (4, 64)",
           mm, sa=u8(4, 3))
    raises(ValueError, "b_scales has shape (8,), expected (8, 2): one E8M0 byte per block of 32 along the last dimension of b_codes (8, 64)",
           mm, sb=u8(8))
    raises(ValueError, "a_codes is on cpu but a_scales on meta", mm, sa=u8(4, 2, device="meta"))
    raises(ValueError, "b_codes is on cpu but b_scales on meta", mm, sb=u8(8, 2, device="meta"))
    raises(ValueError, "unknown MX format 'fp8': one of ['mxfp4_e2m1', 'mxfp6_e2m3', 'mxfp6_e3m2', 'mxfp8_e4m3', 'mxfp8_e5m2']",
           mx_matmul, a, sa, "fp8", b, sb, F8)


def test_conv_operand_messages():
    x, sx, w, sw = u8(2, 5, 5, 40), u8(2, 5, 5, 2), u8(16, 3, 3, 40), u8(16, 3, 3, 2)
    conv = lambda x=x, sx=sx, w=w, sw=sw: mx_conv2d(x, sx, F8, w, sw, F8)
    assert conv().shape == (2, 3, 3, 16)
    raises(TypeError, "x_codes must be a tensor, got tuple", conv, x=(1,))
    raises(TypeError, f"w_scales must be uint8 ({RETURNS}), got torch.int32", conv, sw=sw.int())
    raises(ValueError, "x_codes needs 4 dimensions [B, H, W, C], got shape (4, 64)", conv, x=u8(4, 64), sx=u8(4, 2))
    raises(ValueError, "w_codes needs 4 dimensions [Cout, KH, KW, C], got shape (1, 16, 3, 3, 40)", conv, w=u8(1, 16, 3, 3, 40), sw=sw)
    raises(ValueError, "x_scales has shape (2, 5, 5, 1), expected (2, 5, 5, 2): one E8M0 byte per block of 32 along the last dimension (the "
           "channels) of x_codes (2, 5, 5, 40)", conv, sx=u8(2, 5, 5, 1))
    raises(ValueError, "w_scales has shape (16, 3, 3), expected (16, 3, 3, 2): one E8M0 byte per block of 32 along the last dimension (the "
           "channels) of w_codes (16, 3, 3, 40)", conv, sw=u8(16, 3, 3))
    raises(ValueError, "x_codes is on cpu but x_scales on meta", conv, sx=u8(2, 5, 5, 2, device="meta"))
    raises(ValueError, "w_codes is on cpu but w_scales on meta", conv, sw=u8(16, 3, 3, 2, device="meta"))


def test_weight_gradient_operand_messages():
    g, sg, x, sx = u8(3, 3, 16, 40), u8(3, 3, 16, 2), u8(5, 5, 8, 40), u8(5, 5, 8, 2)
    wgrad = lambda g=g, sg=sg, x=x, sx=sx: mx_conv2d_weight_grad(g, sg, F8, x, sx, F8, 3)
    assert wgrad().shape == (16, 3, 3, 8)
    raises(TypeError, "dyt_scales must be a tensor, got int", wgrad, sg=3)
    raises(TypeError, "dyt_codes must be uint8 (the bytes mx_quantize_2way returns), got torch.float32", wgrad, g=g.float())
    raises(TypeError, "xt_scales must be uint8 (the bytes mx_quantize_2way returns), got torch.int8", wgrad, sx=sx.to(torch.int8))
    raises(ValueError, "dyt_codes needs 4 dimensions [OH, OW, Cout, B], got shape (9, 16, 40)", wgrad, g=u8(9, 16, 40), sg=u8(9, 16, 2))
    raises(ValueError, "xt_codes needs 4 dimensions [H, W, C, B], got shape (8, 8)", wgrad, x=u8(8, 8), sx=u8(8, 1))
    raises(ValueError, "dyt_scales has shape (3, 3, 16, 40), expected (3, 3, 16, 2): one E8M0 byte per block of 32 along the last dimension "
           "(the batch) of dyt_codes (3, 3, 16, 40)", wgrad, sg=u8(3, 3, 16, 40))
    raises(ValueError, "xt_scales has shape (5, 5, 8, 1), expected (5, 5, 8, 2): one E8M0 byte per block of 32 along the last dimension "
           "(the batch) of xt_codes (5, 5, 8, 40)", wgrad, sx=u8(5, 5, 8, 1))
    raises(ValueError, "dyt_codes is on cpu but dyt_scales on meta", wgrad, sg=u8(3, 3, 16, 2, device="meta"))
    raises(ValueError, "xt_codes is on cpu but xt_scales on meta", wgrad, sx=u8(5, 5, 8, 2, device="meta"))


def test_bias_and_out_dtype_messages():
    dtypes = "(torch.float32, torch.bfloat16, torch.float16)"
    mm = lambda bias, out_dtype=torch.float32: mx_matmul(u8(4, 64), u8(4, 2), F8, u8(8, 64), u8(8, 2), F8, bias, out_dtype)
    conv = lambda bias, out_dtype=torch.float32: mx_conv2d(u8(2, 5, 5, 40), u8(2, 5, 5, 2), F8, u8(16, 3, 3, 40), u8(16, 3, 3, 2), F8, bias,
                                                          out_dtype=out_dtype)
    for product, n, first in ((mm, 8, "a_codes"), (conv, 16, "x_codes")):
        assert product(torch.ones(n))[0].flatten()[0] == 1.0
        raises(TypeError, "bias must be a float32 tensor", product, torch.ones(n, dtype=torch.float64))
        raises(TypeError, "bias must be a float32 tensor", product, [0.0] * n)
        raises(ValueError, f"bias has shape (3,), expected ({n},)", product, torch.ones(3))
        raises(ValueError, f"bias has shape (1, {n}), expected ({n},)", product, torch.ones(1, n))
        raises(ValueError, f"{first} is on cpu but bias on meta", product, torch.ones(n, device="meta"))
        raises(TypeError, f"out_dtype must be one of {dtypes}, got torch.float64", product, None, torch.float64)
    raises(TypeError, f"out_dtype must be one of {dtypes}, got torch.int8", mx_conv2d_weight_grad, u8(3, 3, 16, 40), u8(3, 3, 16, 2), F8,
           u8(5, 5, 8, 40), u8(5, 5, 8, 2), F8, 3, out_dtype=torch.int8)


def test_training_entry_messages():
    dtypes = "(torch.float32, torch.bfloat16, torch.float16)"
    linear = lambda x=torch.zeros(40, 64), w=torch.zeros(32, 64), b=None, **kw: mx_linear(x, w, b, **kw)
    conv = lambda x=torch.zeros(4, 32, 8, 8), w=torch.zeros(16, 32, 3, 3), b=None, **kw: mx_conv2d_train(x, w, b, **kw)
    for entry, n in ((linear, 32), (conv, 16)):
        raises(ValueError, 'wgrad_split_k must be an int >= 1 or "auto", got 0', entry, wgrad_split_k=0)
        raises(ValueError, 'wgrad_split_k must be an int >= 1 or "auto", got \'sixteen\'', entry, wgrad_split_k="sixteen")
        raises(ValueError, f'wgrad_split_k must be an int >= 1 or "auto", got {2 ** 31}', entry, wgrad_split_k=2 ** 31)
        raises(TypeError, 'wgrad_split_k must be an int >= 1 or "auto", got float', entry, wgrad_split_k=2.0)
        raises(TypeError, 'wgrad_split_k must be an int >= 1 or "auto", got bool', entry, wgrad_split_k=True)
        raises(TypeError, "weight must be a tensor, got NoneType", entry, w=None)
        raises(TypeError, f"x must be one of {dtypes}, got torch.float64", entry, x=torch.zeros(40, 64, dtype=torch.float64))
        raises(TypeError, f"bias must be one of {dtypes}, got torch.int64", entry, b=torch.zeros(n, dtype=torch.int64))
        raises(ValueError, "x is on cpu but weight on meta", entry, w=torch.zeros(n, 64, device="meta"))
        raises(ValueError, f"bias has shape (3,), expected ({n},)", entry, b=torch.zeros(3))
        raises(ValueError, "unknown rounding 'up': one of ('nearest', 'stochastic')", entry, grad_rounding="up")
        raises(TypeError, "step must be a one-element int64 tensor (or None)", entry, grad_rounding="stochastic", step=torch.zeros(2, dtype=torch.int64))
        # their order when a call is wrong in several ways: the split request, the formats, the tensors, the rounding, the shapes
        bad = dict(w=torch.zeros(n, 64, dtype=torch.float64), b=torch.zeros(3), grad_rounding="up")
        raises(ValueError, 'wgrad_split_k must be an int >= 1 or "auto", got 0', entry, **bad, x_fmt="fp8", wgrad_split_k=0)
        raises(ValueError, "unknown MX format 'fp8': one of ['mxfp4_e2m1', 'mxfp6_e2m3', 'mxfp6_e3m2', 'mxfp8_e4m3', 'mxfp8_e5m2']", entry, **bad, x_fmt="fp8")
        raises(TypeError, f"weight must be one of {dtypes}, got torch.float64", entry, **bad)
        raises(ValueError, "unknown rounding 'up': one of ('nearest', 'stochastic')", entry, b=torch.zeros(3), grad_rounding="up")
        raises(TypeError, "x must be a tensor, got list", entry, x=[1.0], grad_rounding="stochastic", step=torch.zeros(1, dtype=torch.int64))
    for layer in (lambda **kw: MXTrainLinear(64, 32, **kw), lambda **kw: MXTrainConv2d(32, 16, 3, **kw)):
        raises(ValueError, 'wgrad_split_k must be an int >= 1 or "auto", got -1', layer, wgrad_split_k=-1)
        raises(TypeError, 'wgrad_split_k must be an int >= 1 or "auto", got NoneType', layer, wgrad_split_k=None)
        raises(ValueError, "unknown rounding 'up': one of ('nearest', 'stochastic')", layer, grad_rounding="up")


FMTS = "x_fmt='mxfp8_e4m3', w_fmt='mxfp8_e4m3', grad_fmt='mxfp8_e5m2'"
SR = dict(grad_rounding="stochastic", wgrad_split_k=4)


def test_repr_of_the_training_layers():
    assert isinstance(MXTrainLinear(64, 32), nn.Linear) and isinstance(MXTrainConv2d(32, 16, 3), nn.Conv2d)
    assert repr(MXTrainLinear(64, 32)) == f"MXTrainLinear(in_features=64, out_features=32, bias=True, {FMTS})"
    assert repr(MXTrainLinear(64, 32, bias=False, **SR)) == (f"MXTrainLinear(in_features=64, out_features=32, bias=False, {FMTS}, "
                                                            "grad_rounding='stochastic', wgrad_split_k=4)")
    assert repr(MXTrainConv2d(32, 16, 3, padding=1)) == f"MXTrainConv2d(32, 16, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), {FMTS})"
    assert repr(MXTrainConv2d(32, 16, 3, bias=False, **SR)) == (f"MXTrainConv2d(32, 16, kernel_size=(3, 3), stride=(1, 1), bias=False, {FMTS}, "
                                                               "grad_rounding='stochastic', wgrad_split_k=4)")
    assert repr(MXTrainLinear.from_linear(nn.Linear(64, 32), **SR)) == repr(MXTrainLinear(64, 32, **SR))
    assert repr(MXTrainConv2d.from_conv(nn.Conv2d(32, 16, 3), **SR)) == repr(MXTrainConv2d(32, 16, 3, **SR))


@pytest.mark.parametrize("kind", ["linear", "conv"])
def test_the_step_counter_is_not_saved_and_advances_by_one_per_backward(kind):
    torch.manual_seed(0)
    if kind == "linear":
        base, x = nn.Linear(64, 32), torch.randn(40, 64)
        built, adopted = MXTrainLinear(64, 32, seed=5, **SR), MXTrainLinear.from_linear(base, seed=5, **SR)
    else:
        base, x = nn.Conv2d(32, 16, 3), torch.randn(4, 32, 8, 8)
        built, adopted = MXTrainConv2d(32, 16, 3, seed=5, **SR), MXTrainConv2d.from_conv(base, seed=5, **SR)
    assert adopted.weight is base.weight and adopted.bias is base.bias and adopted.training == base.training
    assert not type(built)(*((64, 32) if kind == "linear" else (32, 16, 3))).state_dict().keys() - {"weight", "bias"}        # nearest: the torch layer's
    assert not hasattr(type(built)(*((64, 32) if kind == "linear" else (32, 16, 3))), "sr_step")
    for layer in (built, adopted):
        assert sorted(layer.state_dict()) == ["bias", "weight"] and "sr_step" in dict(layer.named_buffers())
        assert layer.sr_seed == 5 and layer.sr_step.dtype == torch.int64 and layer.sr_step.tolist() == [0]
        for n in (1, 2, 3):
            y = layer(x)
            assert layer.sr_step.tolist() == [n - 1]            # the forward does not touch it
            y.sum().backward()
            assert layer.sr_step.tolist() == [n]
        with torch.no_grad():
            layer(x)
        assert layer.sr_step.tolist() == [3]
    assert isinstance(MXTrainLinear(64, 32, **SR).sr_seed, int)                # drawn from torch's generator when no seed is given
