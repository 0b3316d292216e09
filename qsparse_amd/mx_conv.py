"""Convolutions on MX codes: ``mx_conv2d`` and the inference-side layer ``MXConv2d`` -- the counterparts of ``mx_matmul`` and
``MXLinear`` for ``nn.Conv2d``.

Layouts are channels-last, so that the MX blocks of 32 run along the input channels: the contraction axis, innermost in memory,
as the matrix instruction needs.  ``quantize_with_mx(x.permute(0, 2, 3, 1), fmt, -1, return_codes=True)`` hands out the
activation's bytes (zero-copy for a ``torch.channels_last`` tensor), a ``quantize(nn.Conv2d(...), callback=MXQuantizer(fmt,
block_dim=1))`` layer exports the weight's.  On the GPU ``mx_conv2d`` is one HIP kernel (``qs_mx_conv2d_v``): an implicit GEMM
on the block-scaled MFMA of gfx950 that gathers the windows while it stages them -- no im2col matrix is ever written -- and
accumulates in float32; on the CPU it evaluates the definition in float64.  ``MXConv2d`` is an inference layer; training through
the three products of a convolution (forward, input gradient, weight gradient) is ``mx_conv2d_train`` / ``MXTrainConv2d`` of
``qsparse_amd/mx_conv_train.py``.  The operand, ``out_dtype`` and bias checks are ``_mx_common.py``'s, shared with ``mx_matmul``."""
from functools import partial
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from qsparse_amd import _hip, _mx_common
from qsparse_amd._mx_common import MXActivation, _check_bias, _check_bias_shape, _check_codes_out, _check_dtype, _codes_out_cpu, _pair
from qsparse_amd.quantize import MX_FORMATS, MXQuantizer, _mx_format, mx_dequantize, quantize_with_mx


# a channels-last operand with blocks along the channels
_check_operand = partial(_mx_common._check_operand, axis=" (the channels)")


def _check_product(fn: str, x_codes, x_scales, x_fmt: str, w_codes, w_scales, w_fmt: str, bias, out_dtype):
    """the operand, C, device, out_dtype and bias checks of the public product `fn` (the name in its messages)"""
    _check_operand("x", x_codes, x_scales, x_fmt, "[B, H, W, C]")
    _check_operand("w", w_codes, w_scales, w_fmt, "[Cout, KH, KW, C]")
    (B, H, W, C), (Cout, KH, KW, Cw) = x_codes.shape, w_codes.shape
    if Cw != C:
        raise ValueError(f"x_codes {tuple(x_codes.shape)} and w_codes {tuple(w_codes.shape)} disagree on C (their last dimensions)")
    if C < 1 or KH < 1 or KW < 1 or H < 1 or W < 1:
        raise ValueError(f"{fn} needs C, H, W, KH, KW >= 1, got x_codes {tuple(x_codes.shape)}, w_codes {tuple(w_codes.shape)}")
    if w_codes.device != x_codes.device:
        raise ValueError(f"x_codes is on {x_codes.device} but w_codes on {w_codes.device}")
    _check_dtype("out_dtype", out_dtype)
    _check_bias(bias, Cout, "x_codes", x_codes.device)


def mx_conv2d(x_codes: torch.Tensor, x_scales: torch.Tensor, x_fmt: str, w_codes: torch.Tensor, w_scales: torch.Tensor, w_fmt: str,
              bias: Optional[torch.Tensor] = None, stride=1, padding=0, dilation=1, out_dtype: torch.dtype = torch.float32,
              out_fmt: Optional[str] = None, act: Optional[str] = None):
    """``conv2d(x, w) (+ bias)`` on MX codes, channels-last.  ``x_codes`` ``[B, H, W, C]`` and ``w_codes`` ``[Cout, KH, KW, C]`` are
    uint8 codes of the formats ``x_fmt`` / ``w_fmt`` (``MX_FORMATS``; they may differ) with blocks along C, ``x_scales`` ``[B, H, W,
    ceil(C / 32)]`` and ``w_scales`` ``[Cout, KH, KW, ceil(C / 32)]`` their E8M0 bytes, ``bias`` float32 ``[Cout]``; ``stride``,
    ``padding`` (zeros) and ``dilation`` an int or a pair each; ``groups`` is 1.  Returns ``[B, OH, OW, Cout]``, contiguous, in
    ``out_dtype`` (float32, bfloat16 or float16):

        y[b, oh, ow, n] = round( sum_{kh, kw, c} val(x[b, ih, iw, c]) 2^(sx[b, ih, iw, c / 32] - 127)
                                               * val(w[n, kh, kw, c]) 2^(sw[n, kh, kw, c / 32] - 127) + bias[n] )
        ih = oh * stride_h - pad_h + kh * dil_h,    iw = ow * stride_w - pad_w + kw * dil_w

    with ``val`` the value of a code as ``mx_dequantize`` decodes it; a tap outside the image contributes zero.  A scale byte 0xFF
    makes every output whose window reads that block NaN.  GPU tensors take the HIP kernel -- float32 accumulation in the order of
    ``mx_matmul`` on the im2col operands, to which the result is bit-identical; there is no fallback: without the library the call
    raises -- CPU tensors evaluate the expression above in float64 and round once.  Input channels are padded to a multiple of 32
    per tap inside the kernel, so a stem (C = 3) spends most of its products on zeros and is slow.

    ``out_fmt`` (a name of ``MX_FORMATS``) makes the convolution hand out MX codes instead of a float tensor: the return is ``(codes
    uint8 [B, OH, OW, Cout], scales uint8 [B, OH, OW, ceil(Cout / 32)])``, bit for bit the codes and scales of
    ``quantize_with_mx(act(y), out_fmt, -1, return_codes=True)`` with ``y`` the float32 result above and blocks along Cout -- the next
    convolution's C.  ``act`` is ``None`` or ``"relu"`` (NaN stays NaN, everything else that is not positive becomes +0) and needs
    ``out_fmt``; ``out_dtype`` must stay at its default.  On the GPU it is one kernel (``qs_mx_conv2d_q_v``): the quantizer runs on
    the accumulators and no float ``y`` is written or read.  CPU tensors round the float64 result once to float32, apply ``act`` and
    run the CPU quantizer."""
    _check_codes_out("mx_conv2d", out_fmt, act, out_dtype)
    _check_product("mx_conv2d", x_codes, x_scales, x_fmt, w_codes, w_scales, w_fmt, bias, out_dtype)
    (H, W), (KH, KW) = x_codes.shape[1:3], w_codes.shape[1:3]
    stride, padding, dilation = _pair("stride", stride, 1), _pair("padding", padding, 0), _pair("dilation", dilation, 1)
    OH = _hip.mx_conv_out_size(H, KH, stride[0], padding[0], dilation[0])
    OW = _hip.mx_conv_out_size(W, KW, stride[1], padding[1], dilation[1])
    if OH < 1 or OW < 1:
        raise ValueError(f"the kernel {KH}x{KW} (dilation {dilation}) does not fit the padded image {H + 2 * padding[0]}x{W + 2 * padding[1]}: "
                         f"the output would be {OH}x{OW}")
    if x_codes.is_cuda and out_fmt is not None:
        return _hip.mx_conv2d_q(x_codes.contiguous(), x_scales.contiguous(), x_fmt, w_codes.contiguous(), w_scales.contiguous(), w_fmt,
                                None if bias is None else bias.contiguous(), stride, padding, dilation, out_fmt, act)
    if x_codes.is_cuda:
        return _hip.mx_conv2d(x_codes.contiguous(), x_scales.contiguous(), x_fmt, w_codes.contiguous(), w_scales.contiguous(), w_fmt,
                              None if bias is None else bias.contiguous(), stride, padding, dilation, out_dtype)
    x = mx_dequantize(x_codes, x_scales, x_fmt, -1, torch.float64).permute(0, 3, 1, 2)
    w = mx_dequantize(w_codes, w_scales, w_fmt, -1, torch.float64).permute(0, 3, 1, 2)
    # a 0xFF block is NaN in every window that reads it, also against a zero (NaN * 0 is NaN): the convolution's own propagation
    y = F.conv2d(x, w, None if bias is None else bias.to(torch.float64), stride, padding, dilation)
    y = y.permute(0, 2, 3, 1).to(out_dtype).contiguous()
    return y if out_fmt is None else _codes_out_cpu(y, out_fmt, act)


class _MXConvBase(nn.Module):
    """what ``MXConv2d`` and ``MXConvTranspose2d`` share: the weight buffers and attributes, the checks of an exported weight and
    ``forward``.  A subclass names the layer it stands for and the layout of that layer's weight, and supplies ``_product``."""
    _layer = None                  # the torch layer
    _weight_layout = ""            # of its weight, for messages
    _perm = ()                     # that weight -> [Cout, KH, KW, C]
    _block_dim = 0                 # the input channels in that weight
    _block_dim_note = ""

    def __init__(self, weight_codes: torch.Tensor, weight_scales: torch.Tensor, weight_fmt: str, bias, stride, padding, dilation, act_fmt: str,
                 out_dtype: torch.dtype):
        super().__init__()
        _mx_format(act_fmt)
        _check_operand("w", weight_codes, weight_scales, weight_fmt, "[Cout, KH, KW, C]")
        _check_dtype("out_dtype", out_dtype)
        _check_bias_shape(bias, weight_codes.shape[0])
        self.weight_fmt, self.act_fmt, self.out_dtype = weight_fmt, act_fmt, out_dtype
        self.stride, self.padding, self.dilation = _pair("stride", stride, 1), _pair("padding", padding, 0), _pair("dilation", dilation, 1)
        self.out_channels, self.in_channels = weight_codes.shape[0], weight_codes.shape[3]
        self.kernel_size = (weight_codes.shape[1], weight_codes.shape[2])
        self.register_buffer("weight_codes", weight_codes.detach().clone().contiguous())
        self.register_buffer("weight_scales", weight_scales.detach().clone().contiguous())
        self.register_buffer("bias", None if bias is None else bias.detach().to(torch.float32).clone().contiguous())

    def _extra_field(self) -> str:
        """what ``extra_repr`` shows between the padding and the dilation"""
        return ""

    def extra_repr(self) -> str:
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, "
                f"{self._extra_field()}dilation={self.dilation}, bias={self.bias is not None}, weight_fmt={self.weight_fmt!r}, "
                f"act_fmt={self.act_fmt!r}")

    @classmethod
    def _channels_last(cls, qt):
        """the codes and scales ``[Cout, KH, KW, C]`` of an exported weight ``qt``, checked"""
        name = f"MX{cls._layer.__name__}"
        if getattr(qt, "kind", None) != "mx":
            raise ValueError(f"{name} needs an MX weight (QuantizedTensor.kind == 'mx'), got kind {getattr(qt, 'kind', None)!r}")
        if qt.codes.dim() != 4:
            raise ValueError(f"{name} needs a 4-d weight {cls._weight_layout}, got shape {tuple(qt.codes.shape)}")
        if qt.block_dim % qt.codes.dim() != cls._block_dim:
            raise ValueError(f"the weight's MX blocks run along dim {qt.block_dim}, not along the input channels ({cls._block_dim_note}): "
                             "such blocks cannot feed the matrix instruction -- quantize the layer with "
                             f"MXQuantizer(fmt, block_dim={cls._block_dim})")
        return qt.codes.permute(*cls._perm).contiguous(), qt.block_scale.permute(*cls._perm).contiguous()

    def _product(self, codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def _input_codes(self, x: torch.Tensor):
        """the checks of a float input ``[B, C, H, W]`` and its channels-last codes and scales in ``act_fmt``"""
        layer = self._layer.__name__
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError(f"MX{layer} is an inference layer: its input requires grad.  Train with the simulated layer "
                               f"(quantize(nn.{layer}(...), callback=MXQuantizer(...))) or call it under torch.no_grad()")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"MX{layer} expects [B, {self.in_channels}, H, W], got shape {tuple(x.shape)}")
        with torch.no_grad():
            _, codes, scales = quantize_with_mx(x.permute(0, 2, 3, 1), self.act_fmt, -1, return_codes=True)
            if not codes.is_contiguous():      # an input that was not channels_last: one layout pass
                codes, scales = codes.contiguous(), scales.contiguous()
            return codes, scales

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        codes, scales = self._input_codes(x)
        with torch.no_grad():
            return self._product(codes, scales).permute(0, 3, 1, 2)


class MXConv2d(_MXConvBase):
    """``nn.Conv2d`` (``groups == 1``, zero padding) for inference on MX codes: the weight is held channels-last as uint8 codes
    ``weight_codes [Cout, KH, KW, C]`` and E8M0 scales ``weight_scales [Cout, KH, KW, ceil(C / 32)]`` of the format ``weight_fmt``
    (buffers, with the optional float32 ``bias``).  ``forward`` takes ``[B, C, H, W]`` in float32 / bfloat16 / float16, quantizes it
    to ``act_fmt`` along the channels with the MX quantizer and convolves the two sets of codes with ``mx_conv2d``; it returns a
    ``torch.channels_last`` ``[B, Cout, OH, OW]`` tensor in ``out_dtype`` that never requires grad.  An input that requires grad
    while gradients are enabled is refused -- training runs on the simulated layers this one is built from.

    Memory format: a ``torch.channels_last`` input is quantized where it lies (its ``[B, H, W, C]`` view is contiguous and takes
    the quantizer's innermost-axis route).  An NCHW-contiguous input pays one extra layout pass over the activation before the
    quantizer; keep the network channels_last to avoid it.

    Chaining without a float tensor in between: with ``out_fmt`` (keyword; optionally ``act="relu"``) ``forward`` returns an
    ``MXActivation`` holding channels-last codes ``[B, OH, OW, Cout]`` -- the codes and scales of ``quantize_with_mx(act(y), out_fmt)``
    along the channels, written by the convolution's own epilogue -- and ``forward`` also TAKES an ``MXActivation`` with ``[B, H, W,
    C]`` codes in place of a float tensor: its codes are convolved as they are, in their own format (``act_fmt`` is not consulted: the
    product takes any pair).  ``nn.Sequential(MXConv2d(..., out_fmt=f, act="relu"), MXConv2d(...))`` computes bit for bit what the
    two layers compute with a float ReLU between them when the second one's ``act_fmt`` is ``f``."""

    _layer, _weight_layout, _perm, _block_dim, _block_dim_note = nn.Conv2d, "[Cout, C, KH, KW]", (0, 2, 3, 1), 1, "dim 1"

    def __init__(self, weight_codes: torch.Tensor, weight_scales: torch.Tensor, weight_fmt: str, bias: Optional[torch.Tensor] = None,
                 stride=1, padding=0, dilation=1, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *,
                 out_fmt: Optional[str] = None, act: Optional[str] = None):
        super().__init__(weight_codes, weight_scales, weight_fmt, bias, stride, padding, dilation, act_fmt, out_dtype)
        _check_codes_out("MXConv2d", out_fmt, act, out_dtype)
        self.out_fmt, self.act = out_fmt, act

    def extra_repr(self) -> str:
        return (super().extra_repr() + (f", out_fmt={self.out_fmt!r}" if self.out_fmt is not None else "") +
                (f", act={self.act!r}" if self.act is not None else ""))

    @classmethod
    def from_exported(cls, qt, bias: Optional[torch.Tensor] = None, stride=1, padding=0, dilation=1, act_fmt: str = "mxfp8_e4m3",
                      out_dtype: torch.dtype = torch.float32, *, out_fmt: Optional[str] = None, act: Optional[str] = None):
        """from the ``QuantizedTensor(kind="mx")`` ``export_integer`` returns for a conv layer's weight ``[Cout, C, KH, KW]`` with
        blocks along dim 1; codes and scales are permuted to channels-last once, here"""
        return cls(*cls._channels_last(qt), qt.fmt, bias, stride, padding, dilation, act_fmt, out_dtype, out_fmt=out_fmt, act=act)

    @classmethod
    def from_quantized(cls, layer: nn.Module, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *,
                       out_fmt: Optional[str] = None, act: Optional[str] = None):
        """from a ``quantize(nn.Conv2d(...), bits=w, callback=MXQuantizer(fmt, block_dim=1))`` layer that is past its timeout: the
        weight codes are the export's, stride / padding / dilation the layer's, the bias what its evaluation-mode forward adds"""
        from qsparse_amd.export import export_integer
        q = layer.__dict__.get("_modules", {}).get("quantize")
        if not isinstance(layer, nn.Conv2d) or q is None or not isinstance(q.callback, MXQuantizer):
            raise ValueError("MXConv2d.from_quantized needs an nn.Conv2d wrapped by quantize(..., callback=MXQuantizer(...))")
        if layer.groups != 1:
            raise ValueError(f"MXConv2d supports groups == 1 only, the layer has groups={layer.groups}")
        if layer.padding_mode != "zeros":
            raise ValueError(f"MXConv2d supports zero padding only, the layer has padding_mode={layer.padding_mode!r}")
        if isinstance(layer.padding, str):
            raise ValueError(f"MXConv2d needs the padding as numbers, the layer has padding={layer.padding!r}")
        rec = export_integer(nn.Sequential(layer)).get("0")
        if rec is None or rec.weight is None:
            raise ValueError("the layer has not quantized its weight yet (still inside its timeout): nothing to build an MXConv2d from")
        was = layer.training
        layer.eval()
        try:
            with torch.no_grad():
                b = layer.bias
                bias = None if b is None else b.detach().to(torch.float32)
        finally:
            layer.train(was)
        return cls.from_exported(rec.weight, bias, tuple(layer.stride), tuple(layer.padding), tuple(layer.dilation), act_fmt, out_dtype,
                                 out_fmt=out_fmt, act=act)

    def forward(self, x):
        if isinstance(x, MXActivation):
            codes, scales, fmt = x.codes, x.scales, x.fmt
            if not x.channels_last:
                raise ValueError("MXConv2d expects an MXActivation with channels_last=True: codes [B, H, W, C] with blocks along the channels")
            if codes.dim() != 4 or codes.shape[3] != self.in_channels:
                raise ValueError(f"MXConv2d expects an MXActivation with codes [B, H, W, {self.in_channels}], got shape {tuple(codes.shape)}")
        else:
            (codes, scales), fmt = self._input_codes(x), self.act_fmt
        with torch.no_grad():
            y = mx_conv2d(codes, scales, fmt, self.weight_codes, self.weight_scales, self.weight_fmt, self.bias, self.stride, self.padding,
                          self.dilation, self.out_dtype, self.out_fmt, self.act)
            return y.permute(0, 3, 1, 2) if self.out_fmt is None else MXActivation(*y, self.out_fmt, True)


__all__ = ["mx_conv2d", "MXConv2d", "MXActivation", "MX_FORMATS"]
