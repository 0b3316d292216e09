"""Transposed convolutions on MX codes: ``mx_conv_transpose2d``, the inference-side layer ``MXConvTranspose2d`` -- the counterparts
of ``mx_conv2d`` and ``MXConv2d`` for ``nn.ConvTranspose2d`` -- and ``mx_conv2d_input_grad``, the input gradient (dgrad) of a
convolution, which is the same product: the transposed convolution of ``dy`` with the convolution's weight.

Layouts are channels-last with the MX blocks of 32 along the contraction channels ``C``: the activation ``[B, H, W, C]`` as
``quantize_with_mx(x.permute(0, 2, 3, 1), fmt, -1, return_codes=True)`` hands it out, the weight ``[Cout, KH, KW, C]`` --
``nn.ConvTranspose2d.weight [C, Cout, KH, KW].permute(1, 2, 3, 0)`` with blocks along its dim 0, which a ``quantize(nn.ConvTranspose2d(
...), callback=MXQuantizer(fmt, block_dim=0))`` layer exports.  For dgrad the contraction runs over the convolution's output
channels: ``dy [B, OH, OW, Cout]`` quantized along its last axis and ``conv.weight [Cout, Cin, KH, KW].permute(1, 2, 3, 0)`` with
blocks along ``Cout``.  On the GPU it is one HIP kernel (``qs_mx_conv_transpose2d_v``): the implicit GEMM of ``mx_conv2d`` with a
fractionally-strided image operand, accumulating in float32; on the CPU the definition is evaluated in float64.  A stride ``s``
spends ``sh sw - 1`` of every ``sh sw`` products on zero codes -- the kernel is correct and untuned, it has no sub-pixel
decomposition.  The weight gradient of a convolution is ``mx_conv2d_weight_grad`` (``qsparse_amd/mx_conv_train.py``)."""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from qsparse_amd import _hip
from qsparse_amd.mx_conv import _check_operand, _check_product, _MXConvBase, _pair
from qsparse_amd.quantize import MX_FORMATS, MXQuantizer, mx_dequantize


def mx_conv_transpose2d(x_codes: torch.Tensor, x_scales: torch.Tensor, x_fmt: str, w_codes: torch.Tensor, w_scales: torch.Tensor, w_fmt: str,
                        bias: Optional[torch.Tensor] = None, stride=1, padding=0, output_padding=0, dilation=1,
                        out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``conv_transpose2d(x, w) (+ bias)`` on MX codes, channels-last.  ``x_codes`` ``[B, H, W, C]`` and ``w_codes`` ``[Cout, KH, KW,
    C]`` are uint8 codes of the formats ``x_fmt`` / ``w_fmt`` (``MX_FORMATS``; they may differ) with blocks along C, ``x_scales``
    ``[B, H, W, ceil(C / 32)]`` and ``w_scales`` ``[Cout, KH, KW, ceil(C / 32)]`` their E8M0 bytes, ``bias`` float32 ``[Cout]``;
    ``stride``, ``padding``, ``output_padding`` (``< max(stride, dilation)``) and ``dilation`` an int or a pair each; ``groups`` is 1.
    Returns ``[B, OH, OW, Cout]``, contiguous, in ``out_dtype`` (float32, bfloat16 or float16), ``OH = (H - 1) stride_h - 2 pad_h +
    dil_h (KH - 1) + out_pad_h + 1``:

        y[b, oh, ow, n] = round( sum_{kh, kw, c} val(x[b, ih, iw, c]) 2^(sx[b, ih, iw, c / 32] - 127)
                                               * val(w[n, kh, kw, c]) 2^(sw[n, kh, kw, c / 32] - 127) + bias[n] )
        ih = (oh + pad_h - kh * dil_h) / stride_h,    iw = (ow + pad_w - kw * dil_w) / stride_w

    a tap exists only where both divisions are exact and the pixel lies inside the image; the kernel indices are the weight's own
    (``w[n, kh, kw, c] = conv_transpose.weight[c, n, kh, kw]``).  A scale byte 0xFF of the weight makes its output channel NaN at every
    pixel, one of the activation exactly the outputs with a tap on that pixel.  GPU tensors take the HIP kernel -- float32
    accumulation in the order of ``mx_matmul`` on the gathered operands, to which the result is bit-identical; there is no fallback:
    without the library the call raises -- CPU tensors evaluate the expression above in float64 and round once."""
    _check_product("mx_conv_transpose2d", x_codes, x_scales, x_fmt, w_codes, w_scales, w_fmt, bias, out_dtype)
    (B, H, W, C), (KH, KW) = x_codes.shape, w_codes.shape[1:3]
    stride, padding, dilation = _pair("stride", stride, 1), _pair("padding", padding, 0), _pair("dilation", dilation, 1)
    output_padding = _pair("output_padding", output_padding, 0)
    if any(op >= max(s, d) for op, s, d in zip(output_padding, stride, dilation)):
        raise ValueError(f"output_padding must be smaller than either stride or dilation, got output_padding {output_padding}, stride "
                         f"{stride}, dilation {dilation}")
    OH = _hip.mx_conv_transpose_out_size(H, KH, stride[0], padding[0], dilation[0], output_padding[0])
    OW = _hip.mx_conv_transpose_out_size(W, KW, stride[1], padding[1], dilation[1], output_padding[1])
    if OH < 1 or OW < 1:
        raise ValueError(f"the padding {padding} crops the whole output of the image {H}x{W} under the kernel {KH}x{KW} (stride {stride}, "
                         f"dilation {dilation}): the output would be {OH}x{OW}")
    if x_codes.is_cuda:
        return _hip.mx_conv_transpose2d(x_codes.contiguous(), x_scales.contiguous(), x_fmt, w_codes.contiguous(), w_scales.contiguous(),
                                        w_fmt, None if bias is None else bias.contiguous(), stride, padding, output_padding, dilation,
                                        out_dtype)
    x = mx_dequantize(x_codes, x_scales, x_fmt, -1, torch.float64).permute(0, 3, 1, 2)
    w = mx_dequantize(w_codes, w_scales, w_fmt, -1, torch.float64).permute(0, 3, 1, 2)
    # zeros between the pixels, the flipped kernel at full padding d (k - 1) cropped by p and extended by the output padding.  The
    # padding is written out, so that every output sums all of its taps: a 0xFF block is NaN also against a zero (NaN * 0 is NaN)
    z = x.new_zeros(B, C, (H - 1) * stride[0] + 1, (W - 1) * stride[1] + 1)
    z[:, :, ::stride[0], ::stride[1]] = x
    full = (dilation[0] * (KH - 1), dilation[1] * (KW - 1))
    z = F.pad(z, (full[1] - padding[1], full[1] - padding[1] + output_padding[1], full[0] - padding[0], full[0] - padding[0] + output_padding[0]))
    y = F.conv2d(z, w.flip(2, 3), None if bias is None else bias.to(torch.float64), 1, 0, dilation)
    return y.permute(0, 2, 3, 1).to(out_dtype).contiguous()


def mx_conv2d_input_grad(dy_codes: torch.Tensor, dy_scales: torch.Tensor, dy_fmt: str, wt_codes: torch.Tensor, wt_scales: torch.Tensor,
                         w_fmt: str, input_size, stride=1, padding=0, dilation=1, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The input gradient ``dx [B, H, W, Cin]`` of ``conv2d(x, w, stride, padding, dilation)`` (``groups == 1``) on MX codes:
    ``dy_codes [B, OH, OW, Cout]`` / ``dy_scales`` are the output gradient quantized along its channels
    (``quantize_with_mx(dy_channels_last, fmt, -1, return_codes=True)``), ``wt_codes [Cin, KH, KW, Cout]`` / ``wt_scales [Cin, KH, KW,
    ceil(Cout / 32)]`` the weight ``[Cout, Cin, KH, KW].permute(1, 2, 3, 0)`` with blocks along ``Cout``, ``input_size = (H, W)`` the
    extent of the convolution's input.  It is ``mx_conv_transpose2d`` with the output padding that ``input_size`` implies -- the rows
    and columns of ``x`` that no window reaches get a zero gradient -- and has no kernel of its own."""
    _check_operand("dy", dy_codes, dy_scales, dy_fmt, "[B, OH, OW, Cout]")
    _check_operand("wt", wt_codes, wt_scales, w_fmt, "[Cin, KH, KW, Cout]")
    H, W = _pair("input_size", input_size, 1)
    stride, padding, dilation = _pair("stride", stride, 1), _pair("padding", padding, 0), _pair("dilation", dilation, 1)
    (KH, KW), out_pad = wt_codes.shape[1:3], []
    for n, got, k, s, p, d in zip((H, W), dy_codes.shape[1:3], (KH, KW), stride, padding, dilation):
        want = _hip.mx_conv_out_size(n, k, s, p, d)
        if got != want:
            raise ValueError(f"dy_codes {tuple(dy_codes.shape)} is not the gradient of a convolution of an input {H}x{W} with the kernel "
                             f"{KH}x{KW} (stride {stride}, padding {padding}, dilation {dilation}): its output is "
                             f"{_hip.mx_conv_out_size(H, KH, stride[0], padding[0], dilation[0])}x"
                             f"{_hip.mx_conv_out_size(W, KW, stride[1], padding[1], dilation[1])}")
        out_pad.append(n - _hip.mx_conv_transpose_out_size(got, k, s, p, d, 0))       # the remainder of the forward's division: < s
    return mx_conv_transpose2d(dy_codes, dy_scales, dy_fmt, wt_codes, wt_scales, w_fmt, None, stride, padding, tuple(out_pad), dilation,
                               out_dtype)


class MXConvTranspose2d(_MXConvBase):
    """``nn.ConvTranspose2d`` (``groups == 1``, zero padding) for inference on MX codes: the weight is held channels-last as uint8
    codes ``weight_codes [Cout, KH, KW, C]`` and E8M0 scales ``weight_scales [Cout, KH, KW, ceil(C / 32)]`` of the format
    ``weight_fmt`` (buffers, with the optional float32 ``bias``).  ``forward`` takes ``[B, C, H, W]`` in float32 / bfloat16 / float16,
    quantizes it to ``act_fmt`` along the channels with the MX quantizer and runs ``mx_conv_transpose2d`` on the two sets of codes;
    it returns a ``torch.channels_last`` ``[B, Cout, OH, OW]`` tensor in ``out_dtype`` that never requires grad.  An input that
    requires grad while gradients are enabled is refused -- training runs on the simulated layers this one is built from.  As for
    ``MXConv2d``, a ``torch.channels_last`` input is quantized where it lies; an NCHW-contiguous one pays one layout pass."""

    _layer, _weight_layout, _perm, _block_dim = nn.ConvTranspose2d, "[C, Cout, KH, KW]", (1, 2, 3, 0), 0
    _block_dim_note = "dim 0 of a transposed convolution's weight"

    def __init__(self, weight_codes: torch.Tensor, weight_scales: torch.Tensor, weight_fmt: str, bias: Optional[torch.Tensor] = None,
                 stride=1, padding=0, output_padding=0, dilation=1, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32):
        super().__init__(weight_codes, weight_scales, weight_fmt, bias, stride, padding, dilation, act_fmt, out_dtype)
        self.output_padding = _pair("output_padding", output_padding, 0)

    def _extra_field(self) -> str:
        return f"output_padding={self.output_padding}, "

    @classmethod
    def from_exported(cls, qt, bias: Optional[torch.Tensor] = None, stride=1, padding=0, output_padding=0, dilation=1,
                      act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32):
        """from the ``QuantizedTensor(kind="mx")`` ``export_integer`` returns for a transposed conv layer's weight ``[C, Cout, KH,
        KW]`` with blocks along dim 0; codes and scales are permuted to channels-last once, here"""
        return cls(*cls._channels_last(qt), qt.fmt, bias, stride, padding, output_padding, dilation, act_fmt, out_dtype)

    @classmethod
    def from_quantized(cls, layer: nn.Module, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32):
        """from a ``quantize(nn.ConvTranspose2d(...), bits=w, callback=MXQuantizer(fmt, block_dim=0))`` layer that is past its
        timeout: the weight codes are the export's, stride / padding / output padding / dilation and the bias the layer's"""
        from qsparse_amd.export import export_integer
        q = layer.__dict__.get("_modules", {}).get("quantize")
        if not isinstance(layer, nn.ConvTranspose2d) or q is None or not isinstance(q.callback, MXQuantizer):
            raise ValueError("MXConvTranspose2d.from_quantized needs an nn.ConvTranspose2d wrapped by quantize(..., callback=MXQuantizer(...))")
        if layer.groups != 1:
            raise ValueError(f"MXConvTranspose2d supports groups == 1 only, the layer has groups={layer.groups}")
        if layer.padding_mode != "zeros":
            raise ValueError(f"MXConvTranspose2d supports zero padding only, the layer has padding_mode={layer.padding_mode!r}")
        rec = export_integer(nn.Sequential(layer)).get("0")
        if rec is None or rec.weight is None:
            raise ValueError("the layer has not quantized its weight yet (still inside its timeout): nothing to build an MXConvTranspose2d from")
        b = layer.bias
        bias = None if b is None else b.detach().to(torch.float32)
        return cls.from_exported(rec.weight, bias, tuple(layer.stride), tuple(layer.padding), tuple(layer.output_padding),
                                 tuple(layer.dilation), act_fmt, out_dtype)

    def _product(self, codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
        return mx_conv_transpose2d(codes, scales, self.act_fmt, self.weight_codes, self.weight_scales, self.weight_fmt, self.bias,
                                   self.stride, self.padding, self.output_padding, self.dilation, self.out_dtype)


__all__ = ["mx_conv_transpose2d", "mx_conv2d_input_grad", "MXConvTranspose2d", "MX_FORMATS"]
