"""Training through convolutions on MX codes: ``mx_conv2d_weight_grad`` (the weight gradient, wgrad), ``mx_conv2d_train`` (a
differentiable ``conv2d`` whose three products run on MX codes) and the layer ``MXTrainConv2d`` -- the counterparts of ``mx_matmul``'s
weight-gradient use, ``mx_linear`` and ``MXTrainLinear`` for ``nn.Conv2d``.

The weight gradient contracts over ``(b, oh, ow)``.  Its operands carry their MX blocks of 32 along the BATCH: a block of 32 images
at one pixel and channel is the same 32 numbers under every tap ``(kh, kw)``, so ``x`` and ``dy`` are each quantized once and serve
all taps -- blocks along the output pixels would map to other pixels of ``x`` for every tap.  The operands are the column pair of
``mx_quantize_2way`` on the channels-last tensor seen as ``[B, H W C]``: ``xt_codes [H, W, C, B]``, ``xt_scales [H, W, C, ceil(B /
32)]``.  When the channel count is a multiple of 32 the row pair of the same call is, bit for bit, the forward (``mx_conv2d``) or
input-gradient (``mx_conv2d_input_grad``) operand, since a block of 32 along the flat ``H W C`` axis is then a block along ``C``.
On the GPU the product is one HIP kernel (``qs_mx_conv2d_wgrad_v``): an implicit GEMM on the block-scaled MFMA of gfx950, split
along the contraction into slices that are added in a fixed order; on the CPU the definition is evaluated in float64.  A batch
below 32 pads its block with zero codes: ``B = 8`` spends 3/4 of the products on zeros.  What the layer and its autograd function
share with ``MXTrainLinear`` -- options, counter, ``repr``, the quantization of ``dy`` -- is ``_mx_common.py``'s."""
from functools import partial
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from qsparse_amd import _hip, _mx_common
from qsparse_amd._mx_common import (_check_bias_shape, _check_dtype, _check_train_entry, _MXTrainMixin, _pair,
                                    _quantize_grad, _save_train_ctx, _split_request)
from qsparse_amd.mx_conv import MXConv2d, mx_conv2d
from qsparse_amd.mx_conv_transpose import mx_conv2d_input_grad
from qsparse_amd.mx_gemm import mx_quantize_2way
from qsparse_amd.quantize import MX_BLOCK, MX_FORMATS, mx_dequantize, quantize_with_mx


# an operand with blocks along the batch, its last axis
_check_batch_operand = partial(_mx_common._check_operand, source="mx_quantize_2way", axis=" (the batch)")


def mx_conv2d_weight_grad(dyt_codes: torch.Tensor, dyt_scales: torch.Tensor, dy_fmt: str, xt_codes: torch.Tensor, xt_scales: torch.Tensor,
                          x_fmt: str, kernel_size, stride=1, padding=0, dilation=1, out_dtype: torch.dtype = torch.float32,
                          split_k="auto") -> torch.Tensor:
    """The weight gradient ``dW [Cout, KH, KW, C]`` of ``conv2d(x, w, stride, padding, dilation)`` (``groups == 1``) on MX codes with
    blocks of 32 along the batch.  ``dyt_codes [OH, OW, Cout, B]`` / ``dyt_scales [OH, OW, Cout, ceil(B / 32)]`` are the output
    gradient, ``xt_codes [H, W, C, B]`` / ``xt_scales [H, W, C, ceil(B / 32)]`` the convolution's input -- the column pairs of
    ``mx_quantize_2way(t.view(B, -1), None, fmt)`` for the channels-last ``t [B, ., ., .]`` -- in the formats ``dy_fmt`` / ``x_fmt``
    (``MX_FORMATS``; they may differ); ``kernel_size`` is ``(KH, KW)``; ``stride``, ``padding`` (zeros) and ``dilation`` an int or a pair
    each.  Returns a contiguous tensor in ``out_dtype`` (float32, bfloat16 or float16):

        dW[n, kh, kw, c] = round( sum_{oh, ow, b} val(dyt[oh, ow, n, b]) 2^(sg[oh, ow, n, b / 32] - 127)
                                                * val(xt[ih, iw, c, b])  2^(sx[ih, iw, c, b / 32] - 127) )
        ih = oh * stride_h - pad_h + kh * dil_h,    iw = ow * stride_w - pad_w + kw * dil_w

    a tap outside the image contributes zero.  A scale byte 0xFF of ``dyt`` at channel ``n`` makes ``dW[n]`` NaN everywhere; one of
    ``xt`` at ``(ih, iw, c)`` makes ``dW[:, kh, kw, c]`` NaN for exactly the taps through which some output pixel reads ``(ih, iw)``.

    GPU tensors take the HIP kernel: float32 accumulation in the order of ``mx_matmul(G, SG, dy_fmt, X', SX', x_fmt, split_k=S)`` on
    the gathered operands ``G [Cout, OH OW Bp]``, ``X' [KH KW C, OH OW Bp]`` (``k' = (oh OW + ow) Bp + b``, ``Bp = 32 ceil(B / 32)``), to
    which the result is bit-identical; no gathered matrix is written and there is no fallback: without the library the call raises.
    ``split_k`` (an int ``>= 1`` or ``"auto"``) is ``mx_matmul``'s: that many slices of the contraction run side by side and their
    float32 partial sums are added in ascending order -- the result is a pure function of the operands and ``split_k``.  ``"auto"``
    (the default) lets the library choose from the shape; this product has few output tiles and a long contraction, so it usually
    splits.  CPU tensors evaluate the expression above in float64 and round once; ``split_k`` is checked and has no order to cut.
    A batch below 32 pads its block with zero codes and spends the rest of the block's products on them."""
    request = _split_request(split_k)
    _check_batch_operand("dyt", dyt_codes, dyt_scales, dy_fmt, "[OH, OW, Cout, B]")
    _check_batch_operand("xt", xt_codes, xt_scales, x_fmt, "[H, W, C, B]")
    (OH, OW, Cout, B), (H, W, C, Bx) = dyt_codes.shape, xt_codes.shape
    if Bx != B:
        raise ValueError(f"dyt_codes {tuple(dyt_codes.shape)} and xt_codes {tuple(xt_codes.shape)} disagree on B (their last dimensions)")
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"mx_conv2d_weight_grad needs B, H, W >= 1, got dyt_codes {tuple(dyt_codes.shape)}, xt_codes {tuple(xt_codes.shape)}")
    if xt_codes.device != dyt_codes.device:
        raise ValueError(f"dyt_codes is on {dyt_codes.device} but xt_codes on {xt_codes.device}")
    _check_dtype("out_dtype", out_dtype)
    KH, KW = _pair("kernel_size", kernel_size, 1)
    stride, padding, dilation = _pair("stride", stride, 1), _pair("padding", padding, 0), _pair("dilation", dilation, 1)
    want = tuple(_hip.mx_conv_out_size(n, k, s, p, d) for n, k, s, p, d in zip((H, W), (KH, KW), stride, padding, dilation))
    if (OH, OW) != want:
        raise ValueError(f"dyt_codes {tuple(dyt_codes.shape)} is not the gradient of a convolution of an input {H}x{W} with the kernel "
                         f"{KH}x{KW} (stride {stride}, padding {padding}, dilation {dilation}): its output is {want[0]}x{want[1]}")
    if dyt_codes.is_cuda:
        return _hip.mx_conv2d_wgrad(dyt_codes.contiguous(), dyt_scales.contiguous(), dy_fmt, xt_codes.contiguous(), xt_scales.contiguous(),
                                    x_fmt, (KH, KW), stride, padding, dilation, out_dtype, request)
    dy = mx_dequantize(dyt_codes, dyt_scales, dy_fmt, -1, torch.float64).permute(3, 2, 0, 1)        # [B, Cout, OH, OW]
    x = mx_dequantize(xt_codes, xt_scales, x_fmt, -1, torch.float64).permute(3, 2, 0, 1)            # [B, C, H, W]
    # the padding is written out and every window unfolded, so that every element of dW sums all of its (oh, ow, b): a 0xFF block is
    # NaN also against a zero (NaN * 0 is NaN) -- matmul's own propagation
    x = F.pad(x, (padding[1], padding[1], padding[0], padding[0]))
    cols = F.unfold(x, (KH, KW), dilation, 0, stride)                                               # [B, C KH KW, OH OW]
    dw = dy.reshape(B, Cout, OH * OW).permute(1, 0, 2).reshape(Cout, -1) @ cols.permute(0, 2, 1).reshape(-1, C * KH * KW)
    return dw.reshape(Cout, C, KH, KW).permute(0, 2, 3, 1).to(out_dtype).contiguous()


def _channels_last_view(t: torch.Tensor) -> torch.Tensor:
    """`t [B, C, H, W]` as a contiguous `[B, H, W, C]`: a view of a ``torch.channels_last`` tensor, one layout pass over any other"""
    return t.permute(0, 2, 3, 1).contiguous()


def _row_and_col(t: torch.Tensor, fmt: str, want_row: bool, want_col: bool, rounding: str = "nearest", seed: int = 0, step=None):
    """the two MX forms of a contiguous channels-last `t [B, H, W, C]`: (codes [B, H, W, C], scales [B, H, W, ceil(C / 32)]) with blocks
    along C and (codes [H, W, C, B], scales [H, W, C, ceil(B / 32)]) with blocks along B; a form that is not wanted is (None, None).
    One `mx_quantize_2way` call on `t.view(B, -1)` yields both when C % 32 == 0 -- a block of 32 along H W C is then a block along C;
    otherwise the row form is the one-way quantizer's and the column form a column-only two-way call.  With stochastic rounding the
    row form draws its words on stream 0 and the column form on stream 1 either way."""
    B, H, W, C = t.shape
    t2 = t.view(B, H * W * C)
    rc = rs = cc = cs = None
    if C % MX_BLOCK == 0:
        rc, rs, cc, cs = mx_quantize_2way(t2, fmt if want_row else None, fmt if want_col else None, rounding, seed, step)
        if want_row:
            rc, rs = rc.view(B, H, W, C), rs.view(B, H, W, C // MX_BLOCK)
    else:
        if want_row:
            _, rc, rs = quantize_with_mx(t, fmt, -1, return_codes=True, rounding=rounding, seed=seed, step=step, stream=0)
        if want_col:
            _, _, cc, cs = mx_quantize_2way(t2, None, fmt, rounding, seed, step)
    if want_col:
        cc, cs = cc.view(H, W, C, B), cs.view(H, W, C, -1)
    return rc, rs, cc, cs


def _weight_rows(w: torch.Tensor, fmt: str):
    """codes and scales of a 4-d `w [N, ., ., K]` with blocks along its last axis (any K: every (n, ., .) is a row of its own)"""
    N, A, Bk, K = w.shape
    codes, scales, _, _ = mx_quantize_2way(w.reshape(N * A * Bk, K), fmt, None)
    return codes.view(N, A, Bk, K), scales.view(N, A, Bk, -1)


class _MXConv2dFunction(torch.autograd.Function):
    """y = conv(Q(x), Q(W)) + b, dx = conv_transpose(Q(dy), Q(W)), dW = wgrad(Q(dy^T), Q(x^T)) on MX codes; every quantizer
    straight-through"""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, dilation, x_fmt, w_fmt, grad_fmt, need_col, grad_rounding="nearest", seed=0,
                step=None, wgrad_split_k="auto"):
        # `need_col`: a weight gradient can be asked for -- decided by mx_conv2d_train, where the grad mode is still the caller's
        xl = _channels_last_view(x.detach())
        x_codes, x_scales, x_col, x_cs = _row_and_col(xl, x_fmt, True, need_col)
        w_codes, w_scales = _weight_rows(weight.detach().permute(0, 2, 3, 1), w_fmt)
        b32 = None if bias is None else bias.detach().to(torch.float32)
        y = mx_conv2d(x_codes, x_scales, x_fmt, w_codes, w_scales, w_fmt, b32, stride, padding, dilation, x.dtype)
        # the weight itself (autograd's version counter guards it), and x as its batch-blocked codes: 1 + 1/32 bytes per element
        ctx.save_for_backward(weight, x_col, x_cs)
        ctx.geometry = (stride, padding, dilation)
        _save_train_ctx(ctx, (x_fmt, w_fmt, grad_fmt), (grad_rounding, seed, step), wgrad_split_k, x, bias)
        ctx.x_size = tuple(x.shape[2:])
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        weight, x_col, x_cs = ctx.saved_tensors
        x_fmt, w_fmt, grad_fmt = ctx.fmts
        stride, padding, dilation = ctx.geometry
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        dyl = _channels_last_view(dy)
        dx = dw = db = None
        if need_dx or need_dw:
            # blocks along Cout for dx, along B for dW
            g_codes, g_scales, g_col, g_cs = _quantize_grad(ctx, lambda *sr: _row_and_col(dyl, grad_fmt, need_dx, need_dw, *sr))
        if need_dx:
            wt_codes, wt_scales = _weight_rows(weight.permute(1, 2, 3, 0), w_fmt)
            dx = mx_conv2d_input_grad(g_codes, g_scales, grad_fmt, wt_codes, wt_scales, w_fmt, ctx.x_size, stride, padding, dilation,
                                      ctx.x_dtype).permute(0, 3, 1, 2)
        if need_dw:
            dw = mx_conv2d_weight_grad(g_col, g_cs, grad_fmt, x_col, x_cs, x_fmt, tuple(weight.shape[2:]), stride, padding, dilation,
                                       weight.dtype, ctx.wgrad_split_k).permute(0, 3, 1, 2)
        if need_db:
            db = dyl.sum((0, 1, 2), dtype=torch.float32).to(ctx.bias_dtype)
        return (dx, dw, db) + (None,) * 11


def mx_conv2d_train(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, stride=1, padding=0, dilation=1,
                    x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest",
                    seed: int = 0, step: Optional[torch.Tensor] = None, wgrad_split_k="auto") -> torch.Tensor:
    """``F.conv2d`` (``groups == 1``, zero padding) whose three products run on MX codes, differentiable in ``x``, ``weight`` and
    ``bias``.  ``x`` is ``[B, C, H, W]`` (``B >= 1``) in float32 / bfloat16 / float16, ``weight`` ``[Cout, C, KH, KW]`` and ``bias``
    ``[Cout]`` in any of the three; the result is a ``torch.channels_last`` ``[B, Cout, OH, OW]`` in ``x.dtype``.  With ``Q_f(t; a)`` the
    MX quantization of ``t`` in format ``f`` with blocks of 32 along its axis ``a`` and ``dy`` the incoming gradient:

        y  = mx_conv2d(Q_x(x; C), Q_w(W; C)) + bias
        dx = mx_conv2d_input_grad(Q_g(dy; Cout), Q_w(W; Cout))
        dW = mx_conv2d_weight_grad(Q_g(dy; B), Q_x(x; B))
        db = sum over (b, oh, ow) of dy (float32)

    -- the straight-through rule of ``quantize_with_mx`` applied to all six quantizers.  The operands come from ``mx_quantize_2way``
    on the channels-last tensor seen as ``[B, H W C]``: when the channel count is a multiple of 32 one call yields both forms (its
    row pair has blocks along C, its column pair along B); otherwise the C form is the one-way quantizer's and the B form a
    column-only call.  The backward keeps ``weight`` and ``Q_x(x; B)`` only: 1 + 1/32 bytes per element of ``x``.  Gradients nobody
    asks for are not computed, and without grad ``Q_x(x; B)`` is not either.  GPU tensors run HIP kernels only (no host
    synchronisation: a step can be graph-captured); CPU tensors evaluate the same formulas in float64.

    Memory format: a ``torch.channels_last`` ``x`` (and ``dy``) is quantized where it lies; an NCHW-contiguous one pays one layout
    pass over the tensor first.  Keep the network channels_last to avoid it.

    ``grad_rounding="stochastic"`` rounds the two forms of ``dy`` -- and nothing else -- stochastically, the Cout form on stream 0 and
    the B form on stream 1, as ``mx_linear`` does; ``step`` (a one-element int64 tensor on ``x``'s device, or None) is part of the key
    and is advanced by one in place after each backward that quantizes ``dy``.

    ``wgrad_split_k`` (an int ``>= 1`` or ``"auto"``) is ``mx_conv2d_weight_grad``'s ``split_k``; ``y`` and ``dx`` are untouched by it.
    A batch below 32 pads the weight gradient's blocks with zero codes (``B = 8``: 3/4 of its products)."""
    _check_train_entry(x, weight, bias, (x_fmt, w_fmt, grad_fmt), grad_rounding, step, wgrad_split_k)
    if weight.dim() != 4:
        raise ValueError(f"weight must be [Cout, C, KH, KW], got shape {tuple(weight.shape)}")
    if x.dim() != 4 or x.shape[1] != weight.shape[1]:
        raise ValueError(f"x {tuple(x.shape)} must be [B, C, H, W] with the C of weight {tuple(weight.shape)}")
    if x.shape[0] < 1 or min(weight.shape) < 1:
        raise ValueError(f"mx_conv2d_train needs B, Cout, C, KH, KW >= 1, got x {tuple(x.shape)}, weight {tuple(weight.shape)}")
    _check_bias_shape(bias, weight.shape[0])
    stride, padding, dilation = _pair("stride", stride, 1), _pair("padding", padding, 0), _pair("dilation", dilation, 1)
    need_col = torch.is_grad_enabled() and weight.requires_grad
    return _MXConv2dFunction.apply(x, weight, bias, stride, padding, dilation, x_fmt, w_fmt, grad_fmt, need_col, grad_rounding, seed, step,
                                   wgrad_split_k)


class MXTrainConv2d(_MXTrainMixin, nn.Conv2d):
    """Drop-in ``nn.Conv2d`` (``groups == 1``, zero padding given as numbers) that trains through MX products: float ``weight`` /
    ``bias`` parameters (``nn.Conv2d``'s own ``state_dict``), ``forward`` is ``mx_conv2d_train`` in the formats ``x_fmt`` / ``w_fmt`` /
    ``grad_fmt``.  Under ``torch.autocast`` the input is cast to the autocast dtype, as ``nn.Conv2d``'s would be, and the output has
    that dtype.  The output is ``torch.channels_last``; an NCHW-contiguous input pays one layout pass.

    ``grad_rounding="stochastic"`` rounds the gradient operands stochastically (``mx_conv2d_train``).  The layer then owns
    ``sr_seed`` -- ``seed``, or a draw from torch's default CPU generator when that is None -- and a non-persistent int64 buffer
    ``sr_step`` that counts its backwards on the device.  With ``"nearest"`` neither exists and the ``state_dict`` is ``nn.Conv2d``'s.

    ``wgrad_split_k`` is ``mx_conv2d_train``'s: ``"auto"`` (the default) lets the library split the weight-gradient product where
    that fills the GPU, which changes ``weight.grad`` in float32 summation order only, deterministically."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride=1, padding=0, dilation=1, groups: int = 1,
                 bias: bool = True, padding_mode: str = "zeros", device=None, dtype=None, x_fmt: str = "mxfp8_e4m3",
                 w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest", seed: Optional[int] = None,
                 wgrad_split_k="auto"):
        if groups != 1:
            raise ValueError(f"MXTrainConv2d supports groups == 1 only, the layer has groups={groups}")
        if padding_mode != "zeros":
            raise ValueError(f"MXTrainConv2d supports zero padding only, the layer has padding_mode={padding_mode!r}")
        if isinstance(padding, str):
            raise ValueError(f"MXTrainConv2d needs the padding as numbers, the layer has padding={padding!r}")
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device=device,
                         dtype=dtype)
        self._init_mx(dict(x_fmt=x_fmt, w_fmt=w_fmt, grad_fmt=grad_fmt), grad_rounding, seed)
        self._init_split(wgrad_split_k)

    @classmethod
    def from_conv(cls, layer: nn.Conv2d, x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2",
                  grad_rounding: str = "nearest", seed: Optional[int] = None, wgrad_split_k="auto"):
        """a layer on ``layer``'s own parameters (shared, not copied)"""
        if not isinstance(layer, nn.Conv2d):
            raise TypeError(f"MXTrainConv2d.from_conv needs an nn.Conv2d, got {type(layer).__name__}")
        return cls(layer.in_channels, layer.out_channels, layer.kernel_size, layer.stride, layer.padding, layer.dilation, layer.groups,
                   layer.bias is not None, layer.padding_mode, device="meta", x_fmt=x_fmt, w_fmt=w_fmt, grad_fmt=grad_fmt,
                   grad_rounding=grad_rounding, seed=seed, wgrad_split_k=wgrad_split_k)._adopt(layer)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x, seed, step = self._mx_input(x)
        return mx_conv2d_train(x, self.weight, self.bias, self.stride, self.padding, self.dilation, self.x_fmt, self.w_fmt, self.grad_fmt,
                               self.grad_rounding, seed, step, self.wgrad_split_k)

    def to_inference(self, act_fmt: Optional[str] = None, out_dtype: torch.dtype = torch.float32, *, out_fmt: Optional[str] = None,
                     act: Optional[str] = None) -> MXConv2d:
        """the ``MXConv2d`` on the current weight: its weight bytes are the codes the training forward convolves with"""
        codes, scales = _weight_rows(self.weight.detach().permute(0, 2, 3, 1), self.w_fmt)
        return MXConv2d(codes, scales, self.w_fmt, None if self.bias is None else self.bias.detach(), self.stride, self.padding,
                        self.dilation, act_fmt or self.x_fmt, out_dtype, out_fmt=out_fmt, act=act)


__all__ = ["mx_conv2d_weight_grad", "mx_conv2d_train", "MXTrainConv2d", "MX_FORMATS"]
