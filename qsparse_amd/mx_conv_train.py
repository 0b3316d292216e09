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
below 32 pads its block with zero codes: ``B = 8`` spends 3/4 of the products on zeros."""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from qsparse_amd import _hip
from qsparse_amd.mx_conv import MXConv2d, _pair, mx_conv2d
from qsparse_amd.mx_conv_transpose import mx_conv2d_input_grad
from qsparse_amd.mx_gemm import _OUT_DTYPES, _split_request, mx_quantize_2way
from qsparse_amd.quantize import MX_BLOCK, MX_FORMATS, _mx_check_rounding, _mx_format, mx_dequantize, quantize_with_mx


def _check_batch_operand(name: str, what: str, codes: torch.Tensor, scales: torch.Tensor, fmt: str):
    _mx_format(fmt)
    for label, t in ((f"{name}_codes", codes), (f"{name}_scales", scales)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{label} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.uint8:
            raise TypeError(f"{label} must be uint8 (the bytes mx_quantize_2way returns), got {t.dtype}")
    if codes.dim() != 4:
        raise ValueError(f"{name}_codes needs 4 dimensions {what}, got shape {tuple(codes.shape)}")
    B = codes.shape[-1]
    want = tuple(codes.shape[:-1]) + ((B + MX_BLOCK - 1) // MX_BLOCK,)
    if tuple(scales.shape) != want:
        raise ValueError(f"{name}_scales has shape {tuple(scales.shape)}, expected {want}: one E8M0 byte per block of {MX_BLOCK} "
                         f"along the last dimension (the batch) of {name}_codes {tuple(codes.shape)}")
    if scales.device != codes.device:
        raise ValueError(f"{name}_codes is on {codes.device} but {name}_scales on {scales.device}")


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
    _check_batch_operand("dyt", "[OH, OW, Cout, B]", dyt_codes, dyt_scales, dy_fmt)
    _check_batch_operand("xt", "[H, W, C, B]", xt_codes, xt_scales, x_fmt)
    (OH, OW, Cout, B), (H, W, C, Bx) = dyt_codes.shape, xt_codes.shape
    if Bx != B:
        raise ValueError(f"dyt_codes {tuple(dyt_codes.shape)} and xt_codes {tuple(xt_codes.shape)} disagree on B (their last dimensions)")
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"mx_conv2d_weight_grad needs B, H, W >= 1, got dyt_codes {tuple(dyt_codes.shape)}, xt_codes {tuple(xt_codes.shape)}")
    if xt_codes.device != dyt_codes.device:
        raise ValueError(f"dyt_codes is on {dyt_codes.device} but xt_codes on {xt_codes.device}")
    if out_dtype not in _OUT_DTYPES:
        raise TypeError(f"out_dtype must be one of {_OUT_DTYPES}, got {out_dtype}")
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
        ctx.fmts = (x_fmt, w_fmt, grad_fmt)
        # `step` is advanced in place by the backward: an attribute, not a saved tensor (no version check, nothing to differentiate)
        ctx.sr = (grad_rounding, seed, step)
        ctx.wgrad_split_k = wgrad_split_k
        ctx.x_size, ctx.x_dtype = tuple(x.shape[2:]), x.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
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
            # the two forms of dy alone take `grad_rounding` (blocks along Cout: stream 0, for dx; along B: stream 1, for dW); after
            # a stochastic one the counter moves on, on the stream: the next backward -- or the next replay of this one -- draws new words
            rounding, seed, step = ctx.sr
            g_codes, g_scales, g_col, g_cs = _row_and_col(dyl, grad_fmt, need_dx, need_dw, rounding, seed, step)
            if rounding == "stochastic" and step is not None:
                step.add_(1)
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
    _split_request(wgrad_split_k, "wgrad_split_k")
    for fmt in (x_fmt, w_fmt, grad_fmt):
        _mx_format(fmt)
    for name, t in (("x", x), ("weight", weight)) + ((("bias", bias),) if bias is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype not in _OUT_DTYPES:
            raise TypeError(f"{name} must be one of {_OUT_DTYPES}, got {t.dtype}")
        if t.device != x.device:
            raise ValueError(f"x is on {x.device} but {name} on {t.device}")
    _mx_check_rounding(grad_rounding, step, x)
    if weight.dim() != 4:
        raise ValueError(f"weight must be [Cout, C, KH, KW], got shape {tuple(weight.shape)}")
    if x.dim() != 4 or x.shape[1] != weight.shape[1]:
        raise ValueError(f"x {tuple(x.shape)} must be [B, C, H, W] with the C of weight {tuple(weight.shape)}")
    if x.shape[0] < 1 or min(weight.shape) < 1:
        raise ValueError(f"mx_conv2d_train needs B, Cout, C, KH, KW >= 1, got x {tuple(x.shape)}, weight {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"bias has shape {tuple(bias.shape)}, expected ({weight.shape[0]},)")
    stride, padding, dilation = _pair("stride", stride, 1), _pair("padding", padding, 0), _pair("dilation", dilation, 1)
    need_col = torch.is_grad_enabled() and weight.requires_grad
    return _MXConv2dFunction.apply(x, weight, bias, stride, padding, dilation, x_fmt, w_fmt, grad_fmt, need_col, grad_rounding, seed, step,
                                   wgrad_split_k)


class MXTrainConv2d(nn.Conv2d):
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
        for fmt in (x_fmt, w_fmt, grad_fmt):
            _mx_format(fmt)
        _mx_check_rounding(grad_rounding, None, self.weight)
        _split_request(wgrad_split_k, "wgrad_split_k")
        self.wgrad_split_k = wgrad_split_k
        self.x_fmt, self.w_fmt, self.grad_fmt, self.grad_rounding = x_fmt, w_fmt, grad_fmt, grad_rounding
        if grad_rounding == "stochastic":
            self.sr_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if seed is None else int(seed)
            self.register_buffer("sr_step", torch.zeros(1, dtype=torch.int64, device=self.weight.device), persistent=False)

    @classmethod
    def from_conv(cls, layer: nn.Conv2d, x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2",
                  grad_rounding: str = "nearest", seed: Optional[int] = None, wgrad_split_k="auto"):
        """a layer on ``layer``'s own parameters (shared, not copied)"""
        if not isinstance(layer, nn.Conv2d):
            raise TypeError(f"MXTrainConv2d.from_conv needs an nn.Conv2d, got {type(layer).__name__}")
        new = cls(layer.in_channels, layer.out_channels, layer.kernel_size, layer.stride, layer.padding, layer.dilation, layer.groups,
                  layer.bias is not None, layer.padding_mode, device="meta", x_fmt=x_fmt, w_fmt=w_fmt, grad_fmt=grad_fmt,
                  grad_rounding=grad_rounding, seed=seed, wgrad_split_k=wgrad_split_k)
        new.weight, new.bias = layer.weight, layer.bias
        if grad_rounding == "stochastic":
            new.sr_step = torch.zeros(1, dtype=torch.int64, device=layer.weight.device)
        new.train(layer.training)
        return new

    def extra_repr(self) -> str:
        sr = f", grad_rounding={self.grad_rounding!r}" if self.grad_rounding != "nearest" else ""
        split = f", wgrad_split_k={self.wgrad_split_k!r}" if self.wgrad_split_k != "auto" else ""
        return f"{super().extra_repr()}, x_fmt={self.x_fmt!r}, w_fmt={self.w_fmt!r}, grad_fmt={self.grad_fmt!r}{sr}{split}"

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        dev = x.device.type
        if torch.is_autocast_enabled(dev):
            x = x.to(torch.get_autocast_dtype(dev))
        seed, step = (self.sr_seed, self.sr_step) if self.grad_rounding == "stochastic" else (0, None)
        return mx_conv2d_train(x, self.weight, self.bias, self.stride, self.padding, self.dilation, self.x_fmt, self.w_fmt, self.grad_fmt,
                               self.grad_rounding, seed, step, self.wgrad_split_k)

    def to_inference(self, act_fmt: Optional[str] = None, out_dtype: torch.dtype = torch.float32) -> MXConv2d:
        """the ``MXConv2d`` on the current weight: its weight bytes are the codes the training forward convolves with"""
        codes, scales = _weight_rows(self.weight.detach().permute(0, 2, 3, 1), self.w_fmt)
        return MXConv2d(codes, scales, self.w_fmt, None if self.bias is None else self.bias.detach(), self.stride, self.padding,
                        self.dilation, act_fmt or self.x_fmt, out_dtype)


__all__ = ["mx_conv2d_weight_grad", "mx_conv2d_train", "MXTrainConv2d", "MX_FORMATS"]
