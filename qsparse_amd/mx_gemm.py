"""Matrix products on MX codes: ``mx_matmul`` and the inference-side layer ``MXLinear``.

``quantize_with_mx(..., block_dim=-1, return_codes=True)`` and ``export_integer`` hand out the bytes of an MX tensor -- one code
per element, one E8M0 scale per block of 32 along K.  ``mx_matmul`` computes ``A . B^T`` directly on those bytes: on the GPU
through the block-scaled MFMA of gfx950 (``qs_mx_matmul_v``: FP8 / FP6 / FP4 operands of either format on either side, float32
accumulation), on the CPU by evaluating the definition in float64.  ``MXLinear`` is what a simulated layer
(``quantize(nn.Linear(...), callback=MXQuantizer(...))``) becomes for inference.

Training through the product: ``mx_linear`` / ``MXTrainLinear`` run all three matrix products of a linear layer's step -- forward,
input gradient, weight gradient -- through ``mx_matmul``; their operands come from ``mx_quantize_2way``, which reads a tensor once
and writes its codes with blocks along the rows and, transposed, with blocks along the columns (``qs_mx_quant2_v``).  The argument
checks and the layer's options, counter and ``repr`` are ``_mx_common.py``'s, shared with the convolutions."""
from functools import partial
from typing import Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from qsparse_amd import _hip, _mx_common
from qsparse_amd._mx_common import (_OUT_DTYPES, MXActivation, _check_bias, _check_bias_shape, _check_codes_out, _check_dtype,
                                    _check_train_entry, _codes_out_cpu, _MXTrainMixin, _quantize_grad, _save_train_ctx, _split_request)
from qsparse_amd.quantize import (MX_FORMATS, MXQuantizer, _mx_aten, _mx_check_rounding, _mx_format, _mx_sr_words, mx_dequantize,
                                  quantize_with_mx)


# an operand of `mx_matmul`: a is [..., K], b has at least the two dimensions of [N, K]
_check_a = partial(_mx_common._check_operand, what="[..., K]", least=1, most=None, needs="at least one dimension")
_check_b = partial(_mx_common._check_operand, what="[N, K]", least=2, most=None, needs="2 dimensions")


def _check_matmul_operands(fn: str, a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, bias, out_dtype):
    """the operands, the bias and `out_dtype` of `mx_matmul`, and of `mx_glu_matmul` (mx_glu.py), which is `fn` then; returns (K, N)"""
    _check_a("a", a_codes, a_scales, a_fmt)
    _check_b("b", b_codes, b_scales, b_fmt)
    if b_codes.dim() != 2:
        raise ValueError(f"b_codes must be [N, K], got shape {tuple(b_codes.shape)}")
    K, N = a_codes.shape[-1], b_codes.shape[0]
    if b_codes.shape[1] != K:
        raise ValueError(f"a_codes {tuple(a_codes.shape)} and b_codes {tuple(b_codes.shape)} disagree on K (their last dimensions)")
    if K < 1:
        raise ValueError(f"{fn} needs K >= 1")
    if b_codes.device != a_codes.device:
        raise ValueError(f"a_codes is on {a_codes.device} but b_codes on {b_codes.device}")
    _check_dtype("out_dtype", out_dtype)
    _check_bias(bias, N, "a_codes", a_codes.device)
    return K, N


def mx_matmul(a_codes: torch.Tensor, a_scales: torch.Tensor, a_fmt: str, b_codes: torch.Tensor, b_scales: torch.Tensor, b_fmt: str,
              bias: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32, *, split_k=1, out_fmt: Optional[str] = None,
              act: Optional[str] = None):
    """``A . B^T (+ bias)`` on MX codes.  ``a_codes`` ``[..., K]`` and ``b_codes`` ``[N, K]`` (an ``nn.Linear`` weight) are uint8
    codes of the formats ``a_fmt`` / ``b_fmt`` (``MX_FORMATS``; they may differ) with blocks along K, ``a_scales`` ``[..., ceil(K /
    32)]`` and ``b_scales`` ``[N, ceil(K / 32)]`` their E8M0 bytes, ``bias`` float32 ``[N]``.  Returns ``[..., N]`` in ``out_dtype``
    (float32, bfloat16 or float16):

        y[m, n] = round( sum_k val(a[m, k]) 2^(sa[m, k / 32] - 127) val(b[n, k]) 2^(sb[n, k / 32] - 127) + bias[n] )

    with ``val`` the value of a code as ``mx_dequantize`` decodes it.  A scale byte 0xFF (a block that held NaN / Inf) makes every
    output that reads it NaN.  GPU tensors take the HIP kernel (float32 accumulation; there is no fallback: without the library
    the call raises), CPU tensors evaluate the expression above in float64 and round once.

    ``split_k`` (keyword; an int ``>= 1`` or ``"auto"``) cuts the walk along K into that many slices of whole steps of 128 codes
    (``qs_mx_matmul_splitk_v``): the slices run side by side, their float32 partial sums go to a workspace and are added in ascending
    order, then the bias, then the one rounding -- no atomics, so the result is a pure function of the operands and ``split_k``,
    the same on every run.  It is for products with a small output and a long K (a weight gradient), which otherwise occupy a
    fraction of the GPU.  ``1`` (the default) is the unsplit kernel, bit for bit; ``"auto"`` lets the library choose from the shape
    (1 whenever ``ceil(K / 128) < 32`` or the output has 256 tiles of 128 x 128 or more).  A request that leaves one slice is the
    unsplit call.  The CPU path checks the argument and evaluates the float64 definition, which has no order to cut.

    ``out_fmt`` (keyword; a name of ``MX_FORMATS``) makes the product hand out MX codes instead of a float tensor: the return is
    ``(codes uint8 [..., N], scales uint8 [..., ceil(N / 32)])``, bit for bit the codes and scales of
    ``quantize_with_mx(act(y), out_fmt, -1, return_codes=True)`` with ``y`` the float32 result above and blocks along N -- the next
    product's K.  ``act`` (keyword) is ``None`` or ``"relu"`` (NaN stays NaN, everything else that is not positive becomes +0) and
    needs ``out_fmt``.  On the GPU it is one kernel (``qs_mx_matmul_q_v``): the quantizer runs on the accumulators and no float ``y``
    is written or read.  ``out_dtype`` must stay at its default and ``split_k`` at 1 (the split product's reduction does not
    quantize).  CPU tensors round the float64 result once to float32, apply ``act`` and run the CPU quantizer."""
    request = _split_request(split_k)
    _check_codes_out("mx_matmul", out_fmt, act, out_dtype, request)
    K, N = _check_matmul_operands("mx_matmul", a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, bias, out_dtype)
    lead = tuple(a_codes.shape[:-1])
    a2, sa2 = a_codes.reshape(-1, K), a_scales.reshape(-1, a_scales.shape[-1])
    if a_codes.is_cuda and out_fmt is not None:
        codes, scales = _hip.mx_matmul_q(a2.contiguous(), sa2.contiguous(), a_fmt, b_codes.contiguous(), b_scales.contiguous(), b_fmt,
                                         None if bias is None else bias.contiguous(), out_fmt, act)
        return codes.reshape(lead + (N,)), scales.reshape(lead + (scales.shape[-1],))
    if a_codes.is_cuda:
        y = _hip.mx_matmul(a2.contiguous(), sa2.contiguous(), a_fmt, b_codes.contiguous(), b_scales.contiguous(), b_fmt,
                           None if bias is None else bias.contiguous(), out_dtype, request)
    else:
        a = mx_dequantize(a2, sa2, a_fmt, -1, torch.float64)
        b = mx_dequantize(b_codes, b_scales, b_fmt, -1, torch.float64)
        # a 0xFF block is NaN in every product that reads it, also against a zero (NaN * 0 is NaN): matmul's own propagation
        y = a @ b.t()
        if bias is not None:
            y = y + bias.to(torch.float64)
        y = y.to(out_dtype)
        if out_fmt is not None:
            return _codes_out_cpu(y.reshape(lead + (N,)), out_fmt, act)
    return y.reshape(lead + (N,))


class MXLinear(nn.Module):
    """``nn.Linear`` for inference on MX codes: the weight is held as uint8 codes ``weight_codes [N, K]`` and E8M0 scales
    ``weight_scales [N, ceil(K / 32)]`` of the format ``weight_fmt`` (buffers, with the optional float32 ``bias``); ``forward``
    quantizes its input to ``act_fmt`` along the last dimension with the MX quantizer (``quantize_with_mx``) and multiplies the two
    sets of codes with ``mx_matmul``.  The output is float32 (or ``out_dtype``) and never requires grad; an input that requires
    grad while gradients are enabled is refused -- training runs on the simulated layers this one is built from.

    Chaining without a float tensor in between: with ``out_fmt`` (keyword; optionally ``act="relu"``) ``forward`` returns an
    ``MXActivation`` -- the codes and scales of ``quantize_with_mx(act(y), out_fmt, -1)``, written by the product's own epilogue --
    and ``forward`` also TAKES an ``MXActivation`` in place of a float tensor: its codes are multiplied as they are, in their own
    format (``act_fmt`` is not consulted: the product takes any pair).  ``nn.Sequential(MXLinear(..., out_fmt=f, act="relu"),
    MXLinear(...))`` computes bit for bit what the two layers compute with a float ReLU between them when the second one's
    ``act_fmt`` is ``f``."""

    def __init__(self, weight_codes: torch.Tensor, weight_scales: torch.Tensor, weight_fmt: str, bias: Optional[torch.Tensor] = None,
                 act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *, out_fmt: Optional[str] = None,
                 act: Optional[str] = None):
        super().__init__()
        _mx_format(act_fmt)
        _check_codes_out("MXLinear", out_fmt, act, out_dtype)
        self.out_fmt, self.act = out_fmt, act
        _check_b("b", weight_codes, weight_scales, weight_fmt)
        if weight_codes.dim() != 2:
            raise ValueError(f"weight_codes must be [N, K], got shape {tuple(weight_codes.shape)}")
        _check_bias_shape(bias, weight_codes.shape[0])
        self.weight_fmt, self.act_fmt, self.out_dtype = weight_fmt, act_fmt, out_dtype
        self.out_features, self.in_features = weight_codes.shape
        self.register_buffer("weight_codes", weight_codes.detach().clone().contiguous())
        self.register_buffer("weight_scales", weight_scales.detach().clone().contiguous())
        self.register_buffer("bias", None if bias is None else bias.detach().to(torch.float32).clone().contiguous())

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"weight_fmt={self.weight_fmt!r}, act_fmt={self.act_fmt!r}" +
                (f", out_fmt={self.out_fmt!r}" if self.out_fmt is not None else "") + (f", act={self.act!r}" if self.act is not None else ""))

    @classmethod
    def from_exported(cls, qt, bias: Optional[torch.Tensor] = None, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *,
                      out_fmt: Optional[str] = None, act: Optional[str] = None):
        """from the ``QuantizedTensor(kind="mx")`` ``export_integer`` returns for a linear layer's weight"""
        if getattr(qt, "kind", None) != "mx":
            raise ValueError(f"MXLinear needs an MX weight (QuantizedTensor.kind == 'mx'), got kind {getattr(qt, 'kind', None)!r}")
        if qt.codes.dim() != 2:
            raise ValueError(f"MXLinear needs a 2-d weight [N, K], got shape {tuple(qt.codes.shape)}")
        if qt.block_dim % qt.codes.dim() != 1:
            raise ValueError(f"the weight's MX blocks run along dim {qt.block_dim}, not along K (dim 1): blocks along N cannot feed the "
                             "matrix instruction -- quantize the layer with MXQuantizer(fmt, block_dim=1)")
        return cls(qt.codes, qt.block_scale, qt.fmt, bias, act_fmt, out_dtype, out_fmt=out_fmt, act=act)

    @classmethod
    def from_quantized(cls, layer: nn.Module, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *,
                       out_fmt: Optional[str] = None, act: Optional[str] = None):
        """from a ``quantize(nn.Linear(...), bits=w, callback=MXQuantizer(fmt, block_dim=1))`` layer that is past its timeout:
        the weight codes are the export's, the bias what the layer's evaluation-mode forward adds"""
        from qsparse_amd.export import export_integer
        q = layer.__dict__.get("_modules", {}).get("quantize")
        if not isinstance(layer, nn.Linear) or q is None or not isinstance(q.callback, MXQuantizer):
            raise ValueError("MXLinear.from_quantized needs an nn.Linear wrapped by quantize(..., callback=MXQuantizer(...))")
        rec = export_integer(nn.Sequential(layer)).get("0")
        if rec is None or rec.weight is None:
            raise ValueError("the layer has not quantized its weight yet (still inside its timeout): nothing to build an MXLinear from")
        was = layer.training
        layer.eval()
        try:
            with torch.no_grad():
                b = layer.bias
                bias = None if b is None else b.detach().to(torch.float32)
        finally:
            layer.train(was)
        return cls.from_exported(rec.weight, bias, act_fmt, out_dtype, out_fmt=out_fmt, act=act)

    def forward(self, x):
        taken = isinstance(x, MXActivation)
        if not taken and torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("MXLinear is an inference layer: its input requires grad.  Train with the simulated layer "
                               "(quantize(nn.Linear(...), callback=MXQuantizer(...))) or call it under torch.no_grad()")
        with torch.no_grad():
            if taken:
                if x.channels_last:
                    raise ValueError("MXLinear got an MXActivation with channels_last=True: the [B, H, W, C] codes of a convolution, whose "
                                     "float form is [B, C, H, W] -- flatten the float tensor, or pass MXActivation(codes, scales, fmt)")
                codes, scales, fmt = x.codes, x.scales, x.fmt
            else:
                fmt = self.act_fmt
                _, codes, scales = quantize_with_mx(x, fmt, -1, return_codes=True)
            y = mx_matmul(codes, scales, fmt, self.weight_codes, self.weight_scales, self.weight_fmt, self.bias, self.out_dtype,
                          out_fmt=self.out_fmt, act=self.act)
            return y if self.out_fmt is None else MXActivation(*y, self.out_fmt)


def mx_quantize_2way(x: torch.Tensor, row_fmt: Optional[str] = None, col_fmt: Optional[str] = None, rounding: str = "nearest",
                     seed: int = 0, step: Optional[torch.Tensor] = None):
    """MX codes of a 2-d float32 / bfloat16 / float16 tensor ``x [R, C]`` both ways from one read: returns ``(row_codes [R, C],
    row_scales [R, ceil(C / 32)], col_codes [C, R], col_scales [C, ceil(R / 32)])`` -- the row pair is the codes and scales of
    ``quantize_with_mx(x, row_fmt, -1, return_codes=True)``, the col pair those of ``quantize_with_mx(x.t().contiguous(), col_fmt,
    -1, return_codes=True)``, bit for bit.  A pair whose format is ``None`` is not computed and comes back as ``(None, None)``; at
    least one format must be given.  No de-quantized tensor is produced and the outputs are never differentiable.  GPU tensors take
    the HIP kernel (one launch; no fallback), CPU tensors two evaluations of the definition.

    ``rounding="stochastic"`` (``seed``, ``step`` as in ``quantize_with_mx``): the row pair is the stochastic one-way quantizer on
    ``x`` with ``stream=0``, the col pair the one on ``x.t().contiguous()`` with ``stream=1`` -- the two forms of a tensor are
    rounded independently, each indexed in its own output."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a tensor, got {type(x).__name__}")
    if x.dim() != 2:
        raise ValueError(f"mx_quantize_2way needs a 2-d tensor [R, C], got shape {tuple(x.shape)}")
    _check_dtype("x", x.dtype)
    if row_fmt is None and col_fmt is None:
        raise ValueError("mx_quantize_2way needs row_fmt, col_fmt or both")
    for fmt in (row_fmt, col_fmt):
        if fmt is not None:
            _mx_format(fmt)
    _mx_check_rounding(rounding, step, x)
    x = x.detach()
    sr = rounding == "stochastic"
    if x.is_cuda:
        return _hip.mx_quant2(x.contiguous(), row_fmt, col_fmt, rounding, seed, step)
    rc = rs = cc = cs = None
    if row_fmt is not None:
        _, rc, rs = _mx_aten(x, row_fmt, 1, torch.float32, True, _mx_sr_words(x.shape, seed, step, 0) if sr else None)
    if col_fmt is not None:
        xt = x.t()
        _, cc, cs = _mx_aten(xt, col_fmt, 1, torch.float32, True, _mx_sr_words(xt.shape, seed, step, 1) if sr else None)
    return rc, rs, cc, cs


class _MXLinearFunction(torch.autograd.Function):
    """y = Q(x) Q(W)^T + b, dx = Q(dy) Q(W^T)^T, dW = Q(dy^T) Q(x^T)^T on MX codes; every quantizer straight-through"""

    @staticmethod
    def forward(ctx, x, weight, bias, x_fmt, w_fmt, grad_fmt, need_col, grad_rounding="nearest", seed=0, step=None, wgrad_split_k=1):
        # `need_col`: a weight gradient can be asked for -- decided by mx_linear, where the grad mode is still the caller's (it is
        # always off in here, and needs_input_grad is requires_grad whatever the mode)
        N, K = weight.shape
        x2 = x.reshape(-1, K)
        x_row, x_rs, x_col, x_cs = mx_quantize_2way(x2, x_fmt, x_fmt if need_col else None)
        w_row, w_rs, _, _ = mx_quantize_2way(weight, w_fmt, None)
        b32 = None if bias is None else bias.detach().to(torch.float32)
        y = mx_matmul(x_row, x_rs, x_fmt, w_row, w_rs, w_fmt, b32, x.dtype)
        # the weight itself (autograd's version counter guards it), and x as its transposed codes: 1 + 1/32 bytes per element
        ctx.save_for_backward(weight, x_col, x_cs)
        _save_train_ctx(ctx, (x_fmt, w_fmt, grad_fmt), (grad_rounding, seed, step), wgrad_split_k, x, bias)
        ctx.x_shape = x.shape
        return y.reshape(x.shape[:-1] + (N,))

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        weight, x_col, x_cs = ctx.saved_tensors
        x_fmt, w_fmt, grad_fmt = ctx.fmts
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        N = weight.shape[0]
        dy2 = dy.reshape(-1, N).contiguous()
        dx = dw = db = None
        if need_dx or need_dw:
            g_row, g_rs, g_col, g_cs = _quantize_grad(ctx, lambda *sr: mx_quantize_2way(dy2, grad_fmt if need_dx else None,
                                                                                         grad_fmt if need_dw else None, *sr))
        if need_dx:
            _, _, w_col, w_cs = mx_quantize_2way(weight, None, w_fmt)
            dx = mx_matmul(g_row, g_rs, grad_fmt, w_col, w_cs, w_fmt, None, ctx.x_dtype).reshape(ctx.x_shape)
        if need_dw:
            dw = mx_matmul(g_col, g_cs, grad_fmt, x_col, x_cs, x_fmt, None, weight.dtype, split_k=ctx.wgrad_split_k)
        if need_db:
            db = dy2.sum(0, dtype=torch.float32).to(ctx.bias_dtype)
        return dx, dw, db, None, None, None, None, None, None, None, None


def mx_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, x_fmt: str = "mxfp8_e4m3",
              w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest", seed: int = 0,
              step: Optional[torch.Tensor] = None, wgrad_split_k="auto") -> torch.Tensor:
    """``F.linear`` whose three matrix products run on MX codes (``mx_matmul``), differentiable in ``x``, ``weight`` and ``bias``.
    ``x`` is ``[..., K]`` in float32 / bfloat16 / float16, ``weight`` ``[N, K]`` and ``bias`` ``[N]`` in any of the three (float32
    parameters next to a bfloat16 ``x`` are fine); the result is ``[..., N]`` in ``x.dtype``.  With ``Q_f(t)`` the MX quantization of
    ``t`` in format ``f`` with blocks of 32 along its LAST axis, ``M`` the number of rows of ``x`` and ``dy`` the incoming gradient:

        y  = Q_x(x) Q_w(W)^T + bias            blocks along K
        dx = Q_g(dy) Q_w(W^T)^T                blocks along N
        dW = Q_g(dy^T) Q_x(x^T)^T              blocks along M
        db = sum over rows of dy (float32)

    -- the straight-through rule of ``quantize_with_mx`` applied to all six quantizers.  ``mx_quantize_2way`` prepares the operands:
    one call on ``x`` yields ``Q_x(x)`` and ``Q_x(x^T)`` (the latter is what the backward keeps instead of ``x``), one on ``dy``
    both forms of the gradient.  Gradients nobody asks for are not computed, and without grad the transposed codes of ``x`` are
    not either.  GPU tensors run HIP kernels only (no host synchronisation: a step can be graph-captured); CPU tensors evaluate
    the same formulas in float64.

    ``grad_rounding="stochastic"`` rounds the two forms of ``dy`` -- and nothing else: ``x`` and ``W`` stay round-to-nearest-even, ``y``
    is the nearest mode's bit for bit -- stochastically (``mx_quantize_2way(dy, ..., "stochastic", seed, step)``), which makes
    ``Q_g(dy)`` an unbiased estimate of ``dy`` also in the FP6 / FP4 formats, where nearest rounding zeroes every element below half
    its block's smallest step.  ``step`` (a one-element int64 tensor on ``x``'s device, or None) is part of the key and is advanced
    by one in place after each backward that quantizes ``dy``, without a host synchronisation: successive steps, and successive
    replays of a captured step, draw different words.

    ``wgrad_split_k`` (an int ``>= 1`` or ``"auto"``) is ``mx_matmul``'s ``split_k`` for the weight-gradient product alone -- the one
    with a small output ``[N, K]`` and the contraction over the ``M`` rows; ``y`` and ``dx`` are untouched by it.  The default
    ``"auto"`` lets the library split that product when its shape leaves most of the GPU idle: ``dW`` then differs from
    ``wgrad_split_k=1`` in the order of its float32 additions only (deterministically: same bits on every run), and only for shapes
    the rule splits -- none with fewer than 3969 rows ``M``, none whose weight has 256 tiles of 128 x 128 or more."""
    _check_train_entry(x, weight, bias, (x_fmt, w_fmt, grad_fmt), grad_rounding, step, wgrad_split_k)
    if weight.dim() != 2:
        raise ValueError(f"weight must be [N, K], got shape {tuple(weight.shape)}")
    if x.dim() < 1 or x.shape[-1] != weight.shape[1]:
        raise ValueError(f"x {tuple(x.shape)} and weight {tuple(weight.shape)} disagree on K (their last dimensions)")
    if weight.shape[1] < 1:
        raise ValueError("mx_linear needs K >= 1")
    _check_bias_shape(bias, weight.shape[0])
    need_col = torch.is_grad_enabled() and weight.requires_grad
    return _MXLinearFunction.apply(x, weight, bias, x_fmt, w_fmt, grad_fmt, need_col, grad_rounding, seed, step, wgrad_split_k)


class MXTrainLinear(_MXTrainMixin, nn.Linear):
    """Drop-in ``nn.Linear`` that trains through MX matrix products: float ``weight`` / ``bias`` parameters (``nn.Linear``'s own
    ``state_dict``), ``forward`` is ``mx_linear`` in the formats ``x_fmt`` / ``w_fmt`` / ``grad_fmt``.  Under ``torch.autocast``
    the input is cast to the autocast dtype, as ``nn.Linear``'s would be, and the output has that dtype.

    ``grad_rounding="stochastic"`` rounds the gradient operands stochastically (``mx_linear``).  The layer then owns ``sr_seed`` --
    ``seed``, or a draw from torch's default CPU generator when that is None, so ``torch.manual_seed`` makes a model reproducible
    and no two layers share their noise -- and a non-persistent int64 buffer ``sr_step`` that counts its backwards on the device.
    With ``"nearest"`` neither exists and the ``state_dict`` is ``nn.Linear``'s.

    ``wgrad_split_k`` is ``mx_linear``'s: ``"auto"`` (the default) lets the library split the weight-gradient product along the batch
    rows where that fills the GPU, which changes ``weight.grad`` in float32 summation order only (never below 3969 rows)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=None, x_fmt: str = "mxfp8_e4m3",
                 w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest", seed: Optional[int] = None,
                 wgrad_split_k="auto"):
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)
        self._init_mx(dict(x_fmt=x_fmt, w_fmt=w_fmt, grad_fmt=grad_fmt), grad_rounding, seed)
        self._init_split(wgrad_split_k)

    @classmethod
    def from_linear(cls, layer: nn.Linear, x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2",
                    grad_rounding: str = "nearest", seed: Optional[int] = None, wgrad_split_k="auto"):
        """a layer on ``layer``'s own parameters (shared, not copied)"""
        if not isinstance(layer, nn.Linear):
            raise TypeError(f"MXTrainLinear.from_linear needs an nn.Linear, got {type(layer).__name__}")
        return cls(layer.in_features, layer.out_features, bias=layer.bias is not None, device="meta", x_fmt=x_fmt, w_fmt=w_fmt,
                   grad_fmt=grad_fmt, grad_rounding=grad_rounding, seed=seed, wgrad_split_k=wgrad_split_k)._adopt(layer)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x, seed, step = self._mx_input(x)
        return mx_linear(x, self.weight, self.bias, self.x_fmt, self.w_fmt, self.grad_fmt, self.grad_rounding, seed, step,
                         self.wgrad_split_k)

    def to_inference(self, act_fmt: Optional[str] = None, out_dtype: torch.dtype = torch.float32, *, out_fmt: Optional[str] = None,
                     act: Optional[str] = None) -> MXLinear:
        """the ``MXLinear`` on the current weight: its weight bytes are the row pair the training forward multiplies with"""
        codes, scales, _, _ = mx_quantize_2way(self.weight, self.w_fmt, None)
        return MXLinear(codes, scales, self.w_fmt, None if self.bias is None else self.bias.detach(), act_fmt or self.x_fmt, out_dtype,
                        out_fmt=out_fmt, act=act)


__all__ = ["mx_matmul", "MXLinear", "MXActivation", "mx_quantize_2way", "mx_linear", "MXTrainLinear", "MX_FORMATS"]
