"""Training through the gated (SwiGLU / GeGLU) matrix products on MX codes: ``mx_glu_backward_quantize``, ``mx_glu_linear``,
``mx_grouped_glu_linear`` and the layers ``MXTrainGLULinear``, ``MXTrainGroupedGLULinear`` and ``MXTrainGatedMoEFeedForward``.

Notation.  ``W`` is the combined weight ``[2 H, K]`` (``[E, 2 H, K]`` grouped) in the 32-row interleave of
``mx_glu_interleave``, ``v = Q(x) Q(W)^T + bias`` the pre-activations ``[T, 2 H]``, ``g`` and ``u`` their de-interleaved halves and
``h = act(g) * u``.  The forward is the gated product of ``mx_glu.py`` with ``preact_dtype``: one launch hands out ``h`` and keeps
``v``.  The backward needs ``dv [T, 2 H]``, interleaved like ``v``, with ``dg = (dh * u) * act'(g)`` and ``du = dh * act(g)``, as MX
codes both ways; ``mx_glu_backward_quantize`` produces those from one read of ``dh`` and ``v`` without ``dv`` ever being in memory.
From there ``dx`` and ``dW`` are the products of ``mx_linear`` / ``mx_grouped_linear``: the contraction over ``2 H`` does not care about
the interleave, and ``dW`` comes out interleaved like ``W``.  The checks and the autograd scaffold are ``_mx_common.py``'s."""
import math
from typing import Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from qsparse_amd import _hip
from qsparse_amd._mx_common import (_act, _check_bias_shape, _check_dtype, _check_train_entry, _MXTrainMixin, _quantize_grad,
                                    _save_train_ctx)
from qsparse_amd.mx_batched_train import mx_quantize_2way_batched
from qsparse_amd.mx_gemm import mx_matmul, mx_quantize_2way
from qsparse_amd.mx_glu import (GLU_ACTS, MXGatedMoEFeedForward, MXGLULinear, MXGroupedGLULinear, _check_hidden, mx_glu_deinterleave,
                                mx_glu_interleave, mx_glu_matmul, mx_grouped_glu_matmul)
from qsparse_amd.mx_grouped_train import MXTrainGroupedLinear, MXTrainMoEFeedForward, _check_offs, _grouped_backward
from qsparse_amd.quantize import MX_BLOCK, _mx_check_rounding, _mx_format

_GELU_ALPHA = math.sqrt(0.5)
_GELU_BETA = 2.0 / math.sqrt(math.pi) * math.sqrt(0.5) * 0.5


def _glu_dv(dh: torch.Tensor, v: torch.Tensor, act: str) -> torch.Tensor:
    """the definition of dv [T, 2 H] in float32 by elementary torch ops, one rounding each, in the header's order"""
    g, u = mx_glu_deinterleave(v.to(torch.float32), dim=-1)
    d = dh.to(torch.float32)
    if act == "relu":
        a, da = _act(g, "relu"), torch.where(g > 0, torch.ones_like(g), torch.where(g != g, g, torch.zeros_like(g)))
    elif act == "silu":
        s = 1.0 / (1.0 + torch.exp(-g))
        a, da = g / (1.0 + torch.exp(-g)), s * (1.0 + g * (1.0 - s))
    else:
        a = (g * 0.5) * (1.0 + torch.erf(g * _GELU_ALPHA))
        if g.is_cuda:       # ATen's GPU kernel is the header's factor bit for bit (qs_common.h: gelu_grad_factor), its one fma included
            da = torch.ops.aten.gelu_backward(torch.ones_like(g), g)
        else:               # (addcmul is what torch offers for that fma on the CPU, where it may round twice: the CPU path's own)
            da = torch.addcmul(0.5 * (1.0 + torch.erf(g * _GELU_ALPHA)), g, torch.exp(-0.5 * g * g) * _GELU_BETA)
    return mx_glu_interleave((d * u) * da, d * a, dim=-1)


def mx_glu_backward_quantize(dh: torch.Tensor, v: torch.Tensor, *, act: str, row_fmt: Optional[str] = None, col_fmt: Optional[str] = None,
                             rounding: str = "nearest", seed: int = 0, step: Optional[torch.Tensor] = None):
    """The gradient of ``h = act(g) * u`` with respect to the interleaved pre-activations, as MX codes both ways, from one read of
    ``dh [T, H]`` and ``v [T, 2 H]`` (float32 / bfloat16 / float16, independently; ``H % 32 == 0``).  With ``g = v[:, 64 q + t]``, ``u =
    v[:, 64 q + 32 + t]`` and ``d = dh[:, 32 q + t]``, all widened to float32:

        dv[:, 64 q + t]      = (d * u) * act'(g)
        dv[:, 64 q + 32 + t] = d * act(g)

    ``act`` as in ``mx_glu_matmul``; ``act'`` is ``g > 0 ? 1 : (NaN stays NaN, else +0)``, ``s * (1 + g * (1 - s))`` with ``s = 1 / (1 +
    expf(-g))``, or the factor of ATen's GPU ``gelu_backward``.  Returns ``(row_codes [T, 2 H], row_scales [T, 2 H / 32], col_codes
    [2 H, T], col_scales [2 H, ceil(T / 32)])``: bit for bit ``mx_quantize_2way(dv, row_fmt, col_fmt, rounding, seed, step)`` on the
    float32 ``dv``, a skipped pair (format ``None``) as ``(None, None)``.  GPU tensors take the HIP kernel
    (``qs_mx_glu_bwd_quant2_v``): one launch, ``dv`` is never rounded to a narrower type and never in memory; no fallback.  CPU
    tensors evaluate the definition with torch ops and ``mx_quantize_2way``."""
    for name, t in (("dh", dh), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        _check_dtype(name, t.dtype)
    if act not in GLU_ACTS:
        raise ValueError(f"unknown act {act!r}: mx_glu_backward_quantize takes one of {GLU_ACTS}")
    if dh.dim() != 2 or v.dim() != 2 or v.shape[0] != dh.shape[0] or v.shape[1] != 2 * dh.shape[1]:
        raise ValueError(f"dh must be [T, H] and v [T, 2 H], got shapes {tuple(dh.shape)} and {tuple(v.shape)}")
    _check_hidden(dh.shape[1], "mx_glu_backward_quantize")
    if v.device != dh.device:
        raise ValueError(f"dh is on {dh.device} but v on {v.device}")
    if row_fmt is None and col_fmt is None:
        raise ValueError("mx_glu_backward_quantize needs row_fmt, col_fmt or both")
    for fmt in (row_fmt, col_fmt):
        if fmt is not None:
            _mx_format(fmt)
    _mx_check_rounding(rounding, step, dh)
    dh, v = dh.detach(), v.detach()
    if dh.is_cuda:
        return _hip.mx_glu_bwd_quant2(dh.contiguous(), v.contiguous(), act, row_fmt, col_fmt, rounding, seed, step)
    if dh.numel() == 0:
        return mx_quantize_2way(v.new_zeros(v.shape, dtype=torch.float32), row_fmt, col_fmt)
    return mx_quantize_2way(_glu_dv(dh, v, act), row_fmt, col_fmt, rounding, seed, step)


class _MXGLULinearFunction(torch.autograd.Function):
    """the table of `mx_glu_linear` on MX codes; every quantizer straight-through.  `need_dx` / `need_dw`: that gradient can be asked
    for -- decided by mx_glu_linear, where the grad mode is still the caller's"""

    @staticmethod
    def forward(ctx, x, weight, bias, act, x_fmt, w_fmt, grad_fmt, out_dtype, preact_dtype, need_dx, need_dw, grad_rounding, seed, step,
                wgrad_split_k):
        N, K = weight.shape
        x2 = x.reshape(-1, K)
        x_row, x_rs, x_col, x_cs = mx_quantize_2way(x2, x_fmt, x_fmt if need_dw else None)
        w_row, w_rs, w_col, w_cs = mx_quantize_2way(weight, w_fmt, w_fmt if need_dx else None)
        b32 = None if bias is None else bias.detach().to(torch.float32)
        h, v = mx_glu_matmul(x_row, x_rs, x_fmt, w_row, w_rs, w_fmt, b32, out_dtype, act=act, preact_dtype=preact_dtype)
        ctx.save_for_backward(v, x_col, x_cs, w_col, w_cs)
        _save_train_ctx(ctx, (x_fmt, w_fmt, grad_fmt), (grad_rounding, seed, step), wgrad_split_k, x, bias)
        ctx.act, ctx.x_shape, ctx.w_dtype = act, x.shape, weight.dtype
        return h.reshape(x.shape[:-1] + (N // 2,))

    @staticmethod
    @once_differentiable
    def backward(ctx, dh):
        v, x_col, x_cs, w_col, w_cs = ctx.saved_tensors
        x_fmt, w_fmt, grad_fmt = ctx.fmts
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        need_dx, need_dw = need_dx and w_col is not None, need_dw and x_col is not None
        dh2 = dh.reshape(-1, v.shape[1] // 2).contiguous()
        dx = dw = db = None
        if need_dx or need_dw:
            g_row, g_rs, g_col, g_cs = _quantize_grad(ctx, lambda *sr: mx_glu_backward_quantize(
                dh2, v, act=ctx.act, row_fmt=grad_fmt if need_dx else None, col_fmt=grad_fmt if need_dw else None, rounding=sr[0],
                seed=sr[1], step=sr[2]))
        if need_dx:
            dx = mx_matmul(g_row, g_rs, grad_fmt, w_col, w_cs, w_fmt, None, ctx.x_dtype).reshape(ctx.x_shape)
        if need_dw:
            dw = mx_matmul(g_col, g_cs, grad_fmt, x_col, x_cs, x_fmt, None, ctx.w_dtype, split_k=ctx.wgrad_split_k)
        if need_db:         # the float32 row sum of dv by torch ops: a pass of its own
            db = _glu_dv(dh2, v, ctx.act).sum(0, dtype=torch.float32).to(ctx.bias_dtype)
        return (dx, dw, db) + (None,) * 12


def _check_glu_entry(fn: str, act, out_dtype, preact_dtype, x):
    if act not in GLU_ACTS:
        raise ValueError(f"unknown act {act!r}: {fn} takes one of {GLU_ACTS}")
    out_dtype = x.dtype if out_dtype is None else out_dtype
    _check_dtype("out_dtype", out_dtype)
    _check_dtype("preact_dtype", preact_dtype)
    return out_dtype


def _check_interleaved_rows(fn: str, N: int):
    if N % (2 * MX_BLOCK) != 0:
        raise ValueError(f"{fn}: the weight has {N} rows, not 2 H with H a multiple of {MX_BLOCK}: it must be the {MX_BLOCK}-row "
                         "interleave of mx_glu_interleave(w_gate, w_up)")


def mx_glu_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, act: str = "silu",
                  x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2",
                  out_dtype: Optional[torch.dtype] = None, preact_dtype: torch.dtype = torch.float32, grad_rounding: str = "nearest",
                  seed: int = 0, step: Optional[torch.Tensor] = None, wgrad_split_k="auto") -> torch.Tensor:
    """The hidden layer of a gated MLP, ``act(x Wg^T + bg) * (x Wu^T + bu)``, with all three products of a step on MX codes,
    differentiable in ``x``, ``weight`` and ``bias``.  ``x`` is ``[..., K]``; ``weight [2 H, K]`` and ``bias [2 H]`` are INTERLEAVED
    (``mx_glu_interleave(w_gate, w_up)``), so ``dW`` and ``dbias`` come out interleaved and nothing is permuted during a step.  The
    result is ``[..., H]`` in ``out_dtype`` (default ``x.dtype``).  With ``Q`` the MX quantizer along the last axis:

        v  = Q(x) Q(W)^T + bias,  h = act(g) * u          mx_glu_matmul(..., preact_dtype): one launch, v kept in preact_dtype
        dv = interleave((dh * u) * act'(g), dh * act(g))   never in memory: mx_glu_backward_quantize(dh, v) hands out Q(dv), Q(dv^T)
        dx = Q(dv) Q(W^T)^T                                mx_matmul on the col pair of W
        dW = Q(dv^T) Q(x^T)^T                              mx_matmul(..., split_k=wgrad_split_k) on the col pairs
        dbias = sum over rows of dv (float32)              torch ops on the device, only when the bias asks for a gradient

    The forward calls ``mx_quantize_2way`` once on ``x`` and once on ``W`` and saves ``v`` and the col pairs the backward multiplies;
    pairs nobody needs are skipped.  ``grad_rounding="stochastic"`` rounds the two forms of ``dv`` and nothing else stochastically
    (``seed``, ``step`` as in ``mx_linear``; ``step`` is advanced after a backward that quantizes).  The ``dbias`` pass is NOT fused
    into the quantizer: it evaluates ``dv`` again in float32 with torch ops (gated MLPs of current models have no bias).  GPU tensors
    run HIP kernels only and nothing synchronises with the host.  CPU tensors evaluate the same formulas on the CPU paths."""
    _check_train_entry(x, weight, bias, (x_fmt, w_fmt, grad_fmt), grad_rounding, step, wgrad_split_k)
    out_dtype = _check_glu_entry("mx_glu_linear", act, out_dtype, preact_dtype, x)
    if weight.dim() != 2:
        raise ValueError(f"weight must be [2 H, K], got shape {tuple(weight.shape)}")
    if x.dim() < 1 or x.shape[-1] != weight.shape[1]:
        raise ValueError(f"x {tuple(x.shape)} and weight {tuple(weight.shape)} disagree on K (their last dimensions)")
    if weight.shape[1] < 1:
        raise ValueError("mx_glu_linear needs K >= 1")
    _check_interleaved_rows("mx_glu_linear", weight.shape[0])
    _check_bias_shape(bias, weight.shape[0])
    grad = torch.is_grad_enabled()
    return _MXGLULinearFunction.apply(x, weight, bias, act, x_fmt, w_fmt, grad_fmt, out_dtype, preact_dtype, grad and x.requires_grad,
                                      grad and weight.requires_grad, grad_rounding, seed, step, wgrad_split_k)


class _MXGroupedGLULinearFunction(torch.autograd.Function):
    """the table of `mx_grouped_glu_linear` on MX codes; every quantizer straight-through"""

    @staticmethod
    def forward(ctx, x, weight, bias, offs, act, x_fmt, w_fmt, grad_fmt, out_dtype, preact_dtype, need_dx, need_dw, grad_rounding, seed,
                step):
        x_row, x_rs, x_col, x_cs = mx_quantize_2way(x, x_fmt, x_fmt if need_dw else None)
        w_row, w_rs, w_col, w_cs = mx_quantize_2way_batched(weight, w_fmt, w_fmt if need_dx else None)
        b32 = None if bias is None else bias.detach().to(torch.float32)
        h, v = mx_grouped_glu_matmul(x_row, x_rs, x_fmt, w_row, w_rs, w_fmt, offs, b32, out_dtype, act=act, preact_dtype=preact_dtype)
        ctx.save_for_backward(v, x_col, x_cs, w_col, w_cs, offs)
        _save_train_ctx(ctx, (x_fmt, w_fmt, grad_fmt), (grad_rounding, seed, step), None, x, bias)
        ctx.act, ctx.w_dtype = act, weight.dtype
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, dh):
        v, *pairs_offs = ctx.saved_tensors
        dh = dh.contiguous()
        quantize = lambda row_fmt, col_fmt, rounding, seed, step: mx_glu_backward_quantize(
            dh, v, act=ctx.act, row_fmt=row_fmt, col_fmt=col_fmt, rounding=rounding, seed=seed, step=step)
        # mx_grouped_linear's backward on the operands of dv; dbias sums dv, evaluated again in float32 by torch ops
        return _grouped_backward(ctx, dh, *pairs_offs, quantize, lambda: _glu_dv(dh, v, ctx.act)) + (None,) * 12


def mx_grouped_glu_linear(x: torch.Tensor, weight: torch.Tensor, offs: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
                          act: str = "silu", x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2",
                          out_dtype: Optional[torch.dtype] = None, preact_dtype: torch.dtype = torch.float32,
                          grad_rounding: str = "nearest", seed: int = 0, step: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mx_glu_linear`` for ``E`` ragged groups of rows: ``x [T, K]``, ``weight [E, 2 H, K]`` and ``bias [E, 2 H]`` INTERLEAVED per
    group, ``offs`` the cumulative group ends of ``mx_grouped_matmul``; the result is ``[T, H]`` in ``out_dtype``.  The forward is
    ``mx_grouped_glu_matmul(..., preact_dtype)`` on ``mx_quantize_2way(x)`` and ``mx_quantize_2way_batched(weight)``; the backward one
    ``mx_glu_backward_quantize(dh, v)``, then ``dx = mx_grouped_matmul`` on the col pair of ``W`` and ``dW = mx_grouped_weight_grad``
    on the col pairs of ``dv`` and ``x``, exactly as ``mx_grouped_linear`` computes them from the pairs of ``dy``.  The tail rows are
    ``+0`` in ``h`` and ``v`` and reach nothing.  ``dbias[e]`` is the float32 sum of ``dv`` over the rows of group ``e`` -- the
    membership matrix of ``mx_grouped_linear`` times ``dv`` by torch ops, NOT fused, only when the bias asks for a gradient.  Nothing
    reads ``offs`` on the host: a step can be captured in a graph and replayed with other boundaries.  Stochastic rounding as in
    ``mx_glu_linear``."""
    _check_train_entry(x, weight, bias, (x_fmt, w_fmt, grad_fmt), grad_rounding, step, None)
    out_dtype = _check_glu_entry("mx_grouped_glu_linear", act, out_dtype, preact_dtype, x)
    if x.dim() != 2 or weight.dim() != 3:
        raise ValueError(f"x needs [T, K] and weight [E, 2 H, K], got shapes {tuple(x.shape)} and {tuple(weight.shape)}: one weight "
                         "[2 H, K] for every row of x is mx_glu_linear")
    E, N, K = weight.shape
    if x.shape[1] != K:
        raise ValueError(f"x {tuple(x.shape)} and weight {tuple(weight.shape)} disagree on K (their last dimensions)")
    if min(E, N, K) < 1:
        raise ValueError("mx_grouped_glu_linear needs E, H, K >= 1")
    _check_interleaved_rows("mx_grouped_glu_linear", N)
    if bias is not None and tuple(bias.shape) != (E, N):
        raise ValueError(f"bias has shape {tuple(bias.shape)}, expected {(E, N)}")
    _check_offs(offs, E, x.device, "x", f"weight of {tuple(weight.shape)}")
    grad = torch.is_grad_enabled()
    return _MXGroupedGLULinearFunction.apply(x, weight, bias, offs, act, x_fmt, w_fmt, grad_fmt, out_dtype, preact_dtype,
                                             grad and x.requires_grad, grad and weight.requires_grad, grad_rounding, seed, step)


class _TrainGLUMixin(_MXTrainMixin):
    """what ``MXTrainGLULinear`` and ``MXTrainGroupedGLULinear`` add to the scaffold: ONE interleaved parameter per kind, ``act``,
    ``preact_dtype``, ``repr``"""

    def _init_glu(self, weight, bias, act, x_fmt, w_fmt, grad_fmt, out_dtype, preact_dtype, grad_rounding, seed):
        if act not in GLU_ACTS:
            raise ValueError(f"unknown act {act!r}: {type(self).__name__} takes one of {GLU_ACTS}")
        fmts, dtypes = dict(x_fmt=x_fmt, w_fmt=w_fmt, grad_fmt=grad_fmt), dict(out_dtype=out_dtype, preact_dtype=preact_dtype)
        self._check_mx(fmts, dtypes)        # (before the weight is looked at, as ever; `_init_mx` makes them again)
        _check_interleaved_rows(type(self).__name__, weight.shape[-2])
        as_param = lambda t: t if isinstance(t, nn.Parameter) else nn.Parameter(t.detach())
        self.weight = as_param(weight)
        self.bias = None if bias is None else as_param(bias)
        self._init_mx(fmts, grad_rounding, seed, **dtypes)
        self.act = act
        self.out_features, self.in_features = weight.shape[-2] // 2, weight.shape[-1]

    @classmethod
    def from_float(cls, w_gate: torch.Tensor, w_up: torch.Tensor, b_gate: Optional[torch.Tensor] = None,
                   b_up: Optional[torch.Tensor] = None, **options):
        """from the float halves ``w_gate``, ``w_up`` (``[H, K]``, or ``[E, H, K]`` for the grouped layer) and their biases (``[H]`` /
        ``[E, H]``): interleaved ONCE into one parameter ``weight`` (and one ``bias``); ``options`` are the constructor's"""
        if (b_gate is None) != (b_up is None):
            raise ValueError("b_gate and b_up must both be given or both be None")
        with torch.no_grad():
            weight = mx_glu_interleave(w_gate.detach(), w_up.detach())
            bias = None if b_gate is None else mx_glu_interleave(b_gate.detach(), b_up.detach(), dim=-1)
        return cls(weight, bias, **options)

    def gate_up(self):
        """the de-interleaved halves of the current parameters: ``(w_gate, w_up, b_gate, b_up)``, views of them; biases ``None``
        without a bias"""
        b = (None, None) if self.bias is None else mx_glu_deinterleave(self.bias, dim=-1)
        return mx_glu_deinterleave(self.weight) + b

    def extra_repr(self) -> str:
        groups = f"num_groups={self.num_groups}, " if hasattr(self, "num_groups") else ""
        sr = f", grad_rounding={self.grad_rounding!r}" if self.grad_rounding != "nearest" else ""
        return (f"{groups}in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"act={self.act!r}, x_fmt={self.x_fmt!r}, w_fmt={self.w_fmt!r}, grad_fmt={self.grad_fmt!r}{sr}")

    def _mx_glu_input(self, x: torch.Tensor):
        """(x in the autocast dtype, the keywords of the functional form)"""
        x, seed, step = self._mx_input(x)
        return x, dict(act=self.act, x_fmt=self.x_fmt, w_fmt=self.w_fmt, grad_fmt=self.grad_fmt, out_dtype=self.out_dtype,
                       preact_dtype=self.preact_dtype, grad_rounding=self.grad_rounding, seed=seed, step=step)


class MXTrainGLULinear(_TrainGLUMixin, nn.Module):
    """The hidden layer of a gated MLP that trains through MX matrix products: ONE float parameter ``weight [2 H, K]`` (and ``bias
    [2 H]``) in the 32-row interleave of ``mx_glu_interleave``; ``forward`` is ``mx_glu_linear``.  ``from_float(w_gate, w_up, b_gate,
    b_up, ...)`` interleaves once, ``gate_up()`` returns the halves, ``to_inference()`` an ``MXGLULinear`` on the same bytes.
    ``state_dict`` keys: ``weight`` and, with a bias, ``bias`` (interleaved).  ``grad_rounding="stochastic"`` as ``MXTrainLinear``."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, act: str = "silu", x_fmt: str = "mxfp8_e4m3",
                 w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", out_dtype: Optional[torch.dtype] = None,
                 preact_dtype: torch.dtype = torch.float32, grad_rounding: str = "nearest", seed: Optional[int] = None,
                 wgrad_split_k="auto"):
        super().__init__()
        if not isinstance(weight, torch.Tensor) or weight.dim() != 2:
            raise ValueError("MXTrainGLULinear needs an interleaved weight tensor [2 H, K]")
        _check_interleaved_rows("MXTrainGLULinear", weight.shape[0])
        _check_bias_shape(bias, weight.shape[0])
        self._init_split(wgrad_split_k)
        self._init_glu(weight, bias, act, x_fmt, w_fmt, grad_fmt, out_dtype, preact_dtype, grad_rounding, seed)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x, opts = self._mx_glu_input(x)
        return mx_glu_linear(x, self.weight, self.bias, wgrad_split_k=self.wgrad_split_k, **opts)

    def to_inference(self, act_fmt: Optional[str] = None, out_dtype: torch.dtype = torch.float32, *,
                     out_fmt: Optional[str] = None) -> MXGLULinear:
        """the ``MXGLULinear`` on the current weight: its weight bytes are the row pair the training forward multiplies with"""
        codes, scales, _, _ = mx_quantize_2way(self.weight, self.w_fmt, None)
        return MXGLULinear(codes, scales, self.w_fmt, None if self.bias is None else self.bias.detach(), act_fmt or self.x_fmt,
                           out_dtype, act=self.act, out_fmt=out_fmt)


class MXTrainGroupedGLULinear(_TrainGLUMixin, nn.Module):
    """``E`` gated hidden layers on ragged groups of rows that train through MX products: ONE float parameter ``weight [E, 2 H, K]``
    (and ``bias [E, 2 H]``), interleaved per group; ``forward(x, offs)`` is ``mx_grouped_glu_linear``.  ``from_float``, ``gate_up()``
    and ``to_inference()`` (an ``MXGroupedGLULinear``) as ``MXTrainGLULinear``.  ``num_groups`` is ``E``."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, act: str = "silu", x_fmt: str = "mxfp8_e4m3",
                 w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", out_dtype: Optional[torch.dtype] = None,
                 preact_dtype: torch.dtype = torch.float32, grad_rounding: str = "nearest", seed: Optional[int] = None):
        super().__init__()
        if not isinstance(weight, torch.Tensor) or weight.dim() != 3:
            raise ValueError("MXTrainGroupedGLULinear needs an interleaved weight tensor [E, 2 H, K]")
        if bias is not None and tuple(bias.shape) != tuple(weight.shape[:2]):
            raise ValueError(f"bias has shape {tuple(bias.shape)}, expected {tuple(weight.shape[:2])}")
        self.num_groups = weight.shape[0]
        self._init_glu(weight, bias, act, x_fmt, w_fmt, grad_fmt, out_dtype, preact_dtype, grad_rounding, seed)

    def forward(self, x: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
        x, opts = self._mx_glu_input(x)
        return mx_grouped_glu_linear(x, self.weight, offs, self.bias, **opts)

    def to_inference(self, act_fmt: Optional[str] = None, out_dtype: torch.dtype = torch.float32, *,
                     out_fmt: Optional[str] = None) -> MXGroupedGLULinear:
        """the ``MXGroupedGLULinear`` on the current weights: its weight bytes are the row pair the training forward multiplies with"""
        codes, scales, _, _ = mx_quantize_2way_batched(self.weight, self.w_fmt, None)
        return MXGroupedGLULinear(codes, scales, self.w_fmt, None if self.bias is None else self.bias.detach(), act_fmt or self.x_fmt,
                                  out_dtype, act=self.act, out_fmt=out_fmt)


class MXTrainGatedMoEFeedForward(MXTrainMoEFeedForward):
    """``MXTrainMoEFeedForward`` with a gated hidden layer -- the feed-forward block of current mixture-of-experts models, trained: ``up``
    is an ``MXTrainGroupedGLULinear`` ``[E, 2 H, D]`` that returns ``act(x Wg^T) * (x Wu^T)`` in float32, ``down`` an
    ``MXTrainGroupedLinear`` ``[E, D, H]`` that quantizes it to the hidden format.  There is no float ReLU.  Routing, permutation and
    combination are ``MXTrainMoEFeedForward.forward``'s, the same code.  The forward value is bit for bit ``MXGatedMoEFeedForward``'s
    on the same weights (``to_inference()``).  ``state_dict`` keys: ``router``, ``up.weight`` / ``up.bias`` (INTERLEAVED),
    ``down.weight`` / ``down.bias``."""

    _up_type = MXTrainGroupedGLULinear
    _hidden_act = None

    @classmethod
    def from_float(cls, router: torch.Tensor, w_gate: torch.Tensor, b_gate: Optional[torch.Tensor], w_up: torch.Tensor,
                   b_up: Optional[torch.Tensor], w_down: torch.Tensor, b_down: Optional[torch.Tensor], top_k: int,
                   w_fmt: str = "mxfp8_e4m3", act_fmt: str = "mxfp8_e4m3", hidden_fmt: str = "mxfp8_e4m3", *, act: str = "silu",
                   grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest", seed: Optional[int] = None):
        """from float tensors, the arguments of ``MXGatedMoEFeedForward.from_float``; ``w_gate`` / ``w_up`` (and their biases) are
        interleaved once into ``up.weight`` (``up.bias``), ``w_down`` / ``b_down`` are shared with the layer"""
        opts = dict(w_fmt=w_fmt, grad_fmt=grad_fmt, out_dtype=torch.float32, grad_rounding=grad_rounding)
        up = MXTrainGroupedGLULinear.from_float(w_gate, w_up, b_gate, b_up, act=act, x_fmt=act_fmt, seed=seed, **opts)
        down = MXTrainGroupedLinear.from_float(w_down, b_down, x_fmt=hidden_fmt, seed=None if seed is None else seed + 1, **opts)
        return cls(router, up, down, top_k)

    def to_inference(self) -> MXGatedMoEFeedForward:
        """the ``MXGatedMoEFeedForward`` on the current weights, in this block's formats"""
        up = self.up.to_inference(out_fmt=self.down.x_fmt)
        return MXGatedMoEFeedForward(self.router.detach(), up, self.down.to_inference(), self.top_k)


__all__ = ["mx_glu_backward_quantize", "mx_glu_linear", "mx_grouped_glu_linear", "MXTrainGLULinear", "MXTrainGroupedGLULinear",
           "MXTrainGatedMoEFeedForward"]
