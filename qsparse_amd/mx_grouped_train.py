"""Training through grouped (ragged) matrix products on MX codes: ``mx_grouped_weight_grad``, ``mx_grouped_linear`` and the layers
``MXTrainGroupedLinear`` and ``MXTrainMoEFeedForward``.

Two of the three products of a grouped linear layer's step are ``mx_grouped_matmul``: the forward ``Q(x_e) Q(W_e)^T`` and the input
gradient ``Q(dy_e) Q(W_e^T)^T``, the latter on the col pair of ``mx_quantize_2way_batched(W)``.  The third, ``dW[e] = dy_e^T x_e``,
contracts over the ragged axis -- expert ``e`` sums over its own ``n_e`` tokens, between boundaries that live on the device and are
multiples of neither the MX block nor the MFMA's step.  ``mx_grouped_weight_grad`` is that product in one launch
(``qs_mx_grouped_wgrad_v``), without reading the boundaries on the host.  The checks and the autograd scaffold are ``_mx_common.py``'s,
shared with ``mx_linear``, ``mx_conv2d_train`` and ``mx_bmm_train``."""
import math
from functools import partial
from typing import Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from qsparse_amd import _hip, _mx_common
from qsparse_amd._mx_common import _act, _check_dtype, _check_train_entry, _MXTrainMixin, _quantize_grad, _save_train_ctx
from qsparse_amd.mx_batched_train import mx_quantize_2way_batched
from qsparse_amd.mx_gemm import mx_quantize_2way
from qsparse_amd.mx_grouped import MXGroupedLinear, MXMoEFeedForward, _offs_int32, mx_grouped_matmul
from qsparse_amd.quantize import MX_BLOCK, mx_dequantize

_STEP = 128        # tokens per step of the kernel's walk: the alignment of a group's slice in the definition

_check_gt = partial(_mx_common._check_operand, what="[N, T]", least=2, most=2, needs="2 dimensions",
                    source="mx_quantize_2way(dy)'s col pair", axis=" (the tokens)")
_check_xt = partial(_mx_common._check_operand, what="[K, T]", least=2, most=2, needs="2 dimensions",
                    source="mx_quantize_2way(x)'s col pair", axis=" (the tokens)")


def _check_offs(offs, E: Optional[int], device, first: str, per: str):
    """the cumulative group ends: an int32 / int64 tensor ``[E]`` on `device`, the device of the operand called `first`"""
    if not isinstance(offs, torch.Tensor):
        raise TypeError(f"offs must be a tensor, got {type(offs).__name__}")
    if offs.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"offs must be an int32 or int64 tensor (the cumulative end row of every group), got {offs.dtype}")
    if offs.dim() != 1 or E is not None and offs.shape[0] != E:
        raise ValueError(f"offs has shape {tuple(offs.shape)}, expected ({'E' if E is None else E},): one cumulative end row per {per}")
    if offs.device != device:
        raise ValueError(f"{first} is on {device} but offs on {offs.device}")


def _ends_cpu(offs: torch.Tensor, T: int):
    """the group ends of a CPU `offs` as Python integers; refuses what the kernel would clamp"""
    ends = [int(v) for v in offs.tolist()]
    if any(hi < lo for lo, hi in zip([0] + ends, ends + [T])):
        raise ValueError(f"offs must be nondecreasing within [0, {T}] (cumulative group ends over the {T} tokens), got {ends}")
    return ends


def _masked_slice(codes: torch.Tensor, scales: torch.Tensor, lo: int, hi: int):
    """the operand of the definition for the tokens [lo, hi), lo < hi, of `codes` [rows, T]: the columns [s0, s1) with the codes outside
    the group set to 0 and the scale bytes of blocks that do not intersect it to 127"""
    T = codes.shape[1]
    s0, s1 = lo // _STEP * _STEP, min(T, -(-hi // _STEP) * _STEP)
    c = codes[:, s0:s1].clone()
    c[:, :lo - s0] = 0
    c[:, hi - s0:] = 0
    b0 = s0 // MX_BLOCK
    s = scales[:, b0:-(-s1 // MX_BLOCK)].clone()
    s[:, :lo // MX_BLOCK - b0] = 127
    s[:, -(-hi // MX_BLOCK) - b0:] = 127
    return c, s


def mx_grouped_weight_grad(gt_codes: torch.Tensor, gt_scales: torch.Tensor, g_fmt: str, xt_codes: torch.Tensor, xt_scales: torch.Tensor,
                           x_fmt: str, offs: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``dW[e] = dy_e^T x_e`` on MX codes for ``E`` groups of tokens of different sizes: the weight gradient of ``mx_grouped_matmul``.
    Both operands carry their blocks of 32 along the TOKEN axis: ``gt_codes`` ``[N, T]`` / ``gt_scales`` ``[N, ceil(T / 32)]`` and
    ``xt_codes`` ``[K, T]`` / ``xt_scales`` ``[K, ceil(T / 32)]`` are the col pairs of ``mx_quantize_2way(dy)`` and
    ``mx_quantize_2way(x)`` (uint8, formats ``g_fmt`` / ``x_fmt`` of ``MX_FORMATS``, which may differ).  ``offs`` is
    ``mx_grouped_matmul``'s: an int32 or int64 tensor ``[E]`` on the operands' device, the cumulative END token of every group.  Returns
    ``[E, N, K]`` in ``out_dtype`` (float32, bfloat16 or float16).

    Definition.  With ``c_-1 = 0`` and ``c_e = min(max(offs[e], c_{e-1}), T)`` group ``e`` owns the tokens ``[lo, hi) = [c_{e-1}, c_e)``.
    If ``hi == lo``, ``dW[e]`` is ``+0``.  Otherwise let ``s0 = 128 floor(lo / 128)`` and ``s1 = min(T, 128 ceil(hi / 128))``; ``G_e`` is
    ``gt_codes[:, s0:s1]`` with every column outside ``[lo, hi)`` set to byte 0, ``GS_e`` is ``gt_scales[:, s0 / 32 : ceil(s1 / 32)]``
    with every block that does not intersect ``[lo, hi)`` set to 127, ``X_e`` / ``XS_e`` likewise, and ``dW[e]`` is bit for bit
    ``mx_matmul(G_e, GS_e, g_fmt, X_e, XS_e, x_fmt, None, out_dtype)``.  A block that straddles a boundary keeps its shared scale byte
    for both groups (a 0xFF there is NaN in both); a block wholly outside a group contributes nothing to it, whatever its bytes are.
    Tokens from ``c_{E-1}`` on reach nothing.

    GPU tensors take the HIP kernel (``qs_mx_grouped_wgrad_v``): one launch for all groups, no split-K, no atomics, no
    synchronisation, and ``offs`` is neither read on the host nor validated (an int64 one is clamped and then narrowed on the device,
    as in ``mx_grouped_matmul``), so the call can be captured in a graph and replayed with other boundaries written into the same
    tensor.  A non-monotone or out-of-range ``offs`` gives the result of the clamped boundaries, never a fault.  There is no fallback:
    without the library the call raises.  CPU tensors refuse an ``offs`` that is not nondecreasing within ``[0, T]`` with a
    ``ValueError``, then evaluate the definition in float64 and round once."""
    _check_gt("gt", gt_codes, gt_scales, g_fmt)
    _check_xt("xt", xt_codes, xt_scales, x_fmt)
    (N, T), K = gt_codes.shape, xt_codes.shape[0]
    if xt_codes.shape[1] != T:
        raise ValueError(f"gt_codes {tuple(gt_codes.shape)} and xt_codes {tuple(xt_codes.shape)} disagree on T (their last dimensions)")
    if xt_codes.device != gt_codes.device:
        raise ValueError(f"gt_codes is on {gt_codes.device} but xt_codes on {xt_codes.device}")
    _check_offs(offs, None, gt_codes.device, "gt_codes", "group")
    _check_dtype("out_dtype", out_dtype)
    if gt_codes.is_cuda:
        return _hip.mx_grouped_wgrad(gt_codes.contiguous(), gt_scales.contiguous(), g_fmt, xt_codes.contiguous(), xt_scales.contiguous(),
                                     x_fmt, _offs_int32(offs, T), out_dtype)
    ends = _ends_cpu(offs, T)
    dw = torch.zeros((len(ends), N, K), dtype=out_dtype)        # (an empty group: +0)
    for e, (lo, hi) in enumerate(zip([0] + ends, ends)):           # group by group, the expression of mx_matmul's CPU path: the same bits
        if hi > lo:
            g = mx_dequantize(*_masked_slice(gt_codes, gt_scales, lo, hi), g_fmt, -1, torch.float64)
            x = mx_dequantize(*_masked_slice(xt_codes, xt_scales, lo, hi), x_fmt, -1, torch.float64)
            dw[e] = (g @ x.t()).to(out_dtype)
    return dw


def _group_membership(offs: torch.Tensor, T: int) -> torch.Tensor:
    """the 0/1 matrix ``[E, T]`` in float32 of the clamped boundaries, computed where `offs` lives: row e is 1 on the tokens of group e"""
    c = torch.cummax(offs.to(torch.int64).clamp(0, T), 0)[0]
    lo = torch.cat([c.new_zeros(1), c[:-1]])
    t = torch.arange(T, device=offs.device)
    return ((t >= lo.unsqueeze(1)) & (t < c.unsqueeze(1))).to(torch.float32)


def _grouped_backward(ctx, dy: torch.Tensor, x_col, x_cs, w_col, w_cs, offs, quantize, bias_rows):
    """(dx, dw, dbias) of a grouped table from the contiguous incoming gradient `dy` [T, *] and the pairs its forward saved.
    `quantize(row_fmt, col_fmt, rounding, seed, step)`: the four gradient operands [T, N] / [N, T] (a format None: that pair is not
    asked for); `bias_rows()`: the float32 [T, N] whose sum over the rows of a group is its dbias"""
    x_fmt, w_fmt, grad_fmt = ctx.fmts
    need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
    need_dx, need_dw = need_dx and w_col is not None, need_dw and x_col is not None
    dx = dw = db = None
    if need_dx or need_dw:
        g_row, g_rs, g_col, g_cs = _quantize_grad(ctx, lambda *sr: quantize(grad_fmt if need_dx else None,
                                                                             grad_fmt if need_dw else None, *sr))
    if need_dx:         # (the tail rows reach nothing: +0)
        dx = mx_grouped_matmul(g_row, g_rs, grad_fmt, w_col, w_cs, w_fmt, offs, None, ctx.x_dtype)
    if need_dw:
        dw = mx_grouped_weight_grad(g_col, g_cs, grad_fmt, x_col, x_cs, x_fmt, offs, ctx.w_dtype)
    if need_db:         # a 0/1 matrix times the rows in float32: no atomics, no host read of offs
        db = (_group_membership(offs, dy.shape[0]) @ bias_rows()).to(ctx.bias_dtype)
    return dx, dw, db


class _MXGroupedLinearFunction(torch.autograd.Function):
    """the table of `mx_grouped_linear` on MX codes; every quantizer straight-through.  `need_dx` / `need_dw`: that gradient can be
    asked for -- decided by mx_grouped_linear, where the grad mode is still the caller's (as mx_linear's `need_col`)"""

    @staticmethod
    def forward(ctx, x, weight, bias, offs, x_fmt, w_fmt, grad_fmt, out_dtype, need_dx, need_dw, grad_rounding, seed, step):
        x_row, x_rs, x_col, x_cs = mx_quantize_2way(x, x_fmt, x_fmt if need_dw else None)
        # the weights with blocks along K for the forward and, transposed to [E, K, N], with blocks along N for dx
        w_row, w_rs, w_col, w_cs = mx_quantize_2way_batched(weight, w_fmt, w_fmt if need_dx else None)
        b32 = None if bias is None else bias.detach().to(torch.float32)
        y = mx_grouped_matmul(x_row, x_rs, x_fmt, w_row, w_rs, w_fmt, offs, b32, out_dtype)
        # what the backward multiplies, as codes: 1 + 1/32 bytes per element (None where nobody asks)
        ctx.save_for_backward(x_col, x_cs, w_col, w_cs, offs)
        _save_train_ctx(ctx, (x_fmt, w_fmt, grad_fmt), (grad_rounding, seed, step), None, x, bias)
        ctx.w_dtype = weight.dtype
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = dy.contiguous()
        return _grouped_backward(ctx, dy, *ctx.saved_tensors, lambda *fmts_sr: mx_quantize_2way(dy, *fmts_sr),
                                 lambda: dy.to(torch.float32)) + (None,) * 10


def mx_grouped_linear(x: torch.Tensor, weight: torch.Tensor, offs: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
                      x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2",
                      out_dtype: Optional[torch.dtype] = None, grad_rounding: str = "nearest", seed: int = 0,
                      step: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``E`` linear layers applied to ragged groups of rows, all three products of a step on MX codes, differentiable in ``x``,
    ``weight`` and ``bias``.  ``x`` is ``[T, K]`` in float32 / bfloat16 / float16, ``weight`` ``[E, N, K]`` and ``bias`` ``[E, N]`` in
    any of the three, ``offs`` the int32 or int64 cumulative group ends ``[E]`` of ``mx_grouped_matmul`` on ``x``'s device; the result
    is ``[T, N]`` in ``out_dtype``, by default ``x.dtype``.  With ``Q(t)`` the MX codes of ``t`` with blocks of 32 along its LAST axis
    -- in ``x_fmt``, ``w_fmt`` and, for the incoming gradient ``dy``, ``grad_fmt`` -- and ``r_e`` the rows of group ``e``:

        y[r_e]   = Q(x)[r_e] Q(W[e])^T + bias[e]          mx_grouped_matmul, row pairs; the tail rows are +0
        dx[r_e]  = Q(dy)[r_e] Q(W[e]^T)^T                 mx_grouped_matmul on the col pair of W; the tail rows are +0
        dW[e]    = Q(dy^T)[:, r_e] Q(x^T)[:, r_e]^T       mx_grouped_weight_grad on the col pairs of dy and x
        dbias[e] = sum of dy over r_e in float32          a 0/1 membership matrix [E, T] times dy

    -- the straight-through rule of ``quantize_with_mx`` at every quantizer, as ``mx_linear``.  The forward calls
    ``mx_quantize_2way(x)`` and ``mx_quantize_2way_batched(weight)`` once each and keeps, as codes, the pairs the backward multiplies;
    the backward calls ``mx_quantize_2way(dy)`` once.  A pair nobody needs is not computed (nothing is kept under ``torch.no_grad()``),
    a gradient nobody asks for is ``None``.  The tail rows of ``dy`` reach nothing.  GPU tensors run HIP kernels only, and nothing
    synchronises with the host or reads ``offs`` there: a step can be captured in a graph and replayed with other boundaries written
    into the same ``offs`` tensor.  CPU tensors evaluate the same formulas on the CPU paths of the three products.

    ``grad_rounding="stochastic"`` rounds the two forms of ``dy`` and nothing else stochastically (``seed``, ``step`` as in
    ``mx_linear``); ``step`` is advanced by one in place after a backward that quantizes ``dy``."""
    _check_train_entry(x, weight, bias, (x_fmt, w_fmt, grad_fmt), grad_rounding, step, None)
    out_dtype = x.dtype if out_dtype is None else out_dtype
    _check_dtype("out_dtype", out_dtype)
    if x.dim() != 2 or weight.dim() != 3:
        raise ValueError(f"x needs [T, K] and weight [E, N, K], got shapes {tuple(x.shape)} and {tuple(weight.shape)}: one weight [N, K] "
                         "for every row of x is mx_linear")
    E, N, K = weight.shape
    if x.shape[1] != K:
        raise ValueError(f"x {tuple(x.shape)} and weight {tuple(weight.shape)} disagree on K (their last dimensions)")
    if min(E, N, K) < 1:
        raise ValueError("mx_grouped_linear needs E, N, K >= 1")
    if bias is not None and tuple(bias.shape) != (E, N):
        raise ValueError(f"bias has shape {tuple(bias.shape)}, expected {(E, N)}")
    _check_offs(offs, E, x.device, "x", f"weight of {tuple(weight.shape)}")
    grad = torch.is_grad_enabled()
    return _MXGroupedLinearFunction.apply(x, weight, bias, offs, x_fmt, w_fmt, grad_fmt, out_dtype, grad and x.requires_grad,
                                          grad and weight.requires_grad, grad_rounding, seed, step)


class MXTrainGroupedLinear(_MXTrainMixin, nn.Module):
    """``E`` linear layers that train through grouped MX matrix products: float parameters ``weight [E, N, K]`` and ``bias [E, N]``,
    ``forward(x, offs)`` is ``mx_grouped_linear`` in the formats ``x_fmt`` / ``w_fmt`` / ``grad_fmt``; the output is ``out_dtype``, by
    default the input's.  Under ``torch.autocast`` the input is cast to the autocast dtype, as ``MXTrainLinear``'s.

    ``grad_rounding="stochastic"`` rounds the gradient operands stochastically.  The layer then owns ``sr_seed`` -- ``seed``, or a draw
    from torch's default CPU generator when that is None -- and a non-persistent int64 buffer ``sr_step`` that counts its backwards on
    the device, as ``MXTrainLinear`` does.  ``state_dict`` keys: ``weight`` and, with a bias, ``bias``."""

    def __init__(self, num_groups: int, in_features: int, out_features: int, bias: bool = True, device=None, dtype=None,
                 x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2",
                 out_dtype: Optional[torch.dtype] = None, grad_rounding: str = "nearest", seed: Optional[int] = None):
        super().__init__()
        if min(num_groups, in_features, out_features) < 1:
            raise ValueError("MXTrainGroupedLinear needs num_groups, in_features, out_features >= 1")
        self.num_groups, self.in_features, self.out_features = num_groups, in_features, out_features
        self.weight = nn.Parameter(torch.empty((num_groups, out_features, in_features), device=device, dtype=dtype))
        self.bias = nn.Parameter(torch.empty((num_groups, out_features), device=device, dtype=dtype)) if bias else None
        if self.weight.device.type != "meta":       # nn.Linear's initialisation, expert by expert
            bound = 1 / math.sqrt(in_features)
            with torch.no_grad():
                self.weight.uniform_(-bound, bound)
                if bias:
                    self.bias.uniform_(-bound, bound)
        self._init_mx(dict(x_fmt=x_fmt, w_fmt=w_fmt, grad_fmt=grad_fmt), grad_rounding, seed, out_dtype=out_dtype)

    def extra_repr(self) -> str:
        sr = f", grad_rounding={self.grad_rounding!r}" if self.grad_rounding != "nearest" else ""
        return (f"num_groups={self.num_groups}, in_features={self.in_features}, out_features={self.out_features}, "
                f"bias={self.bias is not None}, x_fmt={self.x_fmt!r}, w_fmt={self.w_fmt!r}, grad_fmt={self.grad_fmt!r}{sr}")

    @classmethod
    def from_float(cls, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3",
                   grad_fmt: str = "mxfp8_e5m2", out_dtype: Optional[torch.dtype] = None, grad_rounding: str = "nearest",
                   seed: Optional[int] = None):
        """a layer on the float tensors ``weight [E, N, K]`` and ``bias [E, N]`` themselves (shared, not copied): a ``Parameter`` is
        adopted as it is, a plain tensor becomes one on the same storage"""
        if not isinstance(weight, torch.Tensor) or weight.dim() != 3:
            raise ValueError("MXTrainGroupedLinear.from_float needs a weight tensor [E, N, K], got " +
                             (f"shape {tuple(weight.shape)}" if isinstance(weight, torch.Tensor) else type(weight).__name__))
        E, N, K = weight.shape
        if bias is not None and (not isinstance(bias, torch.Tensor) or tuple(bias.shape) != (E, N)):
            raise ValueError(f"bias has shape {tuple(bias.shape) if isinstance(bias, torch.Tensor) else type(bias).__name__}, "
                             f"expected {(E, N)}")
        layer = cls(E, K, N, bias=bias is not None, device="meta", x_fmt=x_fmt, w_fmt=w_fmt, grad_fmt=grad_fmt, out_dtype=out_dtype,
                    grad_rounding=grad_rounding, seed=seed)
        as_param = lambda t: t if isinstance(t, nn.Parameter) else nn.Parameter(t.detach())
        layer.weight = as_param(weight)
        layer.bias = None if bias is None else as_param(bias)
        if grad_rounding == "stochastic":
            layer.sr_step = torch.zeros(1, dtype=torch.int64, device=weight.device)
        return layer

    def forward(self, x: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
        x, seed, step = self._mx_input(x)
        return mx_grouped_linear(x, self.weight, offs, self.bias, x_fmt=self.x_fmt, w_fmt=self.w_fmt, grad_fmt=self.grad_fmt,
                                 out_dtype=self.out_dtype, grad_rounding=self.grad_rounding, seed=seed, step=step)

    def to_inference(self, act_fmt: Optional[str] = None, out_dtype: torch.dtype = torch.float32, *, out_fmt: Optional[str] = None,
                     act: Optional[str] = None) -> MXGroupedLinear:
        """the ``MXGroupedLinear`` on the current weights: its weight bytes are the row pair the training forward multiplies with"""
        codes, scales, _, _ = mx_quantize_2way_batched(self.weight, self.w_fmt, None)
        return MXGroupedLinear(codes, scales, self.w_fmt, None if self.bias is None else self.bias.detach(), act_fmt or self.x_fmt,
                               out_dtype, out_fmt=out_fmt, act=act)


class MXTrainMoEFeedForward(nn.Module):
    """``MXMoEFeedForward`` that trains: a float32 ``router [E, D]`` (a ``Parameter``), an ``MXTrainGroupedLinear`` ``up`` ``[E, H, D]``
    and an ``MXTrainGroupedLinear`` ``down`` ``[E, D, H]`` whose ``x_fmt`` is the hidden format.  ``forward(x)`` takes a float ``x
    [T, D]`` and returns float32 ``[T, D]``.  It is the composition of ``MXMoEFeedForward`` with differentiable pieces:

        1. ``logits = x32 @ router.t()`` in float32; ``topk(logits, k)``, the softmax over the ``k`` kept logits: the gates
        2. a stable argsort of the ``T k`` expert ids; the counts per expert and their cumulative sum ``offs`` on the device
        3. the rows in that order; ``up`` in float32, the ReLU of the codes-out products (NaN stays NaN, everything else that is not
           positive becomes +0) on the float tensor, ``down``, which quantizes it to the hidden format
        4. the inverse permutation; every token's ``k`` rows times its gates, summed over ``k``

    The forward value is bit for bit ``MXMoEFeedForward``'s on the same weights (``to_inference()``): the quantizing epilogue of its
    ``up`` and the quantizer in front of this ``down`` agree by definition.  Gates, gather and un-permute are plain torch; every index
    they scatter a gradient through is a permutation (the ``k`` copies of a token are an ``expand``, whose gradient is a sum), so no
    atomic decides a bit and two runs give the same gradients.  Nothing synchronises with the host.  No auxiliary load-balancing loss,
    no capacity, no token dropping, no shared expert."""

    _up_type = MXTrainGroupedLinear     # what `up` must be, and
    _hidden_act = "relu"                # the float activation applied to its output: the hooks of MXTrainGatedMoEFeedForward (mx_glu_train.py)

    def __init__(self, router: torch.Tensor, up: MXTrainGroupedLinear, down: MXTrainGroupedLinear, top_k: int):
        super().__init__()
        if not isinstance(up, self._up_type) or not isinstance(down, MXTrainGroupedLinear):
            raise TypeError("up and down must be MXTrainGroupedLinear layers" if self._up_type is MXTrainGroupedLinear else
                            f"up must be a {self._up_type.__name__} layer and down must be MXTrainGroupedLinear")
        if not isinstance(router, torch.Tensor) or router.dim() != 2:
            raise ValueError("router must be a tensor [E, D]")
        E, D = router.shape
        H = up.out_features
        if (up.num_groups, up.in_features) != (E, D) or (down.num_groups, down.out_features, down.in_features) != (E, D, H):
            raise ValueError(f"router [E, D] = {[E, D]} needs up [E, H, D] and down [E, D, H], got "
                             f"{[up.num_groups, up.out_features, up.in_features]} and "
                             f"{[down.num_groups, down.out_features, down.in_features]}")
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= E:
            raise ValueError(f"top_k must be an int in [1, {E}], got {top_k!r}")
        self.up, self.down, self.top_k = up, down, top_k
        self.num_experts, self.embed_dim, self.hidden_dim = E, D, H
        self.router = router if isinstance(router, nn.Parameter) else nn.Parameter(router.detach().to(torch.float32))

    def extra_repr(self) -> str:
        return f"num_experts={self.num_experts}, embed_dim={self.embed_dim}, hidden_dim={self.hidden_dim}, top_k={self.top_k}"

    @classmethod
    def from_float(cls, router: torch.Tensor, w_up: torch.Tensor, b_up: Optional[torch.Tensor], w_down: torch.Tensor,
                   b_down: Optional[torch.Tensor], top_k: int, w_fmt: str = "mxfp8_e4m3", act_fmt: str = "mxfp8_e4m3",
                   hidden_fmt: str = "mxfp8_e4m3", *, grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest",
                   seed: Optional[int] = None):
        """from float tensors, the arguments of ``MXMoEFeedForward.from_float``: ``router [E, D]``, ``w_up [E, H, D]`` / ``b_up [E, H]``,
        ``w_down [E, D, H]`` / ``b_down [E, D]``, all shared with the layer, not copied"""
        opts = dict(w_fmt=w_fmt, grad_fmt=grad_fmt, out_dtype=torch.float32, grad_rounding=grad_rounding)
        up = MXTrainGroupedLinear.from_float(w_up, b_up, x_fmt=act_fmt, seed=seed, **opts)
        down = MXTrainGroupedLinear.from_float(w_down, b_down, x_fmt=hidden_fmt, seed=None if seed is None else seed + 1, **opts)
        return cls(router, up, down, top_k)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 2 or x.shape[1] != self.embed_dim:
            raise ValueError(f"x must be [T, D] with D = {self.embed_dim}, got shape {tuple(x.shape)}")
        k, E = self.top_k, self.num_experts
        top, experts = torch.topk(x.to(torch.float32) @ self.router.t(), k, -1)
        gates = torch.softmax(top, -1)
        ids = experts.reshape(-1)
        order = torch.argsort(ids, stable=True)
        offs = (ids.unsqueeze(1) == torch.arange(E, device=ids.device)).sum(0).cumsum(0).to(torch.int32)
        # row j is token order[j] // k: the k copies of every token, then a permutation
        rows = x.unsqueeze(1).expand(-1, k, -1).reshape(-1, self.embed_dim)[order]
        hidden = _act(self.up(rows, offs), self._hidden_act)
        y = self.down(hidden, offs)
        y = y[torch.argsort(order)].reshape(-1, k, self.embed_dim)
        return (y * gates.unsqueeze(-1)).sum(1)

    def to_inference(self) -> MXMoEFeedForward:
        """the ``MXMoEFeedForward`` on the current weights, in this block's formats"""
        up = self.up.to_inference(out_fmt=self.down.x_fmt, act="relu")
        return MXMoEFeedForward(self.router.detach(), up, self.down.to_inference(), self.top_k)


__all__ = ["mx_grouped_weight_grad", "mx_grouped_linear", "MXTrainGroupedLinear", "MXTrainMoEFeedForward"]
