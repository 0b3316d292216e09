"""Grouped (ragged) matrix products on MX codes: ``mx_grouped_matmul``, the layer ``MXGroupedLinear`` and the inference-side
mixture-of-experts block ``MXMoEFeedForward`` built on it.

``mx_matmul`` multiplies an activation by ONE weight, ``mx_bmm`` equal-sized slices by one weight each.  After the routing of a
mixture-of-experts layer expert ``e`` owns ``n_e`` rows of the token matrix; the ``n_e`` differ, some are 0, they change every step and
they are known only on the device.  ``mx_grouped_matmul`` takes the rows of all groups in one ``[T, K]`` operand, one weight per group
and the cumulative group ENDS as a device tensor, and multiplies in one launch (``qs_mx_grouped_matmul_v``) without reading the
boundaries on the host.  Row by row it computes bit for bit what ``mx_matmul`` computes with the row's group's weight.  The argument
checks are ``_mx_common.py``'s."""
from functools import partial
from typing import Optional

import torch
import torch.nn as nn

from qsparse_amd import _hip, _mx_common
from qsparse_amd._mx_common import MXActivation, _check_codes_out, _check_dtype, _codes_out_cpu
from qsparse_amd.quantize import _mx_format, mx_dequantize, quantize_with_mx

_check_a = partial(_mx_common._check_operand, what="[T, K]", least=2, most=2, needs="2 dimensions")
_check_b = partial(_mx_common._check_operand, what="[E, N, K]", least=3, most=3, needs="3 dimensions")


def _offs_int32(offs: torch.Tensor, T: int) -> torch.Tensor:
    """the int32 boundaries the kernel reads, on the device of ``offs`` and without a host read.  An int64 entry is clamped into ``[0,
    min(T, 2^31 - 1)]`` BEFORE it is narrowed (a plain ``.to(torch.int32)`` wraps: 2^31 would become -2^31).  The boundaries ``c_e`` are a
    running maximum that starts at 0 and is capped at T, so clamping every entry into ``[0, T]`` first changes none of them."""
    if offs.dtype == torch.int64:
        offs = offs.clamp(0, min(T, 2 ** 31 - 1))
    return offs.to(torch.int32).contiguous()


def _check_grouped_operands(fn: str, a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, offs, bias, out_dtype):
    """the operands, `offs`, the bias and `out_dtype` of `mx_grouped_matmul`, and of `mx_grouped_glu_matmul` (mx_glu.py), which is `fn`
    then; returns (T, K, E, N)"""
    _check_a("a", a_codes, a_scales, a_fmt)
    if isinstance(b_codes, torch.Tensor) and b_codes.dim() == 2:
        raise ValueError(f"b_codes must be [E, N, K], one weight per group, got shape {tuple(b_codes.shape)}: one weight [N, K] shared "
                         "by every row of a is mx_matmul")
    _check_b("b", b_codes, b_scales, b_fmt)
    (T, K), (E, N, _) = a_codes.shape, b_codes.shape
    if b_codes.shape[-1] != K:
        raise ValueError(f"a_codes {tuple(a_codes.shape)} and b_codes {tuple(b_codes.shape)} disagree on K (their last dimensions)")
    if K < 1:
        raise ValueError(f"{fn} needs K >= 1")
    if b_codes.device != a_codes.device:
        raise ValueError(f"a_codes is on {a_codes.device} but b_codes on {b_codes.device}")
    if not isinstance(offs, torch.Tensor):
        raise TypeError(f"offs must be a tensor, got {type(offs).__name__}")
    if offs.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"offs must be an int32 or int64 tensor (the cumulative end row of every group), got {offs.dtype}")
    if tuple(offs.shape) != (E,):
        raise ValueError(f"offs has shape {tuple(offs.shape)}, expected ({E},): one cumulative end row per weight of b_codes "
                         f"{tuple(b_codes.shape)}")
    if offs.device != a_codes.device:
        raise ValueError(f"a_codes is on {a_codes.device} but offs on {offs.device}")
    _check_dtype("out_dtype", out_dtype)
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
            raise TypeError("bias must be a float32 tensor")
        if tuple(bias.shape) not in ((N,), (E, N)):
            raise ValueError(f"bias has shape {tuple(bias.shape)}, expected ({N},) or {(E, N)}")
        if bias.device != a_codes.device:
            raise ValueError(f"a_codes is on {a_codes.device} but bias on {bias.device}")
    return T, K, E, N


def mx_grouped_matmul(a_codes: torch.Tensor, a_scales: torch.Tensor, a_fmt: str, b_codes: torch.Tensor, b_scales: torch.Tensor, b_fmt: str,
                      offs: torch.Tensor, bias: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32, *,
                      out_fmt: Optional[str] = None, act: Optional[str] = None):
    """``A[group e] . B[e]^T (+ bias[e])`` on MX codes for ``E`` groups of rows of different sizes.  ``a_codes`` ``[T, K]`` holds the
    rows of all groups, group after group, ``b_codes`` ``[E, N, K]`` one weight per group (uint8 codes of the formats ``a_fmt`` /
    ``b_fmt`` of ``MX_FORMATS``, which may differ, with blocks along K), ``a_scales`` ``[T, ceil(K / 32)]`` and ``b_scales`` ``[E, N,
    ceil(K / 32)]`` their E8M0 bytes, ``bias`` float32 ``[N]`` (shared by the groups) or ``[E, N]``.  ``offs`` is an int32 or int64
    tensor ``[E]`` on the operands' device: the cumulative END row of every group, the convention of torch's grouped mm.  Returns ``[T,
    N]`` in ``out_dtype`` (float32, bfloat16 or float16).

    Boundaries: with ``c_-1 = 0`` and ``c_e = min(max(offs[e], c_{e-1}), T)`` group ``e`` is the rows ``[c_{e-1}, c_e)``.  A row of
    group ``e`` is bit for bit ``mx_matmul`` of that row with ``b[e]`` and the bias of ``e``, on either device.  The TAIL rows ``r >=
    c_{E-1}`` belong to no group and are ``+0`` without a bias -- what a capacity-padded token buffer needs.

    GPU tensors take the HIP kernel: one launch for all groups, no synchronisation, and ``offs`` is neither read on the host nor
    validated (an int64 one is clamped into ``[0, min(T, 2^31 - 1)]`` and then narrowed to int32, on the device: narrowing alone would
    wrap an entry beyond int32, and the clamp changes no ``c_e``), so the call can be captured in a graph and replayed with other
    boundaries written into the same tensor.  The clamp above is the kernel's: the groups partition ``[0, c_{E-1})`` for ANY content of
    ``offs``, a non-monotone or out-of-range one gives the result of the clamped boundaries and never a fault.  There is no fallback:
    without the library the call raises.  CPU tensors refuse an ``offs`` that is not nondecreasing within ``[0, T]`` with a
    ``ValueError``, then evaluate ``mx_matmul``'s float64 expression group by group and round once.

    ``out_fmt`` / ``act`` (keywords) are ``mx_matmul``'s: with ``out_fmt`` the return is ``(codes uint8 [T, N], scales uint8 [T, ceil(N /
    32)])``, the codes of ``quantize_with_mx(act(y), out_fmt, -1, return_codes=True)`` with ``y`` the float32 result, written by the
    product's epilogue on the GPU (``qs_mx_grouped_matmul_q_v``); the tail rows are code 0 with the scale byte 0.  ``act`` is ``None``
    or ``"relu"`` and needs ``out_fmt``, and ``out_dtype`` stays at its default.  There is no ``split_k``."""
    _check_codes_out("mx_grouped_matmul", out_fmt, act, out_dtype)
    T, K, E, N = _check_grouped_operands("mx_grouped_matmul", a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, offs, bias, out_dtype)
    if a_codes.is_cuda:
        ops = (a_codes.contiguous(), a_scales.contiguous(), a_fmt, b_codes.contiguous(), b_scales.contiguous(), b_fmt,
               _offs_int32(offs, T), None if bias is None else bias.contiguous())
        if out_fmt is not None:
            return _hip.mx_grouped_matmul_q(*ops, out_fmt, act)
        return _hip.mx_grouped_matmul(*ops, out_dtype)
    ends = [int(v) for v in offs.tolist()]
    if any(hi < lo for lo, hi in zip([0] + ends, ends + [T])):
        raise ValueError(f"offs must be nondecreasing within [0, {T}] (cumulative group ends over the {T} rows of a_codes), got {ends}")
    y = torch.zeros((T, N), dtype=out_dtype)        # (the tail: +0)
    for e, (lo, hi) in enumerate(zip([0] + ends, ends)):      # group by group, the expression of mx_matmul's CPU path: the same bits
        if hi > lo:
            ye = mx_dequantize(a_codes[lo:hi], a_scales[lo:hi], a_fmt, -1, torch.float64) @ \
                mx_dequantize(b_codes[e], b_scales[e], b_fmt, -1, torch.float64).t()
            if bias is not None:
                ye = ye + (bias[e] if bias.dim() > 1 else bias).to(torch.float64)
            y[lo:hi] = ye.to(out_dtype)
    if out_fmt is not None and y.numel() == 0:      # (the CPU quantizer takes no empty tensor)
        return y.new_empty(y.shape, dtype=torch.uint8), y.new_empty((T, (N + 31) // 32), dtype=torch.uint8)
    if out_fmt is None:
        return y
    codes, scales = _codes_out_cpu(y, out_fmt, act)
    tail = ends[-1] if ends else 0
    codes[tail:], scales[tail:] = 0, 0              # (whatever the quantizer says of a zero block: the definition)
    return codes, scales


class MXGroupedLinear(nn.Module):
    """``E`` linear layers for inference on MX codes, applied to ragged groups of rows: the weights are held as uint8 codes
    ``weight_codes [E, N, K]`` and E8M0 scales ``weight_scales [E, N, ceil(K / 32)]`` of the format ``weight_fmt`` (buffers, with the
    optional float32 ``bias [E, N]``).  ``forward(x, offs)`` takes a float ``x [T, K]``, which it quantizes to ``act_fmt`` along K with
    the MX quantizer (``quantize_with_mx``), or an ``MXActivation``, whose codes are multiplied as they are, and the cumulative group
    ends ``offs [E]`` of ``mx_grouped_matmul``, and returns ``[T, N]`` in ``out_dtype`` -- or, with ``out_fmt`` (optionally
    ``act="relu"``), an ``MXActivation``.  This is how ``MXLinear`` behaves; group ``e`` of the result is bit for bit ``MXLinear`` of
    weight ``e`` on the group's rows.  The output never requires grad, and an input that requires grad while gradients are enabled is
    refused."""

    def __init__(self, weight_codes: torch.Tensor, weight_scales: torch.Tensor, weight_fmt: str, bias: Optional[torch.Tensor] = None,
                 act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *, out_fmt: Optional[str] = None,
                 act: Optional[str] = None):
        super().__init__()
        _mx_format(act_fmt)
        _check_codes_out("MXGroupedLinear", out_fmt, act, out_dtype)
        _check_dtype("out_dtype", out_dtype)
        _check_b("weight", weight_codes, weight_scales, weight_fmt)
        E, N, K = weight_codes.shape
        if bias is not None and tuple(bias.shape) != (E, N):
            raise ValueError(f"bias has shape {tuple(bias.shape)}, expected {(E, N)}")
        self.weight_fmt, self.act_fmt, self.out_dtype, self.out_fmt, self.act = weight_fmt, act_fmt, out_dtype, out_fmt, act
        self.num_groups, self.out_features, self.in_features = E, N, K
        self.register_buffer("weight_codes", weight_codes.detach().clone().contiguous())
        self.register_buffer("weight_scales", weight_scales.detach().clone().contiguous())
        self.register_buffer("bias", None if bias is None else bias.detach().to(torch.float32).clone().contiguous())

    def extra_repr(self) -> str:
        return (f"num_groups={self.num_groups}, in_features={self.in_features}, out_features={self.out_features}, "
                f"bias={self.bias is not None}, weight_fmt={self.weight_fmt!r}, act_fmt={self.act_fmt!r}" +
                (f", out_fmt={self.out_fmt!r}" if self.out_fmt is not None else "") + (f", act={self.act!r}" if self.act is not None else ""))

    @classmethod
    def from_float(cls, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, w_fmt: str = "mxfp8_e4m3", act_fmt: str = "mxfp8_e4m3",
                   out_fmt: Optional[str] = None, act: Optional[str] = None):
        """from float weights ``[E, N, K]`` (and biases ``[E, N]``): quantized with ``quantize_with_mx(weight, w_fmt, -1,
        return_codes=True)``, blocks along K"""
        if not isinstance(weight, torch.Tensor) or weight.dim() != 3:
            raise ValueError("MXGroupedLinear.from_float needs a weight tensor [E, N, K], got " +
                             (f"shape {tuple(weight.shape)}" if isinstance(weight, torch.Tensor) else type(weight).__name__))
        with torch.no_grad():
            _, codes, scales = quantize_with_mx(weight.detach(), w_fmt, -1, return_codes=True)
        return cls(codes, scales, w_fmt, None if bias is None else bias.detach(), act_fmt, out_fmt=out_fmt, act=act)

    @classmethod
    def from_exported(cls, qt, bias: Optional[torch.Tensor] = None, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *,
                      out_fmt: Optional[str] = None, act: Optional[str] = None):
        """from a ``QuantizedTensor(kind="mx")`` that holds the stacked weights ``[E, N, K]`` with blocks along K"""
        if getattr(qt, "kind", None) != "mx":
            raise ValueError(f"MXGroupedLinear needs an MX weight (QuantizedTensor.kind == 'mx'), got kind {getattr(qt, 'kind', None)!r}")
        if qt.codes.dim() != 3:
            raise ValueError(f"MXGroupedLinear needs a 3-d weight [E, N, K], got shape {tuple(qt.codes.shape)}")
        if qt.block_dim % qt.codes.dim() != 2:
            raise ValueError(f"the weight's MX blocks run along dim {qt.block_dim}, not along K (dim 2): only blocks along K can feed the "
                             "matrix instruction")
        return cls(qt.codes, qt.block_scale, qt.fmt, bias, act_fmt, out_dtype, out_fmt=out_fmt, act=act)

    def forward(self, x, offs: torch.Tensor):
        taken = isinstance(x, MXActivation)
        if not taken and torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("MXGroupedLinear is an inference layer: its input requires grad.  Call it under torch.no_grad()")
        with torch.no_grad():
            if taken:
                if x.channels_last:
                    raise ValueError("MXGroupedLinear got an MXActivation with channels_last=True: the codes of a convolution")
                codes, scales, fmt = x.codes, x.scales, x.fmt
            else:
                fmt = self.act_fmt
                if x.dim() != 2:
                    raise ValueError(f"x must be [T, K] with K = {self.in_features}, got shape {tuple(x.shape)}")
                _, codes, scales = quantize_with_mx(x, fmt, -1, return_codes=True)
            y = mx_grouped_matmul(codes, scales, fmt, self.weight_codes, self.weight_scales, self.weight_fmt, offs, self.bias,
                                  self.out_dtype, out_fmt=self.out_fmt, act=self.act)
            return y if self.out_fmt is None else MXActivation(*y, self.out_fmt)


class MXMoEFeedForward(nn.Module):
    """An inference-side top-``k`` mixture-of-experts feed-forward block on MX codes: a float32 ``router [E, D]`` (a buffer), an
    ``MXGroupedLinear`` ``up`` ``[E, H, D]`` that hands out MX codes (``out_fmt``; ``act="relu"`` as ``from_float`` builds it) and an
    ``MXGroupedLinear`` ``down`` ``[E, D, H]`` that returns float32.  ``forward(x)`` takes ``x [T, D]`` -- a float tensor or an
    ``MXActivation`` -- and returns float32 ``[T, D]``.  It is DEFINED as this composition of public calls, and is bit for bit that
    composition:

        1. ``logits = x32 @ router.t()`` in float32 (``x32``: the float input, or the de-quantized ``MXActivation``); ``topk(logits,
           k)``, then the softmax over the ``k`` kept logits: the gates ``[T, k]``
        2. a stable argsort of the ``T k`` expert ids; the counts per expert and their cumulative sum ``offs`` on the device
        3. the rows gathered in that order (row ``j`` is token ``order[j] // k``); ``up(rows, offs)``, then ``down(., offs)``: MX codes
           pass between the two
        4. the inverse permutation as a gather; every token's ``k`` rows times its gates, summed over ``k``

    Nothing in it synchronises with the host (the counts are a comparison against ``arange(E)`` summed, not ``torch.bincount``), so it
    can be captured in a graph, and nothing in it is an atomic or an ``index_add_``: the same bits on every run.  No capacity, no token
    dropping, no shared expert, no training.  ``state_dict`` keys: ``router``, ``up.weight_codes``, ``up.weight_scales``, ``up.bias``,
    ``down.weight_codes``, ``down.weight_scales``, ``down.bias`` (a bias only where the layer has one)."""

    _up_type = MXGroupedLinear      # what `up` must be: the gated block (mx_glu.py) derives from this one and names its own

    def __init__(self, router: torch.Tensor, up: MXGroupedLinear, down: MXGroupedLinear, top_k: int):
        super().__init__()
        if not isinstance(up, self._up_type) or not isinstance(down, MXGroupedLinear):
            raise TypeError("up and down must be MXGroupedLinear layers" if self._up_type is MXGroupedLinear else
                            f"up must be an {self._up_type.__name__} layer and down an MXGroupedLinear layer")
        if not isinstance(router, torch.Tensor) or router.dim() != 2:
            raise ValueError("router must be a tensor [E, D]")
        E, D = router.shape
        H = up.out_features
        if (up.num_groups, up.in_features) != (E, D) or (down.num_groups, down.out_features, down.in_features) != (E, D, H):
            raise ValueError(f"router [E, D] = {[E, D]} needs up [E, H, D] and down [E, D, H], got "
                             f"{[up.num_groups, up.out_features, up.in_features]} and "
                             f"{[down.num_groups, down.out_features, down.in_features]}")
        if up.out_fmt is None:
            raise ValueError("up must hand out MX codes (out_fmt): they pass to down as they are")
        if down.out_fmt is not None or down.out_dtype is not torch.float32:
            raise ValueError("down must return float32 (no out_fmt, out_dtype=torch.float32): the gates weight its rows in float32")
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= E:
            raise ValueError(f"top_k must be an int in [1, {E}], got {top_k!r}")
        self.up, self.down, self.top_k = up, down, top_k
        self.num_experts, self.embed_dim, self.hidden_dim = E, D, H
        self.register_buffer("router", router.detach().to(torch.float32).clone().contiguous())

    def extra_repr(self) -> str:
        return f"num_experts={self.num_experts}, embed_dim={self.embed_dim}, hidden_dim={self.hidden_dim}, top_k={self.top_k}"

    @classmethod
    def from_float(cls, router: torch.Tensor, w_up: torch.Tensor, b_up: Optional[torch.Tensor], w_down: torch.Tensor,
                   b_down: Optional[torch.Tensor], top_k: int, w_fmt: str = "mxfp8_e4m3", act_fmt: str = "mxfp8_e4m3",
                   hidden_fmt: str = "mxfp8_e4m3"):
        """from float tensors: ``router [E, D]``, ``w_up [E, H, D]`` / ``b_up [E, H]``, ``w_down [E, D, H]`` / ``b_down [E, D]``.  The
        hidden activation is ReLU, quantized to ``hidden_fmt`` by ``up``'s epilogue"""
        up = MXGroupedLinear.from_float(w_up, b_up, w_fmt, act_fmt, out_fmt=hidden_fmt, act="relu")
        down = MXGroupedLinear.from_float(w_down, b_down, w_fmt, hidden_fmt)
        return cls(router, up, down, top_k)

    def forward(self, x):
        taken = isinstance(x, MXActivation)
        if not taken and torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError(f"{type(self).__name__} is an inference layer: its input requires grad.  Call it under torch.no_grad()")
        with torch.no_grad():
            x32 = x.dequantize() if taken else x.to(torch.float32)
            if x32.dim() != 2 or x32.shape[1] != self.embed_dim:
                raise ValueError(f"x must be [T, D] with D = {self.embed_dim}, got shape {tuple(x32.shape)}")
            k, E = self.top_k, self.num_experts
            top, experts = torch.topk(x32 @ self.router.t(), k, -1)
            gates = torch.softmax(top, -1)
            ids = experts.reshape(-1)
            order = torch.argsort(ids, stable=True)
            offs = (ids.unsqueeze(1) == torch.arange(E, device=ids.device)).sum(0).cumsum(0).to(torch.int32)
            token = torch.div(order, k, rounding_mode="floor")
            rows = MXActivation(x.codes[token], x.scales[token], x.fmt) if taken else x[token]
            y = self.down(self.up(rows, offs), offs)
            y = y[torch.argsort(order)].reshape(-1, k, self.embed_dim)
            return (y * gates.unsqueeze(-1)).sum(1)


__all__ = ["mx_grouped_matmul", "MXGroupedLinear", "MXMoEFeedForward"]
