"""Gated (SwiGLU / GeGLU) matrix products on MX codes: ``mx_glu_matmul``, ``mx_grouped_glu_matmul``, the layers ``MXGLULinear`` and
``MXGroupedGLULinear`` and the mixture-of-experts block ``MXGatedMoEFeedForward``.

The hidden layer of a gated MLP is ``h = act(x W_gate^T) * (x W_up^T)``.  Here it is ONE product on a combined weight of ``2 H`` rows
whose epilogue multiplies the two halves while they are accumulators, and writes ``H`` columns: a float tensor, or the MX codes the
next product reads (``qs_mx_glu_matmul_v`` / ``qs_mx_grouped_glu_matmul_v``).  For the gate and the up value of one hidden unit to
meet in one lane the combined weight's rows are INTERLEAVED in runs of 32 (``mx_glu_interleave``): rows ``[64 q, 64 q + 32)`` are the
gate rows of the hidden units ``[32 q, 32 q + 32)``, rows ``[64 q + 32, 64 q + 64)`` their up rows.  The weights are static, so that is
done once, when a layer is built.  ``H`` must be a multiple of 32: a block of 32 of the output is one wave's corner of the tile.

Training through the gated products is ``mx_glu_train.py``; its forward asks the products here for the pre-activations with
``preact_dtype``.  Not offered: stochastic rounding of the output, ``split_k``, the tanh GELU, gated ``mx_bmm`` /
convolutions; the ``act`` keyword of ``mx_matmul`` and its kin stays ``None`` or ``"relu"``."""
import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from qsparse_amd import _hip
from qsparse_amd._mx_common import MXActivation, _act, _check_bias_shape, _check_dtype
from qsparse_amd.mx_gemm import _check_b as _check_dense_b
from qsparse_amd.mx_gemm import _check_matmul_operands, mx_matmul
from qsparse_amd.mx_grouped import MXGroupedLinear, MXMoEFeedForward, _check_grouped_operands, _offs_int32, mx_grouped_matmul
from qsparse_amd.mx_grouped import _check_b as _check_grouped_b
from qsparse_amd.quantize import MX_BLOCK, _mx_format, quantize_with_mx

GLU_ACTS = ("silu", "gelu", "relu")
_GELU_ALPHA = math.sqrt(0.5)


def _check_hidden(H: int, what: str):
    if H % MX_BLOCK != 0:
        raise ValueError(f"{what}: H = {H} is not a multiple of {MX_BLOCK}.  The gated epilogue pairs gate and up rows in runs of "
                         f"{MX_BLOCK}, and a block of {MX_BLOCK} of the output is one wave's corner of the tile -- pad the hidden "
                         f"dimension to a multiple of {MX_BLOCK}")


def _glu_axis(t: torch.Tensor, dim: Optional[int]) -> int:
    """the axis of `t` that holds the hidden units: `dim`, or by default the rows of a weight [..., H, K] / the one axis of a 1-d bias"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"expected a tensor, got {type(t).__name__}")
    if t.dim() < 1:
        raise ValueError("the tensor needs at least one dimension")
    if dim is None:
        return 0 if t.dim() == 1 else t.dim() - 2
    if not -t.dim() <= dim < t.dim():
        raise ValueError(f"dim={dim} is out of range for a tensor of {t.dim()} dimensions")
    return dim % t.dim()


def mx_glu_interleave(gate: torch.Tensor, up: torch.Tensor, dim: Optional[int] = None) -> torch.Tensor:
    """the combined operand of the gated products from its two halves.  ``gate`` and ``up`` are weights ``[..., H, K]`` -- ``[H, K]``,
    or a stack ``[E, H, K]`` -- or 1-d biases ``[H]``, of one shape, dtype and device; the result is ``[..., 2 H, K]`` (``[2 H]``) with
    rows ``[64 q, 64 q + 32)`` = ``gate[32 q : 32 q + 32]`` and rows ``[64 q + 32, 64 q + 64)`` = ``up[32 q : 32 q + 32]``.  ``dim`` names
    the axis that holds the ``H`` hidden units where it is not the default (the second to last, or the only one): stacked biases
    ``[E, H]`` take ``dim=-1``.  It works on any dtype, so float weights can be interleaved before they are quantized, or their codes
    and scales after: the blocks run along K and are not touched.  ``H % 32 != 0`` is refused."""
    axis = _glu_axis(gate, dim)
    if not isinstance(up, torch.Tensor) or gate.shape != up.shape or gate.dtype != up.dtype or gate.device != up.device:
        raise ValueError("gate and up must be tensors that agree in shape, dtype and device")
    H = gate.shape[axis]
    _check_hidden(H, "mx_glu_interleave")
    split = tuple(gate.shape[:axis]) + (H // MX_BLOCK, 1, MX_BLOCK) + tuple(gate.shape[axis + 1:])
    both = torch.cat((gate.reshape(split), up.reshape(split)), axis + 1)
    return both.reshape(tuple(gate.shape[:axis]) + (2 * H,) + tuple(gate.shape[axis + 1:]))


def mx_glu_deinterleave(combined: torch.Tensor, dim: Optional[int] = None):
    """the inverse of ``mx_glu_interleave``: ``(gate, up)`` ``[..., H, K]`` from ``[..., 2 H, K]``, or ``[H]`` from a 1-d ``[2 H]``;
    ``dim`` as there.  The columns of a product on an interleaved weight are the weight's rows: ``mx_glu_deinterleave(y, dim=-1)``
    splits ``y [..., 2 H]`` into its gate and up halves."""
    axis = _glu_axis(combined, dim)
    N = combined.shape[axis]
    if N % (2 * MX_BLOCK) != 0:
        raise ValueError(f"mx_glu_deinterleave: {N} entries are not 2 H with H a multiple of {MX_BLOCK}: the interleave pairs runs of "
                         f"{MX_BLOCK} gate rows and {MX_BLOCK} up rows, and a block of {MX_BLOCK} of the output is one wave's corner of "
                         "the tile")
    lead, rest = tuple(combined.shape[:axis]), tuple(combined.shape[axis + 1:])
    c = combined.reshape(lead + (N // (2 * MX_BLOCK), 2, MX_BLOCK) + rest)
    return tuple(c.select(axis + 1, i).reshape(lead + (N // 2,) + rest) for i in (0, 1))


def _glu_act(g: torch.Tensor, act: str) -> torch.Tensor:
    """act(g) in torch ops, float32: what the CPU paths evaluate.  gelu is the header's expression op by op, as ``_glu_dv`` has it: ATen's
    vectorized CPU ``F.gelu`` carries an erf of 1e-7 absolute error, which the cancellation in 1 + erf turns into 2e-4 of gelu(-3),
    five times the bound that follows from the header (tests/mx_glu_ref.py)"""
    if act == "gelu":
        return (g * 0.5) * (1.0 + torch.erf(g * _GELU_ALPHA))
    return F.silu(g) if act == "silu" else _act(g, "relu")


def _check_glu(fn: str, act, out_fmt, out_dtype, b_codes, preact_dtype=None):
    if act not in GLU_ACTS:
        raise ValueError(f"unknown act {act!r}: {fn} takes one of {GLU_ACTS}")
    if preact_dtype is not None:
        _check_dtype("preact_dtype", preact_dtype)
    if out_fmt is not None:
        _mx_format(out_fmt)
        if out_dtype is not torch.float32:
            raise ValueError(f"out_dtype={out_dtype} cannot be combined with out_fmt={out_fmt!r}: the result is MX codes, leave out_dtype "
                             "at its default")
    _check_dtype("out_dtype", out_dtype)
    if isinstance(b_codes, torch.Tensor) and b_codes.dim() >= 2 and b_codes.shape[-2] % (2 * MX_BLOCK) != 0:
        raise ValueError(f"b_codes {tuple(b_codes.shape)} has {b_codes.shape[-2]} rows, not 2 H with H a multiple of {MX_BLOCK}: the gated "
                         f"product takes the {MX_BLOCK}-row interleave of mx_glu_interleave, in which a block of {MX_BLOCK} of the output "
                         "is one wave's corner of the tile")


def _glu_cpu(y: torch.Tensor, act: str, out_dtype, out_fmt):
    """the gated epilogue on the float32 product `y` [..., 2 H] by torch ops: split, act, multiply, then one rounding or the quantizer"""
    g, u = mx_glu_deinterleave(y, dim=-1)
    z = _glu_act(g, act) * u
    if out_fmt is None:
        return z.to(out_dtype)
    if z.numel() == 0:      # (the CPU quantizer takes no empty tensor)
        return z.new_empty(z.shape, dtype=torch.uint8), z.new_empty(z.shape[:-1] + (z.shape[-1] // MX_BLOCK,), dtype=torch.uint8)
    return tuple(quantize_with_mx(z, out_fmt, -1, return_codes=True)[1:])


def mx_glu_matmul(a_codes: torch.Tensor, a_scales: torch.Tensor, a_fmt: str, b_codes: torch.Tensor, b_scales: torch.Tensor, b_fmt: str,
                  bias: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32, *, act: str = "silu",
                  out_fmt: Optional[str] = None, preact_dtype: Optional[torch.dtype] = None):
    """``act(A . Wg^T + bg) * (A . Wu^T + bu)`` on MX codes in one product.  ``a_codes`` ``[..., K]`` / ``a_scales`` are
    ``mx_matmul``'s; ``b_codes`` ``[2 H, K]`` / ``b_scales`` ``[2 H, ceil(K / 32)]`` are the codes of ``mx_glu_interleave(Wg, Wu)``
    and ``bias`` float32 ``[2 H]`` is ``mx_glu_interleave(bg, bu)``.  ``act`` (keyword) is one of ``("silu", "gelu", "relu")``: SwiGLU,
    GeGLU (the erf form) and ReGLU.  Returns ``[..., H]`` in ``out_dtype``, or with ``out_fmt`` (keyword; ``out_dtype`` then stays at
    its default) the pair ``(codes uint8 [..., H], scales uint8 [..., H / 32])``.

    Definition: with ``v = mx_matmul(..., out_dtype=torch.float32)`` on the same operands and ``g, u`` its de-interleaved halves, ``z =
    act(g) * u`` in float32 -- ``g / (1 + expf(-g))``, ``(g * 0.5) * (1 + erff(g * 0.70710678...))``, or ``mx_matmul``'s ReLU (NaN
    stays NaN) -- then one rounding to ``out_dtype``, or ``quantize_with_mx(z, out_fmt, -1, return_codes=True)``.  GPU tensors take
    the HIP kernel (one launch, no float ``v`` or ``z`` in memory; no fallback: without the library the call raises) and equal that
    composition evaluated on the GPU bit for bit.  CPU tensors evaluate the composition with torch ops.  Across devices the results
    agree bit for bit only for ``act="relu"``: ``expf`` and ``erff`` are each device's own.  There is no ``split_k``.

    ``preact_dtype`` (keyword; float32, bfloat16 or float16) makes the call also keep the pre-activations, as a training forward
    needs them: the return is ``(out, v)`` with ``out`` what the call returns without the keyword, bit for bit, and ``v [..., 2 H]``
    bit for bit ``mx_matmul(..., out_dtype=preact_dtype)`` on the same operands -- the accumulator plus bias, rounded once, columns
    interleaved as the rows of ``b_codes``.  On the GPU it is still one launch (``qs_mx_glu_matmul_pre_v``)."""
    _check_glu("mx_glu_matmul", act, out_fmt, out_dtype, b_codes, preact_dtype)
    K, N = _check_matmul_operands("mx_glu_matmul", a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, bias, out_dtype)
    if not a_codes.is_cuda:
        out = _glu_cpu(mx_matmul(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, bias, torch.float32), act, out_dtype, out_fmt)
        if preact_dtype is None:
            return out
        return out, mx_matmul(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, bias, preact_dtype)
    H, lead = N // 2, tuple(a_codes.shape[:-1])
    res = _hip.mx_glu_matmul(a_codes.reshape(-1, K).contiguous(), a_scales.reshape(-1, a_scales.shape[-1]).contiguous(), a_fmt,
                             b_codes.contiguous(), b_scales.contiguous(), b_fmt, None if bias is None else bias.contiguous(), act,
                             out_dtype, out_fmt, preact_dtype=preact_dtype)
    res, v = res if preact_dtype is not None else (res, None)
    if out_fmt is None:
        res = res.reshape(lead + (H,))
    else:
        res = res[0].reshape(lead + (H,)), res[1].reshape(lead + (H // MX_BLOCK,))
    return res if v is None else (res, v.reshape(lead + (N,)))


def mx_grouped_glu_matmul(a_codes: torch.Tensor, a_scales: torch.Tensor, a_fmt: str, b_codes: torch.Tensor, b_scales: torch.Tensor,
                          b_fmt: str, offs: torch.Tensor, bias: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32, *,
                          act: str = "silu", out_fmt: Optional[str] = None, preact_dtype: Optional[torch.dtype] = None):
    """``mx_glu_matmul`` for ``E`` ragged groups of rows: ``a_codes`` ``[T, K]`` and ``offs`` ``[E]`` are ``mx_grouped_matmul``'s, with
    its boundaries ``c_e`` for ANY content of ``offs``, its clamp and its tail rule; ``b_codes`` ``[E, 2 H, K]`` holds one interleaved
    weight per group (``mx_glu_interleave`` on ``[E, H, K]`` tensors), ``bias`` is float32 ``[2 H]`` (shared) or ``[E, 2 H]``,
    interleaved likewise.  Returns ``[T, H]`` in ``out_dtype``, or with ``out_fmt`` ``(codes [T, H], scales [T, H / 32])``.

    A row of group ``e`` is bit for bit ``mx_glu_matmul`` of that row with ``b[e]`` and the bias of ``e``; the tail rows ``r >=
    c_{E-1}`` are ``+0``, or code 0 with the scale byte 0.  GPU tensors take the HIP kernel: one launch, no host synchronisation,
    ``offs`` neither read nor validated on the host (graph capture works as for ``mx_grouped_matmul``).  CPU tensors refuse an
    ``offs`` that is not nondecreasing within ``[0, T]``, as ``mx_grouped_matmul`` does, and evaluate the composition with torch ops.

    ``preact_dtype`` (keyword) as in ``mx_glu_matmul``: the return is ``(out, v)`` with ``v [T, 2 H]`` bit for bit
    ``mx_grouped_matmul(..., out_dtype=preact_dtype)`` on the same operands, ``+0`` in the tail rows (``qs_mx_grouped_glu_matmul_pre_v``)."""
    _check_glu("mx_grouped_glu_matmul", act, out_fmt, out_dtype, b_codes, preact_dtype)
    T, K, E, N = _check_grouped_operands("mx_grouped_glu_matmul", a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, offs, bias,
                                         out_dtype)
    if not a_codes.is_cuda:
        v = mx_grouped_matmul(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, offs, bias, torch.float32)
        res = _glu_cpu(v, act, out_dtype, out_fmt)
        if out_fmt is not None and E:
            tail = int(offs[-1])
            res[0][tail:], res[1][tail:] = 0, 0      # (whatever the quantizer says of a zero block: the definition)
        if preact_dtype is None:
            return res
        return res, mx_grouped_matmul(a_codes, a_scales, a_fmt, b_codes, b_scales, b_fmt, offs, bias, preact_dtype)
    return _hip.mx_grouped_glu_matmul(a_codes.contiguous(), a_scales.contiguous(), a_fmt, b_codes.contiguous(), b_scales.contiguous(),
                                      b_fmt, _offs_int32(offs, T), None if bias is None else bias.contiguous(), act, out_dtype, out_fmt,
                                      preact_dtype=preact_dtype)


def _quantize_interleaved(w_gate: torch.Tensor, w_up: torch.Tensor, w_fmt: str):
    """(codes, scales) of the interleaved weight: blocks run along K, so quantizing the interleaved rows is interleaving the codes"""
    with torch.no_grad():
        _, codes, scales = quantize_with_mx(mx_glu_interleave(w_gate.detach(), w_up.detach()), w_fmt, -1, return_codes=True)
    return codes, scales


def _interleaved_bias(b_gate, b_up):
    if (b_gate is None) != (b_up is None):
        raise ValueError("b_gate and b_up must both be given or both be None")
    if b_gate is None:
        return None
    b_gate, b_up = b_gate.detach().to(torch.float32), b_up.detach().to(torch.float32)
    return mx_glu_interleave(b_gate, b_up, dim=-1)


def _glu_input(layer, x, grouped: bool):
    """(codes, scales, fmt) of a gated layer's input: an ``MXActivation`` as it is, a float tensor through the MX quantizer"""
    name = type(layer).__name__
    if isinstance(x, MXActivation):
        if x.channels_last:
            raise ValueError(f"{name} got an MXActivation with channels_last=True: the codes of a convolution")
        return x.codes, x.scales, x.fmt
    if grouped and x.dim() != 2:
        raise ValueError(f"x must be [T, K] with K = {layer.in_features}, got shape {tuple(x.shape)}")
    _, codes, scales = quantize_with_mx(x, layer.act_fmt, -1, return_codes=True)
    return codes, scales, layer.act_fmt


class _GLUMixin:
    """what ``MXGLULinear`` and ``MXGroupedGLULinear`` share: the options, the buffers and ``repr``"""

    def _init_glu(self, fn: str, weight_codes, weight_scales, weight_fmt, bias, act_fmt, out_dtype, out_fmt, act):
        _mx_format(act_fmt)
        _check_glu(fn, act, out_fmt, out_dtype, weight_codes)
        self.weight_fmt, self.act_fmt, self.out_dtype, self.out_fmt, self.act = weight_fmt, act_fmt, out_dtype, out_fmt, act
        self.register_buffer("weight_codes", weight_codes.detach().clone().contiguous())
        self.register_buffer("weight_scales", weight_scales.detach().clone().contiguous())
        self.register_buffer("bias", None if bias is None else bias.detach().to(torch.float32).clone().contiguous())

    def extra_repr(self) -> str:
        groups = f"num_groups={self.num_groups}, " if hasattr(self, "num_groups") else ""
        return (f"{groups}in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"weight_fmt={self.weight_fmt!r}, act_fmt={self.act_fmt!r}, act={self.act!r}" +
                (f", out_fmt={self.out_fmt!r}" if self.out_fmt is not None else ""))

    def _refuse_grad(self, x):
        if not isinstance(x, MXActivation) and torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError(f"{type(self).__name__} is an inference layer: its input requires grad.  Call it under torch.no_grad()")


def _exported_weight(name: str, qt, dims: int):
    if getattr(qt, "kind", None) != "mx":
        raise ValueError(f"{name} needs an MX weight (QuantizedTensor.kind == 'mx'), got kind {getattr(qt, 'kind', None)!r}")
    if qt.codes.dim() != dims:
        raise ValueError(f"{name} needs a {dims}-d weight, got shape {tuple(qt.codes.shape)}")
    if qt.block_dim % dims != dims - 1:
        raise ValueError(f"the weight's MX blocks run along dim {qt.block_dim}, not along K (dim {dims - 1}): only blocks along K can "
                         "feed the matrix instruction")
    return qt.codes, qt.block_scale, qt.fmt


class MXGLULinear(_GLUMixin, nn.Module):
    """The hidden layer of a gated MLP for inference on MX codes: ``act(x Wg^T + bg) * (x Wu^T + bu)`` through ``mx_glu_matmul``.  The
    two weights are held as ONE set of buffers in the 32-row interleave of ``mx_glu_interleave`` -- ``weight_codes [2 H, K]``,
    ``weight_scales [2 H, ceil(K / 32)]``, ``bias [2 H]`` -- and that is what ``state_dict`` holds: ``mx_glu_deinterleave`` gives the
    halves back.  ``forward`` takes a float tensor ``[..., K]``, which it quantizes to ``act_fmt``, or an ``MXActivation``, and
    returns ``[..., H]`` in ``out_dtype`` -- or, with ``out_fmt``, an ``MXActivation``, as ``MXLinear`` does.  ``in_features`` is
    ``K``, ``out_features`` is ``H``."""

    def __init__(self, weight_codes: torch.Tensor, weight_scales: torch.Tensor, weight_fmt: str, bias: Optional[torch.Tensor] = None,
                 act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *, act: str = "silu", out_fmt: Optional[str] = None):
        super().__init__()
        _check_dense_b("weight", weight_codes, weight_scales, weight_fmt)
        if weight_codes.dim() != 2:
            raise ValueError(f"weight_codes must be [2 H, K], got shape {tuple(weight_codes.shape)}")
        _check_bias_shape(bias, weight_codes.shape[0])
        self._init_glu("MXGLULinear", weight_codes, weight_scales, weight_fmt, bias, act_fmt, out_dtype, out_fmt, act)
        self.out_features, self.in_features = weight_codes.shape[0] // 2, weight_codes.shape[1]

    @classmethod
    def from_float(cls, w_gate: torch.Tensor, w_up: torch.Tensor, b_gate: Optional[torch.Tensor] = None, b_up: Optional[torch.Tensor] = None,
                   w_fmt: str = "mxfp8_e4m3", act_fmt: str = "mxfp8_e4m3", *, act: str = "silu", out_fmt: Optional[str] = None,
                   out_dtype: torch.dtype = torch.float32):
        """from float weights ``w_gate``, ``w_up`` ``[H, K]`` (and biases ``[H]``): interleaved, then quantized with
        ``quantize_with_mx(., w_fmt, -1, return_codes=True)``, blocks along K.  The buffers hold the INTERLEAVED codes"""
        if not isinstance(w_gate, torch.Tensor) or w_gate.dim() != 2:
            raise ValueError("MXGLULinear.from_float needs weight tensors [H, K]")
        codes, scales = _quantize_interleaved(w_gate, w_up, w_fmt)
        return cls(codes, scales, w_fmt, _interleaved_bias(b_gate, b_up), act_fmt, out_dtype, act=act, out_fmt=out_fmt)

    @classmethod
    def from_exported(cls, qt, bias: Optional[torch.Tensor] = None, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *,
                      act: str = "silu", out_fmt: Optional[str] = None):
        """from a ``QuantizedTensor(kind="mx")`` that holds the ALREADY INTERLEAVED weight ``[2 H, K]`` with blocks along K, and the
        interleaved ``bias [2 H]``"""
        return cls(*_exported_weight("MXGLULinear", qt, 2), bias, act_fmt, out_dtype, act=act, out_fmt=out_fmt)

    def forward(self, x):
        self._refuse_grad(x)
        with torch.no_grad():
            codes, scales, fmt = _glu_input(self, x, False)
            y = mx_glu_matmul(codes, scales, fmt, self.weight_codes, self.weight_scales, self.weight_fmt, self.bias, self.out_dtype,
                              act=self.act, out_fmt=self.out_fmt)
            return y if self.out_fmt is None else MXActivation(*y, self.out_fmt)


class MXGroupedGLULinear(_GLUMixin, nn.Module):
    """``E`` gated hidden layers applied to ragged groups of rows through ``mx_grouped_glu_matmul``: ``weight_codes [E, 2 H, K]``,
    ``weight_scales [E, 2 H, ceil(K / 32)]`` and ``bias [E, 2 H]`` are buffers in the 32-row interleave of ``mx_glu_interleave``,
    and that is what ``state_dict`` holds.  ``forward(x, offs)`` takes a float ``x [T, K]`` or an ``MXActivation`` and the cumulative
    group ends of ``mx_grouped_matmul``, and returns ``[T, H]`` in ``out_dtype`` or, with ``out_fmt``, an ``MXActivation``.
    ``num_groups`` is ``E``, ``in_features`` ``K``, ``out_features`` ``H``."""

    def __init__(self, weight_codes: torch.Tensor, weight_scales: torch.Tensor, weight_fmt: str, bias: Optional[torch.Tensor] = None,
                 act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *, act: str = "silu", out_fmt: Optional[str] = None):
        super().__init__()
        _check_grouped_b("weight", weight_codes, weight_scales, weight_fmt)
        E, N, K = weight_codes.shape
        if bias is not None and tuple(bias.shape) != (E, N):
            raise ValueError(f"bias has shape {tuple(bias.shape)}, expected {(E, N)}")
        self._init_glu("MXGroupedGLULinear", weight_codes, weight_scales, weight_fmt, bias, act_fmt, out_dtype, out_fmt, act)
        self.num_groups, self.out_features, self.in_features = E, N // 2, K

    @classmethod
    def from_float(cls, w_gate: torch.Tensor, w_up: torch.Tensor, b_gate: Optional[torch.Tensor] = None, b_up: Optional[torch.Tensor] = None,
                   w_fmt: str = "mxfp8_e4m3", act_fmt: str = "mxfp8_e4m3", *, act: str = "silu", out_fmt: Optional[str] = None,
                   out_dtype: torch.dtype = torch.float32):
        """from float weights ``w_gate``, ``w_up`` ``[E, H, K]`` (and biases ``[E, H]``): interleaved per group, then quantized with
        blocks along K.  The buffers hold the INTERLEAVED codes"""
        if not isinstance(w_gate, torch.Tensor) or w_gate.dim() != 3:
            raise ValueError("MXGroupedGLULinear.from_float needs weight tensors [E, H, K]")
        codes, scales = _quantize_interleaved(w_gate, w_up, w_fmt)
        return cls(codes, scales, w_fmt, _interleaved_bias(b_gate, b_up), act_fmt, out_dtype, act=act, out_fmt=out_fmt)

    @classmethod
    def from_exported(cls, qt, bias: Optional[torch.Tensor] = None, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32, *,
                      act: str = "silu", out_fmt: Optional[str] = None):
        """from a ``QuantizedTensor(kind="mx")`` that holds the stacked, ALREADY INTERLEAVED weights ``[E, 2 H, K]`` with blocks along
        K, and the interleaved ``bias [E, 2 H]``"""
        return cls(*_exported_weight("MXGroupedGLULinear", qt, 3), bias, act_fmt, out_dtype, act=act, out_fmt=out_fmt)

    def forward(self, x, offs: torch.Tensor):
        self._refuse_grad(x)
        with torch.no_grad():
            codes, scales, fmt = _glu_input(self, x, True)
            y = mx_grouped_glu_matmul(codes, scales, fmt, self.weight_codes, self.weight_scales, self.weight_fmt, offs, self.bias,
                                      self.out_dtype, act=self.act, out_fmt=self.out_fmt)
            return y if self.out_fmt is None else MXActivation(*y, self.out_fmt)


class MXGatedMoEFeedForward(MXMoEFeedForward):
    """``MXMoEFeedForward`` with a gated hidden layer -- the feed-forward block of current mixture-of-experts models: ``up`` is an
    ``MXGroupedGLULinear`` ``[E, 2 H, D]`` that hands MX codes of ``act(x Wg^T) * (x Wu^T)`` to ``down``, an ``MXGroupedLinear`` ``[E, D,
    H]`` that returns float32.  The routing, the permutation and the combination are ``MXMoEFeedForward.forward``'s, the same code.
    ``state_dict`` keys are ``MXMoEFeedForward``'s; ``up.weight_codes``, ``up.weight_scales`` and ``up.bias`` hold the INTERLEAVED gate
    and up rows (``mx_glu_interleave``)."""

    _up_type = MXGroupedGLULinear

    @classmethod
    def from_float(cls, router: torch.Tensor, w_gate: torch.Tensor, b_gate: Optional[torch.Tensor], w_up: torch.Tensor,
                   b_up: Optional[torch.Tensor], w_down: torch.Tensor, b_down: Optional[torch.Tensor], top_k: int,
                   w_fmt: str = "mxfp8_e4m3", act_fmt: str = "mxfp8_e4m3", hidden_fmt: str = "mxfp8_e4m3", *, act: str = "silu"):
        """from float tensors: ``router [E, D]``, ``w_gate``, ``w_up`` ``[E, H, D]`` / ``b_gate``, ``b_up`` ``[E, H]``, ``w_down [E, D,
        H]`` / ``b_down [E, D]``.  The hidden activation ``act(gate) * up`` is quantized to ``hidden_fmt`` by ``up``'s epilogue"""
        up = MXGroupedGLULinear.from_float(w_gate, w_up, b_gate, b_up, w_fmt, act_fmt, act=act, out_fmt=hidden_fmt)
        down = MXGroupedLinear.from_float(w_down, b_down, w_fmt, hidden_fmt)
        return cls(router, up, down, top_k)


__all__ = ["mx_glu_interleave", "mx_glu_deinterleave", "mx_glu_matmul", "mx_grouped_glu_matmul", "MXGLULinear", "MXGroupedGLULinear",
           "MXGatedMoEFeedForward", "GLU_ACTS"]
