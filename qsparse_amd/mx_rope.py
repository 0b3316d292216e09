"""Rotary position embedding in front of the MX quantizer: ``mx_rope_table``, ``mx_rope`` and ``mx_rope_quantize``.

A Llama-style model rotates ``q`` and ``k`` before attention.  In torch that is a chain of five or six launches that writes the rotated
float tensors, which ``mx_quantize_2way_batched`` then reads back.  ``mx_rope_quantize`` is that quantizer with the rotation as its
load step -- the rotated float32 values exist only in registers -- and ``mx_rope`` the rotation alone, differentiable, for the places
that need the float (the ``"torch"`` attention, the gradients of the fused one).  The definition (``include/qsparse_hip.h``, "MX rotary
embedding") is a fixed sequence of float32 operations, so the CPU path, which evaluates it in torch ops, and the HIP kernels agree bit
for bit."""
import math
from typing import Optional

import torch

from qsparse_amd import _hip
from qsparse_amd._mx_common import _check_dtype
from qsparse_amd.mx_batched_train import _slice_strides, mx_quantize_2way_batched
from qsparse_amd.quantize import MX_BLOCK, _mx_format


def mx_rope_table(T: int, d: int, *, base: float = 10000.0, positions: Optional[torch.Tensor] = None, device=None):
    """The tables ``(cos, sin)``, float32 ``[T, d / 2]``, of ``mx_rope``: the angle of row ``t`` and pair ``j`` is ``positions[t] *
    base ** (-2 j / d)``, evaluated on the CPU in float64 and rounded ONCE to float32 -- the tables do not depend on a device's
    ``cosf``.  ``positions`` (``T`` numbers, any real or integer dtype; a 1-d tensor or a sequence) defaults to ``arange(T)``; ``device``
    is where the tables are put."""
    for name, n in (("T", T), ("d", d)):
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError(f"{name} must be an int >= 0, got {n!r}")
    if d < 2 or d % 2:
        raise ValueError(f"mx_rope_table needs an even d >= 2, got {d}")
    if isinstance(base, bool) or not isinstance(base, (int, float)) or not base > 0 or math.isinf(base):
        raise ValueError(f"base must be a finite number > 0, got {base!r}")
    if positions is None:
        pos = torch.arange(T, dtype=torch.float64)
    else:
        pos = torch.as_tensor(positions).detach().to(device="cpu", dtype=torch.float64)
        if pos.dim() != 1 or pos.numel() != T:
            raise ValueError(f"positions must hold T = {T} numbers in one dimension, got shape {tuple(pos.shape)}")
    inv = torch.tensor(float(base), dtype=torch.float64) ** (torch.arange(d // 2, dtype=torch.float64) * (-2.0 / d))
    ang = pos[:, None] * inv[None, :]
    return ang.cos().to(torch.float32).to(device), ang.sin().to(torch.float32).to(device)


def _check_rope(fn: str, x, cos, sin):
    """the operand checks `mx_rope` and `mx_rope_quantize` share"""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a tensor, got {type(x).__name__}")
    _check_dtype("x", x.dtype)
    if x.dim() < 2:
        raise ValueError(f"{fn} needs x [..., T, d] with at least 2 dimensions, got shape {tuple(x.shape)}")
    T, d = x.shape[-2:]
    if d < 2 or d % 2:
        raise ValueError(f"{fn} needs an even d >= 2 (the last dimension of x), got {d}")
    _check_tables(cos, sin, T, d, x.device)


def _check_tables(cos, sin, T: int, d: int, device, names=("cos", "sin")):
    for name, t in zip(names, (cos, sin)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if tuple(t.shape) != (T, d // 2):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [T, d / 2] = {(T, d // 2)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.device != device:
            raise ValueError(f"x is on {device} but {name} on {t.device}")
        if t.requires_grad:
            raise RuntimeError(f"{name} requires grad: the tables of mx_rope get no gradient")


def _rope_def(x32: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, interleaved: bool, inverse: bool) -> torch.Tensor:
    """the definition on a float32 `x32` [..., T, d], one torch op per float32 operation"""
    s = -sin if inverse else sin
    if interleaved:
        a, b = x32[..., 0::2], x32[..., 1::2]
    else:
        h = x32.shape[-1] // 2
        a, b = x32[..., :h], x32[..., h:]
    ya = a * cos - b * s
    yb = b * cos + a * s
    return torch.stack((ya, yb), -1).flatten(-2) if interleaved else torch.cat((ya, yb), -1)


def _strided(x: torch.Tensor):
    """(x, G0, G1, strides): `x` as the kernels address it -- where it lies if `_slice_strides` allows, else a contiguous copy"""
    plan = _slice_strides(x)
    if plan is None:
        x = x.contiguous()
        plan = _slice_strides(x)
    return (x,) + plan


def _rope_forward(x: torch.Tensor, cos, sin, interleaved: bool, inverse: bool, out_dtype: torch.dtype) -> torch.Tensor:
    x = x.detach()
    if x.is_cuda:
        xs, G0, G1, strides = _strided(x)
        T, d = x.shape[-2:]
        return _hip.mx_rope(xs, G0, G1, T, d, strides, cos, sin, interleaved, inverse, out_dtype).view(x.shape)
    return _rope_def(x.to(torch.float32), cos, sin, interleaved, inverse).to(out_dtype)


class _MXRopeFunction(torch.autograd.Function):
    """`mx_rope` with its inverse as its backward"""

    @staticmethod
    def forward(ctx, x, cos, sin, interleaved, inverse, out_dtype):
        ctx.tables, ctx.flags, ctx.x_dtype = (cos, sin), (interleaved, inverse), x.dtype
        return _rope_forward(x, cos, sin, interleaved, inverse, out_dtype)

    @staticmethod
    def backward(ctx, dy):
        interleaved, inverse = ctx.flags
        return mx_rope(dy, *ctx.tables, interleaved=interleaved, inverse=not inverse, out_dtype=ctx.x_dtype), None, None, None, None, None


def mx_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, interleaved: bool = False, inverse: bool = False,
            out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Rotary position embedding of ``x [..., T, d]`` (float32 / bfloat16 / float16, ``d`` even, ``h = d / 2``) by the float32 tables
    ``cos``, ``sin`` ``[T, h]`` (``mx_rope_table``; contiguous, on ``x``'s device, shared by all leading dimensions): the dense rotation
    ``[..., T, d]``, rounded once from float32 to ``out_dtype`` (by default ``x.dtype``).

    Pair ``j`` of a row is ``(a, b) = (x[j], x[j + h])`` and lands in ``y[j]``, ``y[j + h]`` (``interleaved=False``: the rotate-half
    form of Llama / NeoX), or ``(x[2 j], x[2 j + 1])`` landing in ``y[2 j]``, ``y[2 j + 1]`` (``interleaved=True``: GPT-J).  With ``c =
    cos[t, j]``, ``s = sin[t, j]`` and every operation a float32 operation rounded on its own:

        y_a = (a * c) - (b * s)
        y_b = (b * c) + (a * s)

    ``inverse=True`` uses ``-s``: bit for bit the same call with ``-sin``, and exactly the gradient of the forward with respect to ``x``.
    So the call is differentiable in ``x`` -- its backward is ``mx_rope(dy, cos, sin, interleaved=interleaved, inverse=not inverse,
    out_dtype=x.dtype)`` -- and a table that requires grad is refused.  NaN, Inf and signed zeros follow from the operations.

    GPU tensors take the HIP kernel (``qs_mx_rope_v``; no fallback): ONE launch.  ``x`` is read where it lies when
    ``mx_quantize_2way_batched`` would read it so (a ``[B, T, h, d].transpose(1, 2)``, a ``chunk`` of a packed projection) and through
    ``contiguous()`` otherwise.  CPU tensors evaluate the definition in torch ops; both give the same bits."""
    _check_rope("mx_rope", x, cos, sin)
    out_dtype = x.dtype if out_dtype is None else out_dtype
    _check_dtype("out_dtype", out_dtype)
    interleaved, inverse = bool(interleaved), bool(inverse)
    if torch.is_grad_enabled() and x.requires_grad:
        return _MXRopeFunction.apply(x, cos, sin, interleaved, inverse, out_dtype)
    return _rope_forward(x, cos, sin, interleaved, inverse, out_dtype)


def mx_rope_quantize(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, row_fmt: Optional[str] = None,
                     col_fmt: Optional[str] = None, interleaved: bool = False, inverse: bool = False):
    """``mx_quantize_2way_batched(mx_rope(x, cos, sin, interleaved=, inverse=, out_dtype=torch.float32), row_fmt, col_fmt)``, bit for
    bit: ``(row_codes [..., T, d], row_scales [..., T, ceil(d / 32)], col_codes [..., d, T], col_scales [..., d, ceil(T / 32)])`` --
    blocks of 32 along ``d`` and, transposed, along ``T`` -- for ``x [..., T, d]`` with at least 3 dimensions.  A pair whose format is
    ``None`` is not computed and comes back as ``(None, None)``; at least one format must be given.  Rounding is to nearest: forward
    activations round to nearest everywhere in the package.  The outputs are contiguous and never differentiable.

    The float32 rotation is never rounded to ``x.dtype`` and, on the GPU, never written: ONE launch (``qs_mx_rope_quant2_v``; no
    fallback) reads ``x`` where it lies (``mx_rope``'s rule), rotates in registers and writes the codes.  CPU tensors evaluate the
    composition above."""
    _check_rope("mx_rope_quantize", x, cos, sin)
    if x.dim() < 3:
        raise ValueError(f"mx_rope_quantize needs [..., T, d] with at least one leading dimension, got shape {tuple(x.shape)}")
    if row_fmt is None and col_fmt is None:
        raise ValueError("mx_rope_quantize needs row_fmt, col_fmt or both")
    for fmt in (row_fmt, col_fmt):
        if fmt is not None:
            _mx_format(fmt)
    interleaved, inverse = bool(interleaved), bool(inverse)
    x = x.detach()
    if not x.is_cuda:
        return mx_quantize_2way_batched(_rope_forward(x, cos, sin, interleaved, inverse, torch.float32), row_fmt, col_fmt)
    lead, (T, d) = tuple(x.shape[:-2]), x.shape[-2:]
    nb = lambda n: (n + MX_BLOCK - 1) // MX_BLOCK
    shapes = (lead + (T, d), lead + (T, nb(d)), lead + (d, T), lead + (d, nb(T)))
    xs, G0, G1, strides = _strided(x)
    out = _hip.mx_rope_quant2(xs, G0, G1, T, d, strides, cos, sin, interleaved, inverse, row_fmt, col_fmt)
    return tuple(None if t is None else t.view(shape) for t, shape in zip(out, shapes))


def _attention_rope(rope, T: int, S: int, d: int, device):
    """the `rope=` keyword of `mx_attention` / `mx_attention_train` as (cos_q, sin_q, cos_k, sin_k), checked; None for None"""
    if rope is None:
        return None
    if not isinstance(rope, (tuple, list)) or len(rope) not in (2, 4):
        raise TypeError("rope must be None, a 2-tuple (cos, sin) or a 4-tuple (cos_q, sin_q, cos_k, sin_k)")
    if d < 2 or d % 2:
        raise ValueError(f"rope needs an even d >= 2 (the last dimension of q and k), got {d}")
    if len(rope) == 2:
        if T != S:
            raise ValueError(f"a 2-tuple rope rotates q and k by the same tables and needs T == S, got T = {T}, S = {S}: give the "
                             "4-tuple (cos_q, sin_q, cos_k, sin_k)")
        rope = tuple(rope) * 2
    _check_tables(rope[0], rope[1], T, d, device, ("cos_q", "sin_q"))
    _check_tables(rope[2], rope[3], S, d, device, ("cos_k", "sin_k"))
    return tuple(rope)


__all__ = ["mx_rope_table", "mx_rope", "mx_rope_quantize"]
