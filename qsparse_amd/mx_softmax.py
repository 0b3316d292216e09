"""Scale, mask and softmax in front of the MX quantizer: ``mx_softmax_quantize``.

Between the two products of attention lie ``* scale``, ``+ mask``, ``softmax`` and the quantizer of ``p`` -- four passes over a float32
``[..., T, S]``.  ``mx_softmax_quantize`` hands ``p`` out as the MX codes the ``P . V`` product multiplies, without any of the tensors in
between: on the GPU ``qs_mx_softmax_quant_v`` (one launch, no fallback), on the CPU the definition below in torch float32 ops.  The
definition (``include/qsparse_hip.h``, "MX softmax quantizer") is NOT "what ``torch.softmax`` gives": it writes its exponential out
(Cody-Waite reduction, a degree-7 polynomial, an exact scaling), rounds every float32 operation on its own and takes the row sum in
``mx_norm``'s fixed order, so both paths give the same bytes.

The argument checks follow ``_mx_common.py``."""
from typing import Optional

import torch

from qsparse_amd import _hip
from qsparse_amd._mx_common import _check_dtype
from qsparse_amd.mx_bmm import _attention_mask
from qsparse_amd.mx_norm import _row_sum
from qsparse_amd.quantize import _mx_check_rounding, _mx_format, quantize_with_mx

_LOG2E, _LN2_HI, _LN2_LO, _T_MIN = 1.44269504, 0.693359375, -2.12194440e-4, -87.0
_COEF = (1 / 5040, 1 / 720, 1 / 120, 1 / 24, 1 / 6, 1 / 2, 1.0, 1.0)        # Horner, highest degree first; each rounded to float32


def _exp_def(t: torch.Tensor) -> torch.Tensor:
    """``E(t)`` of the definition on a float32 tensor ``t <= 0`` (``-inf`` gives +0; a NaN gives +0: its row is NaN as a whole and
    never reads it): one torch op per float32 operation"""
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=t.device)
    live = t >= f(_T_MIN)
    tc = torch.where(live, t, f(_T_MIN))
    n = torch.round(tc * f(_LOG2E))                              # ties to even
    r = (tc - n * f(_LN2_HI)) - n * f(_LN2_LO)
    P = f(_COEF[0]).expand_as(r)
    for c in _COEF[1:]:
        P = P * r + f(c)
    return torch.where(live, torch.ldexp(P, n.to(torch.int32)), f(0.0))


def _softmax_u(s3: torch.Tensor, mask: Optional[torch.Tensor], scale: float, causal: bool) -> torch.Tensor:
    """``u [G, T, S]`` of the definition: ``s * scale (+ mask)``, ``-inf`` where the causal limit excludes the column"""
    G, T, S = s3.shape
    u = s3.to(torch.float32) * torch.tensor(scale, dtype=torch.float32, device=s3.device)
    if mask is not None:
        u = u + mask
    if causal:                                                  # column j of row t is admitted where j < L = t + 1: top-left aligned
        admitted = torch.arange(S, device=s3.device)[None, :] <= torch.arange(T, device=s3.device)[:, None]
        u = torch.where(admitted, u, torch.full_like(u, float("-inf")))
    return u


def _stats_def(s3: torch.Tensor, mask: Optional[torch.Tensor], scale: float, causal: bool):
    """``(p, m, Z)`` of the definition on ``s3 [G, T, S]``: the float32 ``p`` the quantizer is defined on and the row maximum and row
    sum it divides by, float32 ``[G, T]``, both the quiet NaN for a row that is NaN as a whole"""
    G, T, S = s3.shape
    u = _softmax_u(s3, mask, scale, causal)
    m = u.amax(-1, keepdim=True)                                # (a NaN propagates)
    e = _exp_def(u - m)
    Z = _row_sum(e.reshape(G * T, S)).reshape(G, T, 1)
    # a NaN in the row, m = +inf, m = -inf (nothing admitted): the row is NaN as a whole
    ok = torch.isfinite(m)
    nan = torch.full_like(m, float("nan"))
    # (m + 0: a zero maximum of either sign is handed out as +0 -- which zero a maximum of mixed zeros is, no two devices agree on)
    return torch.where(ok, e / Z, torch.full_like(e, float("nan"))), torch.where(ok, m + 0.0, nan).reshape(G, T), \
        torch.where(ok, Z, nan).reshape(G, T)


def _mx_softmax_p(s3: torch.Tensor, mask: Optional[torch.Tensor], scale: float, causal: bool) -> torch.Tensor:
    """the definition in torch float32 ops on ``s3 [G, T, S]`` (``mask`` float32 ``[T, S]`` or ``[G, T, S]`` or None): the float32
    ``p [G, T, S]`` the quantizer is defined on -- the CPU path of ``mx_softmax_quantize``, and what tests compare the GPU against"""
    return _stats_def(s3, mask, scale, causal)[0]


def _softmax_operands(fn: str, s, mask, scale, is_causal, others=()):
    """the checks ``mx_softmax_quantize`` and ``mx_softmax_backward_quantize`` share; returns ``(lead, G, T, S, s3, mask)`` with the
    additive float32 mask ``[T, S]`` or ``[G, T, S]`` (contiguous) or None.  `others`: (name, tensor) pairs refused like ``s`` where they
    require grad"""
    if not isinstance(s, torch.Tensor):
        raise TypeError(f"s must be a tensor, got {type(s).__name__}")
    _check_dtype("s", s.dtype)
    if s.dim() < 2:
        raise ValueError(f"{fn} needs s [..., T, S] with at least 2 dimensions, got shape {tuple(s.shape)}")
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError(f"scale must be a float, got {type(scale).__name__}")
    if mask is not None and is_causal:
        raise ValueError("give mask or is_causal, not both")
    for name, t in (("s", s), ("mask", mask)) + tuple(others):
        if isinstance(t, torch.Tensor) and torch.is_grad_enabled() and t.requires_grad:
            raise RuntimeError(f"{fn} is not differentiable: {name} requires grad; call it under torch.no_grad()")
    lead, (T, S) = tuple(s.shape[:-2]), s.shape[-2:]
    G = 1
    for n in lead:
        G *= n
    with torch.no_grad():
        mask = _attention_mask(mask, False, T, S, s.device)     # additive float32 [..., T, S], or None
        if mask is not None:
            if all(n == 1 for n in mask.shape[:-2]):
                mask = mask.reshape(T, S)                       # one [T, S] for every slice
            else:
                try:
                    mask = torch.broadcast_to(mask, lead + (T, S)).reshape(G, T, S)
                except RuntimeError:
                    raise ValueError(f"mask has shape {tuple(mask.shape)}, which does not broadcast over the leading dimensions of s "
                                     f"{tuple(s.shape)}") from None
            mask = mask.contiguous()
        return lead, G, T, S, s.detach().reshape(G, T, S), mask


def mx_softmax_quantize(s: torch.Tensor, mask: Optional[torch.Tensor] = None, *, scale: float = 1.0, is_causal: bool = False,
                        fmt: str = "mxfp8_e4m3", col_fmt: Optional[str] = None, return_stats: bool = False):
    """MX codes of ``p = softmax(s * scale + mask, -1)`` for scores ``s [..., T, S]`` (float32 / bfloat16 / float16, at least 2
    dimensions), none of the tensors in between written.  ``mask`` is boolean (False adds ``-inf``) or floating (added), ``[..., T, S]``
    broadcast over the leading dimensions of ``s``; ``is_causal`` admits column ``j`` of row ``t`` where ``j <= t`` (the lower triangle
    aligned top-left, as ``F.scaled_dot_product_attention`` takes it; ``T != S`` is allowed) without a mask tensor.  Giving both raises.
    Returns

        (codes uint8 [..., T, S], scales uint8 [..., T, ceil(S / 32)])

    the codes and scales of ``quantize_with_mx(p, fmt, -1, return_codes=True)`` for the ``p`` of this definition, all float32, every
    operation rounded on its own:

        u_j = s_j * scale (+ a_j)          -inf where the causal limit excludes j
        m = max_j u_j,  e_j = E(u_j - m),  Z = sum_j e_j in ``mx_norm_quantize``'s row-sum order,  p_j = e_j / Z
        E(t):  n = rint(t * 1.44269504),  r = (t - n * 0.693359375) - n * -2.12194440e-4,
               P = Horner of degree 7 in r with the coefficients 1 / k!,  E = P * 2^n;  E = 0 for t < -87

    ``E`` lies within one float32 ulp of ``exp``; the codes usually equal those of ``torch.softmax``'s ``p`` but are not defined by it.
    A row that holds a NaN or ``+inf``, or admits no column, is NaN as a whole (scale byte 0xFF in each of its blocks); ``-inf`` beside
    finite values is a plain zero.  The result is never differentiable, and an operand that requires grad while gradients are enabled is
    refused, as ``mx_attention`` refuses it.  GPU tensors take the HIP kernel (one launch, no fallback), CPU tensors the torch
    expression of the definition: the same bytes.

    The training side (keywords; without them the call, its launch and its bytes are as above).  ``col_fmt=f`` appends ``(col_codes
    uint8 [..., S, T], col_scales uint8 [..., S, ceil(T / 32)])``, per slice the bytes of ``quantize_with_mx(p.transpose(-1, -2), f, -1,
    return_codes=True)``: the operand of ``dV = P^T dO``; a row that is NaN as a whole puts 0xFF into every column block it touches.
    ``return_stats=True`` appends ``(m, Z)``, float32 ``[..., T]``: the row maximum (a zero maximum is ``+0``) and the row sum above, both the quiet NaN
    for a row that is NaN as a whole -- what ``mx_softmax_backward_quantize`` forms ``p`` from again.  The order is ``(codes, scales[, col_codes,
    col_scales][, m, Z])`` and the row pair is the same bytes for every combination.  With either keyword GPU tensors take
    ``qs_mx_softmax_quant2_v``: a statistics launch, then the two-way quantizer's tile with ``p`` as its widen step."""
    lead, G, T, S, s3, mask = _softmax_operands("mx_softmax_quantize", s, mask, scale, is_causal)
    _mx_format(fmt)
    if col_fmt is not None:
        _mx_format(col_fmt)
    nb = lambda n: (n + 31) // 32
    two_way = col_fmt is not None or bool(return_stats)
    cc = cs = m = Z = None
    with torch.no_grad():
        if s.is_cuda and not two_way:
            codes, scales = _hip.mx_softmax_quant(s3.contiguous(), mask, float(scale), is_causal, fmt)
        elif s.is_cuda:
            codes, scales, cc, cs, m, Z = _hip.mx_softmax_quant2(s3.contiguous(), mask, float(scale), is_causal, fmt, col_fmt)
        elif s3.numel() == 0:                                   # (the CPU quantizer takes no empty tensor)
            new = lambda *shape: s.new_empty(shape, dtype=torch.uint8)
            codes, scales, cc, cs = new(G, T, S), new(G, T, nb(S)), new(G, S, T), new(G, S, nb(T))
            m, Z = s.new_empty((G, T), dtype=torch.float32), s.new_empty((G, T), dtype=torch.float32)
        else:
            p, m, Z = _stats_def(s3, mask, float(scale), bool(is_causal))
            _, codes, scales = quantize_with_mx(p, fmt, -1, return_codes=True)
            if col_fmt is not None:
                _, cc, cs = quantize_with_mx(p.transpose(-1, -2), col_fmt, -1, return_codes=True)
                cc, cs = cc.contiguous(), cs.contiguous()
    out = (codes.reshape(lead + (T, S)), scales.reshape(lead + (T, nb(S))))
    if col_fmt is not None:
        out += (cc.reshape(lead + (S, T)), cs.reshape(lead + (S, nb(T))))
    if return_stats:
        out += (m.reshape(lead + (T,)), Z.reshape(lead + (T,)))
    return out


def _softmax_ds(dp3: torch.Tensor, s3: torch.Tensor, m: torch.Tensor, Z: torch.Tensor, mask: Optional[torch.Tensor], scale: float,
                causal: bool) -> torch.Tensor:
    """``ds [G, T, S]`` float32 of ``mx_softmax_backward_quantize``'s definition in torch float32 ops, one per operation"""
    G, T, S = s3.shape
    u = _softmax_u(s3, mask, scale, causal)
    m, Z = m.reshape(G, T, 1), Z.reshape(G, T, 1)
    p = torch.where(m != m, torch.full_like(u, float("nan")), _exp_def(u - m) / Z)
    dp32 = dp3.to(torch.float32)
    D = _row_sum((p * dp32).reshape(G * T, S)).reshape(G, T, 1)
    return (p * (dp32 - D)) * torch.tensor(scale, dtype=torch.float32, device=s3.device)


def mx_softmax_backward_quantize(dp: torch.Tensor, s: torch.Tensor, m: torch.Tensor, Z: torch.Tensor,
                                 mask: Optional[torch.Tensor] = None, *, scale: float = 1.0, is_causal: bool = False,
                                 row_fmt: Optional[str], col_fmt: Optional[str], rounding: str = "nearest", seed: int = 0,
                                 step: Optional[torch.Tensor] = None):
    """The softmax backward behind ``mx_softmax_quantize``, as MX codes both ways: from ``dp [..., T, S]`` (the gradient with respect
    to ``p``; float32 / bfloat16 / float16), the forward's ``s``, ``mask``, ``scale`` and ``is_causal`` and its ``return_stats`` pair
    ``m``, ``Z`` (float32 ``[..., T]``), returns

        (row_codes [..., T, S], row_scales [..., T, ceil(S / 32)], col_codes [..., S, T], col_scales [..., S, ceil(T / 32)])

    of the gradient ``ds`` with respect to ``s``; a pair whose format is ``None`` is ``(None, None)``, giving ``None`` for both raises.
    The definition is all float32, every operation rounded on its own, with no contraction:

        u_j  as in the forward;   p_j = E(u_j - m) / Z          (the forward's p, to the bit)
        D    = sum_j (p_j * dp_j)   in ``mx_norm_quantize``'s fixed row-sum order (a function of S alone)
        ds_j = (p_j * (dp_j - D)) * scale
        a row whose m is NaN is NaN as a whole

    and the result is bit for bit ``mx_quantize_2way_batched(ds, row_fmt, col_fmt, rounding, seed, step)`` on that float32 ``ds`` --
    the same Philox words, the same streams for the two pairs, ``step`` read on the device.  A NaN or an Inf in ``dp`` makes its row NaN.
    Neither ``p`` nor ``ds`` is ever written to memory: GPU tensors take ``qs_mx_softmax_bwd_quant_v`` (a row launch for ``D``, then the
    two-way quantizer's tile with the ``ds`` expression as its widen step; no atomics, no host synchronisation, no fallback), CPU
    tensors the definition in torch ops.  Never differentiable: an operand that requires grad while gradients are enabled is refused."""
    if not isinstance(dp, torch.Tensor):
        raise TypeError(f"dp must be a tensor, got {type(dp).__name__}")
    _check_dtype("dp", dp.dtype)
    lead, G, T, S, s3, mask = _softmax_operands("mx_softmax_backward_quantize", s, mask, scale, is_causal,
                                                (("dp", dp), ("m", m), ("Z", Z)))
    if tuple(dp.shape) != tuple(s.shape):
        raise ValueError(f"dp has shape {tuple(dp.shape)}, expected that of s {tuple(s.shape)}")
    for name, t in (("m", m), ("Z", Z)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32 (what mx_softmax_quantize(..., return_stats=True) returns), got {t.dtype}")
        if tuple(t.shape) != lead + (T,):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {lead + (T,)}")
    for name, t in (("dp", dp), ("m", m), ("Z", Z)):
        if t.device != s.device:
            raise ValueError(f"s is on {s.device} but {name} on {t.device}")
    if row_fmt is None and col_fmt is None:
        raise ValueError("mx_softmax_backward_quantize needs row_fmt, col_fmt or both")
    for f in (row_fmt, col_fmt):
        if f is not None:
            _mx_format(f)
    _mx_check_rounding(rounding, step, s)
    nb = lambda n: (n + 31) // 32
    shapes = (lead + (T, S), lead + (T, nb(S)), lead + (S, T), lead + (S, nb(T)))
    with torch.no_grad():
        dp3, m2, Z2 = dp.detach().reshape(G, T, S), m.detach().reshape(G, T), Z.detach().reshape(G, T)
        if s.is_cuda:
            out = _hip.mx_softmax_bwd_quant(dp3.contiguous(), s3.contiguous(), m2.contiguous(), Z2.contiguous(), mask, float(scale),
                                            bool(is_causal), row_fmt, col_fmt, rounding, seed, step)
        elif s3.numel() == 0:                                   # (the CPU quantizer takes no empty tensor)
            out = tuple(None if f is None else s.new_empty(shape, dtype=torch.uint8)
                        for shape, f in zip(shapes, (row_fmt, row_fmt, col_fmt, col_fmt)))
        else:
            from qsparse_amd.mx_batched_train import mx_quantize_2way_batched     # (it imports mx_bmm, as this module does)
            out = mx_quantize_2way_batched(_softmax_ds(dp3, s3, m2, Z2, mask, float(scale), bool(is_causal)), row_fmt, col_fmt,
                                           rounding, seed, step)
    return tuple(None if t is None else t.reshape(shape) for t, shape in zip(out, shapes))


__all__ = ["mx_softmax_quantize", "mx_softmax_backward_quantize"]
