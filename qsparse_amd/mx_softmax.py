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
from qsparse_amd.quantize import _mx_format, quantize_with_mx

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


def _mx_softmax_p(s3: torch.Tensor, mask: Optional[torch.Tensor], scale: float, causal: bool) -> torch.Tensor:
    """the definition in torch float32 ops on ``s3 [G, T, S]`` (``mask`` float32 ``[T, S]`` or ``[G, T, S]`` or None): the float32
    ``p [G, T, S]`` the quantizer is defined on -- the CPU path of ``mx_softmax_quantize``, and what tests compare the GPU against"""
    G, T, S = s3.shape
    u = s3.to(torch.float32) * torch.tensor(scale, dtype=torch.float32, device=s3.device)
    if mask is not None:
        u = u + mask
    if causal:                                                  # column j of row t is admitted where j < L = t + 1: top-left aligned
        admitted = torch.arange(S, device=s3.device)[None, :] <= torch.arange(T, device=s3.device)[:, None]
        u = torch.where(admitted, u, torch.full_like(u, float("-inf")))
    m = u.amax(-1, keepdim=True)                                # (a NaN propagates)
    e = _exp_def(u - m)
    Z = _row_sum(e.reshape(G * T, S)).reshape(G, T, 1)
    # a NaN in the row, m = +inf, m = -inf (nothing admitted): the row is NaN as a whole
    return torch.where(torch.isfinite(m), e / Z, torch.full_like(e, float("nan")))


def mx_softmax_quantize(s: torch.Tensor, mask: Optional[torch.Tensor] = None, *, scale: float = 1.0, is_causal: bool = False,
                        fmt: str = "mxfp8_e4m3"):
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
    expression of the definition: the same bytes."""
    if not isinstance(s, torch.Tensor):
        raise TypeError(f"s must be a tensor, got {type(s).__name__}")
    _check_dtype("s", s.dtype)
    if s.dim() < 2:
        raise ValueError(f"mx_softmax_quantize needs s [..., T, S] with at least 2 dimensions, got shape {tuple(s.shape)}")
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError(f"scale must be a float, got {type(scale).__name__}")
    if mask is not None and is_causal:
        raise ValueError("give mask or is_causal, not both")
    for name, t in (("s", s), ("mask", mask)):
        if isinstance(t, torch.Tensor) and torch.is_grad_enabled() and t.requires_grad:
            raise RuntimeError(f"mx_softmax_quantize is not differentiable: {name} requires grad; call it under torch.no_grad()")
    _mx_format(fmt)
    lead, (T, S) = tuple(s.shape[:-2]), s.shape[-2:]
    G = 1
    for n in lead:
        G *= n
    nb = (S + 31) // 32
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
        s3 = s.detach().reshape(G, T, S)
        if s.is_cuda:
            codes, scales = _hip.mx_softmax_quant(s3.contiguous(), mask, float(scale), is_causal, fmt)
        elif s3.numel() == 0:                                   # (the CPU quantizer takes no empty tensor)
            codes, scales = s.new_empty((G, T, S), dtype=torch.uint8), s.new_empty((G, T, nb), dtype=torch.uint8)
        else:
            _, codes, scales = quantize_with_mx(_mx_softmax_p(s3, mask, float(scale), bool(is_causal)), fmt, -1, return_codes=True)
    return codes.reshape(lead + (T, S)), scales.reshape(lead + (T, nb))


__all__ = ["mx_softmax_quantize"]
