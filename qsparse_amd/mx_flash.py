"""Attention on MX codes in one launch: ``mx_flash_attention``.

``mx_attention(softmax="fused")`` runs ``mx_bmm`` -> ``mx_softmax_quantize`` -> ``mx_bmm``: the float32 scores ``s [..., T, S]`` go to
memory and come back, and so do ``p``'s codes.  ``mx_flash_attention`` is that chain -- bit for bit, on either device -- from one HIP
kernel that keeps a row of scores in registers (``qs_mx_flash_attention_v``, ``csrc/qs_mx_flash.h``); the price is a bounded shape:
``S <= 512``, ``d <= 128``, ``dv <= 128``.  Outside it the call raises; there is no fallback.

The argument checks follow ``_mx_common.py``."""
from functools import partial
from typing import Optional

import torch

from qsparse_amd import _hip, _mx_common
from qsparse_amd._mx_common import _check_dtype
from qsparse_amd.mx_bmm import _attention_mask, mx_bmm
from qsparse_amd.mx_softmax import mx_softmax_quantize
from qsparse_amd.quantize import _mx_format

_check_q = partial(_mx_common._check_operand, what="[..., T, d]", least=3, most=None, needs="at least 3 dimensions")
_check_k = partial(_mx_common._check_operand, what="[..., S, d]", least=3, most=None, needs="at least 3 dimensions")
_check_vt = partial(_mx_common._check_operand, what="[..., dv, S]", least=3, most=None, needs="at least 3 dimensions")


def mx_flash_attention(q_codes: torch.Tensor, q_scales: torch.Tensor, qk_fmt: str, k_codes: torch.Tensor, k_scales: torch.Tensor,
                       vt_codes: torch.Tensor, vt_scales: torch.Tensor, v_fmt: str, mask: Optional[torch.Tensor] = None, *, scale: float,
                       is_causal: bool = False, p_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Scaled dot-product attention on MX codes.  ``q_codes [..., T, d]`` and ``k_codes [..., S, d]`` are uint8 codes of ``qk_fmt`` with
    blocks along ``d``, ``vt_codes [..., dv, S]`` those of ``v_fmt`` with blocks along ``S`` (``v`` transposed: what ``mx_attention``'s
    step 7 produces), the scales as ``mx_bmm`` takes them, the leading dimensions equal.  It is DEFINED as this composition and returns,
    bit for bit on either device, the same bytes:

        s       = mx_bmm(q_codes, q_scales, qk_fmt, k_codes, k_scales, qk_fmt)                       # float32 [..., T, S]
        pc, psc = mx_softmax_quantize(s, mask, scale=scale, is_causal=is_causal, fmt=p_fmt)
        out     = mx_bmm(pc, psc, p_fmt, vt_codes, vt_scales, v_fmt, None, out_dtype)                # [..., T, dv]

    so ``mask`` (boolean or floating, ``[..., T, S]`` broadcast over the leading dimensions), ``is_causal`` (top-left aligned, ``T != S``
    allowed; not together with ``mask``), ``scale`` (any float) and the exceptional rows -- a NaN in ``u``, ``m = +-inf`` or nothing
    admitted make the whole row NaN -- are ``mx_softmax_quantize``'s.  GPU tensors take ONE launch in which neither ``s``, nor ``p``, nor
    ``p``'s codes exist in memory; CPU tensors evaluate the composition itself.

    Supported range: ``1 <= S <= 512``, ``1 <= d <= 128``, ``1 <= dv <= 128``, any ``T`` and leading dimensions, every format triple,
    ``out_dtype`` float32 / bfloat16 / float16.  Anything else raises ``ValueError`` naming the bound: the kernel keeps a whole row of
    scores on chip, and there is no other kernel behind it.  Never differentiable."""
    _check_q("q", q_codes, q_scales, qk_fmt)
    _check_k("k", k_codes, k_scales, qk_fmt)
    _check_vt("vt", vt_codes, vt_scales, v_fmt)
    _mx_format(p_fmt)
    _check_dtype("out_dtype", out_dtype)
    lead, (T, d), S, dv = tuple(q_codes.shape[:-2]), q_codes.shape[-2:], k_codes.shape[-2], vt_codes.shape[-2]
    if tuple(k_codes.shape[:-2]) != lead or tuple(vt_codes.shape[:-2]) != lead:
        raise ValueError(f"q_codes {tuple(q_codes.shape)}, k_codes {tuple(k_codes.shape)} and vt_codes {tuple(vt_codes.shape)} disagree on "
                         "their leading dimensions (nothing is broadcast)")
    if k_codes.shape[-1] != d:
        raise ValueError(f"q_codes {tuple(q_codes.shape)} and k_codes {tuple(k_codes.shape)} disagree on d (their last dimensions)")
    if vt_codes.shape[-1] != S:
        raise ValueError(f"k_codes {tuple(k_codes.shape)} [..., S, d] and vt_codes {tuple(vt_codes.shape)} [..., dv, S] disagree on S")
    for name, n, most in (("S", S, _hip.MX_FLASH_MAX_S), ("d", d, _hip.MX_FLASH_MAX_D), ("dv", dv, _hip.MX_FLASH_MAX_D)):
        if n > most or (n < 1 and name != "dv"):
            raise ValueError(f"mx_flash_attention takes 1 <= {name} <= {most}, got {name} = {n}: a whole row of scores stays on chip; "
                             'longer rows take mx_attention(..., impl="composed")')
    for name, t in (("k_codes", k_codes), ("vt_codes", vt_codes)):
        if t.device != q_codes.device:
            raise ValueError(f"q_codes is on {q_codes.device} but {name} on {t.device}")
    if 0 in (T, dv) or 0 in lead:
        return q_codes.new_empty(lead + (T, dv), dtype=out_dtype)
    if not q_codes.is_cuda:
        s = mx_bmm(q_codes, q_scales, qk_fmt, k_codes, k_scales, qk_fmt)
        pc, psc = mx_softmax_quantize(s, mask, scale=scale, is_causal=is_causal, fmt=p_fmt)
        return mx_bmm(pc, psc, p_fmt, vt_codes, vt_scales, v_fmt, None, out_dtype)
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError(f"scale must be a float, got {type(scale).__name__}")
    if mask is not None and is_causal:
        raise ValueError("give mask or is_causal, not both")
    G = 1
    for n in lead:
        G *= n
    with torch.no_grad():
        mask = _attention_mask(mask, False, T, S, q_codes.device)      # additive float32 [..., T, S], or None: as mx_softmax_quantize
        if mask is not None:
            if all(n == 1 for n in mask.shape[:-2]):
                mask = mask.reshape(T, S)
            else:
                try:
                    mask = torch.broadcast_to(mask, lead + (T, S)).reshape(G, T, S)
                except RuntimeError:
                    raise ValueError(f"mask has shape {tuple(mask.shape)}, which does not broadcast over the leading dimensions "
                                     f"{lead}") from None
            mask = mask.contiguous()
        ops = (q_codes.reshape(G, T, d).contiguous(), q_scales.reshape(G, T, -1).contiguous(), qk_fmt,
               k_codes.reshape(G, S, d).contiguous(), k_scales.reshape(G, S, -1).contiguous(),
               vt_codes.reshape(G, dv, S).contiguous(), vt_scales.reshape(G, dv, -1).contiguous(), v_fmt)
        return _hip.mx_flash_attention(*ops, mask, float(scale), bool(is_causal), p_fmt, out_dtype).reshape(lead + (T, dv))


__all__ = ["mx_flash_attention"]
