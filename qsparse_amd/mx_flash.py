"""Attention on MX codes in one launch: ``mx_flash_attention``.

``mx_attention(softmax="fused")`` runs ``mx_bmm`` -> ``mx_softmax_quantize`` -> ``mx_bmm``: the float32 scores ``s [..., T, S]`` go to
memory and come back, and so do ``p``'s codes.  ``mx_flash_attention`` is that chain -- bit for bit, on either device -- from one HIP
kernel that keeps a row of scores in registers (``qs_mx_flash_attention_v``, ``csrc/qs_mx_flash.h``); the price is a bounded shape:
``S <= 512``, ``d <= 128``, ``dv <= 128``.  Outside it the call raises; there is no fallback.

``rows="streamed"`` is a second kernel (``qs_mx_flash_attention_streamed_v``, ``csrc/qs_mx_flash_stream.h``) for ANY ``S``: it walks the
keys in chunks of 128 with a running maximum, a running sum and a rescaled accumulator.  Its numerics are its own -- ``p`` is quantized
unnormalised, chunk by chunk -- and are DEFINED by ``_streamed_def`` below, a composition of ``mx_bmm``, ``quantize_with_mx`` and
elementary float32 torch ops that gives the kernel's bytes on either device.

The argument checks follow ``_mx_common.py``."""
from functools import partial
from typing import Optional

import torch
import torch.nn.functional as F

from qsparse_amd import _hip, _mx_common
from qsparse_amd._mx_common import _check_dtype
from qsparse_amd.mx_bmm import _attention_mask, mx_bmm
from qsparse_amd.mx_norm import _row_sum
from qsparse_amd.mx_softmax import _exp_def, mx_softmax_quantize
from qsparse_amd.quantize import _mx_format, quantize_with_mx

MX_FLASH_ROWS = ("resident", "streamed")
_CHUNK = 128                     # keys per chunk of the streamed definition: part of it, as 512 is part of `_row_sum`'s

_check_q = partial(_mx_common._check_operand, what="[..., T, d]", least=3, most=None, needs="at least 3 dimensions")
_check_k = partial(_mx_common._check_operand, what="[..., S, d]", least=3, most=None, needs="at least 3 dimensions")
_check_vt = partial(_mx_common._check_operand, what="[..., dv, S]", least=3, most=None, needs="at least 3 dimensions")


def _streamed_def(qc, qs, qk_fmt: str, kc, ks, vc, vs, v_fmt: str, mask, scale: float, causal: bool, p_fmt: str, out_dtype):
    """The streamed kernel's definition (``include/qsparse_hip.h``, "MX flash attention, streamed") on ``qc [G, T, d]``, ``kc [G, S, d]``,
    ``vc [G, dv, S]`` with their scales and an additive float32 ``mask`` ``[T, S]`` / ``[G, T, S]`` or None, on either device: per chunk
    of 128 keys one ``mx_bmm`` for the scores, float32 torch ops (one per operation) for the running maximum ``m``, ``e = E(u - m')``
    and its row sum, ``quantize_with_mx`` for ``e``'s codes, one ``mx_bmm`` against that slice of ``vt``, then ``Z = Z * alpha + z`` and
    ``acc = acc * alpha + o``; ``acc / Z`` at the end.  The CPU path of ``rows="streamed"``, and what tests compare the GPU against."""
    (G, T, _), S, dv, dev = qc.shape, kc.shape[1], vc.shape[1], qc.device
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    chunks = -(-S // _CHUNK)
    vcp = F.pad(vc, (0, chunks * _CHUNK - S))                   # codes past S are zero, scale blocks wholly past S are 127
    vsp = F.pad(vs, (0, 4 * chunks - vs.shape[-1]), value=127)
    m = torch.full((G, T, 1), float("-inf"), dtype=torch.float32, device=dev)
    Z = torch.zeros((G, T, 1), dtype=torch.float32, device=dev)
    acc = torch.zeros((G, T, dv), dtype=torch.float32, device=dev)
    bad = torch.zeros((G, T, 1), dtype=torch.bool, device=dev)
    rows = torch.arange(T, device=dev)[:, None]
    for c in range(chunks):
        lo, hi = c * _CHUNK, min(S, (c + 1) * _CHUNK)
        u = mx_bmm(qc, qs, qk_fmt, kc[:, lo:hi].contiguous(), ks[:, lo:hi].contiguous(), qk_fmt) * f(scale)
        if mask is not None:
            u = u + mask[..., lo:hi]
        if causal:                                              # column j of row t is admitted where j <= t
            u = torch.where(torch.arange(lo, hi, device=dev)[None, :] <= rows, u, f(float("-inf")))
        bad_c = (u.isnan() | (u == float("inf"))).any(-1, keepdim=True)
        m2 = torch.maximum(m, torch.where(u.isnan(), f(float("-inf")), u).amax(-1, keepdim=True))
        e, alpha = F.pad(_exp_def(u - m2), (0, _CHUNK - (hi - lo))), _exp_def(m - m2)
        z = _row_sum(e.reshape(G * T, _CHUNK)).reshape(G, T, 1)
        _, ec, es = quantize_with_mx(e, p_fmt, -1, return_codes=True)
        es = es.clone()
        es[..., -(-(hi - lo) // 32):] = 127                     # a block wholly past S: zero codes under the byte 127
        o = mx_bmm(ec, es, p_fmt, vcp[..., lo:lo + _CHUNK].contiguous(), vsp[..., 4 * c:4 * c + 4].contiguous(), v_fmt)
        live = (rows >= lo) if causal else torch.ones_like(rows, dtype=torch.bool)      # else the row's limit admits nothing here
        m, Z, acc, bad = (torch.where(live, new, old) for new, old in ((m2, m), (Z * alpha + z, Z), (acc * alpha + o, acc),
                                                                       (bad | bad_c, bad)))
    return torch.where(bad | (Z == 0), f(float("nan")), acc / Z).to(out_dtype)


def mx_flash_attention(q_codes: torch.Tensor, q_scales: torch.Tensor, qk_fmt: str, k_codes: torch.Tensor, k_scales: torch.Tensor,
                       vt_codes: torch.Tensor, vt_scales: torch.Tensor, v_fmt: str, mask: Optional[torch.Tensor] = None, *, scale: float,
                       is_causal: bool = False, p_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32,
                       rows: str = "resident") -> torch.Tensor:
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
    scores on chip, and there is no other kernel behind it.  Never differentiable.

    ``rows`` (keyword; ``"resident"``, the default, is everything above, refusals included) ``= "streamed"`` takes ANY ``S >= 1`` with
    the same operands, masks, formats and dtypes: GPU tensors take ONE launch of the streamed kernel, whose registers and LDS do not
    depend on ``S``; CPU tensors evaluate ``_streamed_def``.  The result is NOT the composition above but the chunk recurrence
    ``_streamed_def`` spells (chunks of 128 keys, ``e = E(u - m')`` quantized unnormalised, one division by ``Z`` at the end), bit for bit
    on either device.  A row with a NaN or ``+inf`` in ``u``, or that admits nothing, is NaN as a whole; under ``is_causal`` a chunk
    behind a row's limit is not applied to that row, so a NaN in ``vt`` there leaves it finite."""
    if rows not in MX_FLASH_ROWS:
        raise ValueError(f"unknown rows {rows!r}: one of {MX_FLASH_ROWS}")
    streamed = rows == "streamed"
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
        if streamed and name == "S":
            if n < 1:
                raise ValueError(f"mx_flash_attention takes S >= 1, got S = {n}")
        elif n > most or (n < 1 and name != "dv"):
            raise ValueError(f"mx_flash_attention takes 1 <= {name} <= {most}, got {name} = {n}: a whole row of scores stays on chip; "
                             'longer rows take mx_attention(..., impl="composed")')
    for name, t in (("k_codes", k_codes), ("vt_codes", vt_codes)):
        if t.device != q_codes.device:
            raise ValueError(f"q_codes is on {q_codes.device} but {name} on {t.device}")
    if 0 in (T, dv) or 0 in lead:
        return q_codes.new_empty(lead + (T, dv), dtype=out_dtype)
    if not q_codes.is_cuda and not streamed:
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
        if not q_codes.is_cuda:
            return _streamed_def(*ops, mask, float(scale), bool(is_causal), p_fmt, out_dtype).reshape(lead + (T, dv))
        return _hip.mx_flash_attention(*ops, mask, float(scale), bool(is_causal), p_fmt, out_dtype,
                                       streamed=streamed).reshape(lead + (T, dv))


__all__ = ["mx_flash_attention"]
