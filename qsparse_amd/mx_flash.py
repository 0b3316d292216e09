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


def _empty_state(G: int, T: int, dv: int, dev):
    """the chunk recurrence's state before any chunk: ``(m, Z, acc, bad)`` = (-inf, 0, 0, False) per row"""
    return (torch.full((G, T, 1), float("-inf"), dtype=torch.float32, device=dev), torch.zeros((G, T, 1), dtype=torch.float32, device=dev),
            torch.zeros((G, T, dv), dtype=torch.float32, device=dev), torch.zeros((G, T, 1), dtype=torch.bool, device=dev))


def _chunk_step(state, c: int, qc, qs, qk_fmt: str, kc, ks, vc, vs, v_fmt: str, mask, scale: float, lim, p_fmt: str):
    """One step of the chunk recurrence, shared by ``_streamed_def`` and ``_decode_def``: chunk ``c`` -- the keys ``[128 c, min(S, 128 c +
    128))`` of ``kc [G, S, d]`` / ``vc [G, dv, S]`` -- applied to ``state = (m, Z, acc, bad)``.  ``lim`` is None or an integer tensor
    ``[T, 1]``: row t admits the columns ``j < lim[t]``, and a chunk that starts at or behind ``lim[t]`` leaves the row's state as it was."""
    m, Z, acc, bad = state
    (G, T, _), S, dev = qc.shape, kc.shape[1], qc.device
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    lo, hi = c * _CHUNK, min(S, (c + 1) * _CHUNK)
    u = mx_bmm(qc, qs, qk_fmt, kc[:, lo:hi].contiguous(), ks[:, lo:hi].contiguous(), qk_fmt) * f(scale)
    if mask is not None:
        u = u + mask[..., lo:hi]
    if lim is not None:
        u = torch.where(torch.arange(lo, hi, device=dev)[None, :] < lim, u, f(float("-inf")))
    bad_c = (u.isnan() | (u == float("inf"))).any(-1, keepdim=True)
    m2 = torch.maximum(m, torch.where(u.isnan(), f(float("-inf")), u).amax(-1, keepdim=True))
    e, alpha = F.pad(_exp_def(u - m2), (0, _CHUNK - (hi - lo))), _exp_def(m - m2)
    z = _row_sum(e.reshape(G * T, _CHUNK)).reshape(G, T, 1)
    _, ec, es = quantize_with_mx(e, p_fmt, -1, return_codes=True)
    es = es.clone()
    es[..., -(-(hi - lo) // 32):] = 127                         # a block wholly past S: zero codes under the byte 127
    vcc = F.pad(vc[..., lo:hi], (0, _CHUNK - (hi - lo)))        # codes past S are zero, scale blocks wholly past S are 127
    vsc = F.pad(vs[..., 4 * c:4 * c + 4], (0, 4 - vs[..., 4 * c:4 * c + 4].shape[-1]), value=127)
    o = mx_bmm(ec, es, p_fmt, vcc.contiguous(), vsc.contiguous(), v_fmt)
    live = (lim > lo) if lim is not None else torch.ones((T, 1), dtype=torch.bool, device=dev)
    return tuple(torch.where(live, new, old) for new, old in ((m2, m), (Z * alpha + z, Z), (acc * alpha + o, acc), (bad | bad_c, bad)))


def _streamed_def(qc, qs, qk_fmt: str, kc, ks, vc, vs, v_fmt: str, mask, scale: float, causal: bool, p_fmt: str, out_dtype):
    """The streamed kernel's definition (``include/qsparse_hip.h``, "MX flash attention, streamed") on ``qc [G, T, d]``, ``kc [G, S, d]``,
    ``vc [G, dv, S]`` with their scales and an additive float32 ``mask`` ``[T, S]`` / ``[G, T, S]`` or None, on either device: per chunk
    of 128 keys one ``mx_bmm`` for the scores, float32 torch ops (one per operation) for the running maximum ``m``, ``e = E(u - m')``
    and its row sum, ``quantize_with_mx`` for ``e``'s codes, one ``mx_bmm`` against that slice of ``vt``, then ``Z = Z * alpha + z`` and
    ``acc = acc * alpha + o``; ``acc / Z`` at the end.  The CPU path of ``rows="streamed"``, and what tests compare the GPU against."""
    (G, T, _), S, dv, dev = qc.shape, kc.shape[1], vc.shape[1], qc.device
    rows = torch.arange(T, device=dev)[:, None]
    state = _empty_state(G, T, dv, dev)
    for c in range(-(-S // _CHUNK)):                            # column j of row t is admitted where j <= t
        state = _chunk_step(state, c, qc, qs, qk_fmt, kc, ks, vc, vs, v_fmt, mask, scale, rows + 1 if causal else None, p_fmt)
    return _finish(*state, out_dtype)


def _finish(m, Z, acc, bad, out_dtype):
    """``acc / Z``; a row that is bad, or that admitted nothing, is NaN as a whole"""
    return torch.where(bad | (Z == 0), torch.tensor(float("nan"), dtype=torch.float32, device=Z.device), acc / Z).to(out_dtype)


def _decode_splits(waves_at_one_split: int, chunks: int) -> int:
    """``kv_splits="auto"``: enough splits of the key axis to put about one wave on each of the 1024 SIMDs (256 CUs x 4) of an MI355X,
    never more than the ``chunks`` of 128 keys there are.  A pure function of the shapes -- no device is asked -- because the split
    count is part of the numerics."""
    return min(max(1, chunks), max(1, 1024 // max(1, waves_at_one_split)))


def _decode_def(qc, qs, qk_fmt: str, kc, ks, vc, vs, v_fmt: str, kv_len, scale: float, causal: bool, p_fmt: str, out_dtype, splits: int):
    """The decode kernel's definition (``include/qsparse_hip.h``, "MX flash attention, decode") on ``qc [B, Hq, T, d]``, ``kc [B, Hkv, S,
    d]``, ``vc [B, Hkv, dv, S]`` with their scales and ``kv_len`` (None or int32 ``[B]``), on either device.  Per sequence the operands
    are sliced to ``L_b`` keys; split i owns the chunks ``[i cps, (i + 1) cps)``, ``cps = ceil(ceil(S / 128) / splits)``, and walks them
    with ``_chunk_step`` from the empty state; the splits are combined in ascending order, none skipped.  It reads ``kv_len`` on the
    host: it is what the tests compare against, not what a graph captures."""
    (B, Hq, T, d), (_, Hkv, S, _), dv, dev = qc.shape, kc.shape, vc.shape[2], qc.device
    r = Hq // Hkv
    cps = -(-(-(-S // _CHUNK)) // splits)
    lens = [S] * B if kv_len is None else [min(max(int(n), 0), S) for n in kv_len.tolist()]
    tok = (torch.arange(r * T, device=dev) % T)[:, None]         # packed row rho is query head hk r + rho // T, token rho % T
    out = []
    for b, L in enumerate(lens):
        q = (qc[b].reshape(Hkv, r * T, d), qs[b].reshape(Hkv, r * T, -1))
        kv = (kc[b, :, :L], ks[b, :, :L], vc[b, :, :, :L], vs[b, :, :, :-(-L // 32)])
        lim = (tok + (L - T + 1)).clamp(min=0) if causal else None      # bottom-right: token t admits the keys j <= L - T + t
        states = []
        for i in range(splits):
            state = _empty_state(Hkv, r * T, dv, dev)
            for c in range(i * cps, min((i + 1) * cps, -(-L // _CHUNK))):
                state = _chunk_step(state, c, *q, qk_fmt, *kv[:2], *kv[2:], v_fmt, None, scale, lim, p_fmt)
            states.append(state)
        out.append(_combine(states, out_dtype).reshape(Hq, T, dv))
    return torch.stack(out)


def _combine(states, out_dtype):
    """the states ``(m, Z, acc, bad)`` of a row's runs of chunks combined in the order given, none skipped: ``M`` the maximum over all,
    then ``Z = Z_0 a_0 (+ Z_i a_i ...)`` with ``a_i = E(m_i - M)``, ``acc`` alike, every multiply and add on its own; then ``_finish``"""
    M = states[0][0]
    for st in states[1:]:
        M = torch.maximum(M, st[0])
    Z = acc = bad = None
    for i, (m_i, Z_i, acc_i, bad_i) in enumerate(states):
        a_i = _exp_def(m_i - M)
        Z, acc, bad = (Z_i * a_i, acc_i * a_i, bad_i) if i == 0 else (Z + Z_i * a_i, acc + acc_i * a_i, bad | bad_i)
    return _finish(M, Z, acc, bad, out_dtype)


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


_check_q4 = partial(_mx_common._check_operand, what="[B, Hq, T, d]", least=4, most=4, needs="exactly 4 dimensions")
_check_k4 = partial(_mx_common._check_operand, what="[B, Hkv, S, d]", least=4, most=4, needs="exactly 4 dimensions")
_check_vt4 = partial(_mx_common._check_operand, what="[B, Hkv, dv, S]", least=4, most=4, needs="exactly 4 dimensions")
MX_DECODE_MAX_ROWS = 64          # r * T: the packed rows of a GQA group that one (sequence, kv head) serves


def mx_flash_decode(q_codes: torch.Tensor, q_scales: torch.Tensor, qk_fmt: str, k_codes: torch.Tensor, k_scales: torch.Tensor,
                    vt_codes: torch.Tensor, vt_scales: torch.Tensor, v_fmt: str, kv_len: Optional[torch.Tensor] = None, *, scale: float,
                    is_causal: bool = False, p_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32,
                    kv_splits="auto") -> torch.Tensor:
    """Grouped-query attention on MX codes for decoding: ``q_codes [B, Hq, T, d]`` (a few new tokens) against a cache ``k_codes [B, Hkv,
    S, d]`` / ``vt_codes [B, Hkv, dv, S]``, all exactly 4-D uint8 codes with the scales ``mx_flash_attention`` takes.  ``Hq = r * Hkv`` and
    query head ``h`` uses key/value head ``h // r`` -- the ``repeat_interleave`` convention of ``F.scaled_dot_product_attention(
    enable_gqa=True)`` -- but the cache is read ONCE per group, not ``r`` times.  Returns ``[B, Hq, T, dv]`` in ``out_dtype``.

    ``kv_len`` (None, or an int32 tensor ``[B]`` on the operands' device): sequence ``b`` sees exactly its first ``L_b = clamp(kv_len[b],
    0, S)`` keys; whatever the cache holds behind them -- NaN included -- is not seen.  It is read ON the device: no host
    synchronisation, so the call can be captured in a graph and ``kv_len`` updated in place between replays.

    ``is_causal`` is aligned BOTTOM-RIGHT, the decoding convention: token ``t`` admits the keys ``j <= L_b - T + t``.  For ``T == S ==
    L_b`` that is the top-left triangle of ``mx_flash_attention``; for ``T != S`` the two calls differ.

    ``kv_splits`` (an int ``>= 1`` or ``"auto"``) cuts the key axis into that many runs of whole chunks of 128 keys, counted on ``S``;
    each run is walked with the streamed kernel's chunk recurrence and the runs are combined in ascending order.  The count is part of
    the numerics (``_decode_def``, the header's "MX flash attention, decode"; bit for bit on either device); ``"auto"`` is
    ``_decode_splits``, a function of the shapes alone.  With ``kv_splits=1``, no ``kv_len`` and no ``is_causal`` the result is, bit
    for bit, ``mx_flash_attention(rows="streamed")`` on the ``repeat_interleave``d cache.

    Supported range: ``r * T <= 64``, ``S >= 1``, ``1 <= d <= 128``, ``1 <= dv <= 128``, every format triple, ``out_dtype`` float32 /
    bfloat16 / float16; anything else raises ``ValueError`` naming the bound.  GPU tensors take one launch (``kv_splits == 1``) or two;
    CPU tensors evaluate ``_decode_def``.  Never differentiable; no arbitrary mask."""
    _check_q4("q", q_codes, q_scales, qk_fmt)
    _check_k4("k", k_codes, k_scales, qk_fmt)
    _check_vt4("vt", vt_codes, vt_scales, v_fmt)
    _mx_format(p_fmt)
    _check_dtype("out_dtype", out_dtype)
    (B, Hq, T, d), (_, Hkv, S, _), dv, dev = q_codes.shape, k_codes.shape, vt_codes.shape[2], q_codes.device
    if k_codes.shape[0] != B or tuple(vt_codes.shape[:2]) != (B, Hkv):
        raise ValueError(f"q_codes {tuple(q_codes.shape)}, k_codes {tuple(k_codes.shape)} and vt_codes {tuple(vt_codes.shape)} disagree on "
                         "B or Hkv")
    if Hkv < 1 or Hq % Hkv != 0:
        raise ValueError(f"Hq = {Hq} is no multiple of Hkv = {Hkv}: query head h uses key/value head h // (Hq / Hkv)")
    if k_codes.shape[-1] != d:
        raise ValueError(f"q_codes {tuple(q_codes.shape)} and k_codes {tuple(k_codes.shape)} disagree on d (their last dimensions)")
    if vt_codes.shape[-1] != S:
        raise ValueError(f"k_codes {tuple(k_codes.shape)} [B, Hkv, S, d] and vt_codes {tuple(vt_codes.shape)} [B, Hkv, dv, S] disagree on S")
    R = Hq // Hkv * T
    if R > MX_DECODE_MAX_ROWS:
        raise ValueError(f"mx_flash_decode takes (Hq / Hkv) * T <= {MX_DECODE_MAX_ROWS}, got {Hq // Hkv} * {T} = {R}: longer runs of "
                         'queries take mx_flash_attention(..., rows="streamed") on the repeated cache')
    if S < 1:
        raise ValueError(f"mx_flash_decode takes S >= 1, got S = {S}")
    for name, n in (("d", d), ("dv", dv)):
        if n > _hip.MX_FLASH_MAX_D or (n < 1 and name == "d"):
            raise ValueError(f"mx_flash_decode takes 1 <= {name} <= {_hip.MX_FLASH_MAX_D}, got {name} = {n}")
    for name, t in (("k_codes", k_codes), ("vt_codes", vt_codes)):
        if t.device != dev:
            raise ValueError(f"q_codes is on {dev} but {name} on {t.device}")
    if kv_len is not None:
        if not isinstance(kv_len, torch.Tensor) or kv_len.dtype != torch.int32 or tuple(kv_len.shape) != (B,) or kv_len.device != dev:
            raise ValueError(f"kv_len must be an int32 tensor of shape ({B},) on {dev}, got "
                             + (f"{kv_len.dtype} {tuple(kv_len.shape)} on {kv_len.device}" if isinstance(kv_len, torch.Tensor)
                                else type(kv_len).__name__))
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError(f"scale must be a float, got {type(scale).__name__}")
    chunks = -(-S // _CHUNK)
    if kv_splits == "auto":
        kv_splits = _decode_splits(B * Hkv * -(-R // 16), chunks)
    elif isinstance(kv_splits, bool) or not isinstance(kv_splits, int) or kv_splits < 1:
        raise ValueError(f'kv_splits must be an int >= 1 or "auto", got {kv_splits!r}')
    if 0 in (B, Hq, T, dv):
        return q_codes.new_empty((B, Hq, T, dv), dtype=out_dtype)
    with torch.no_grad():
        ops = (q_codes.contiguous(), q_scales.contiguous(), qk_fmt, k_codes.contiguous(), k_scales.contiguous(),
               vt_codes.contiguous(), vt_scales.contiguous(), v_fmt, None if kv_len is None else kv_len.contiguous())
        if not q_codes.is_cuda:
            return _decode_def(*ops, float(scale), bool(is_causal), p_fmt, out_dtype, kv_splits)
        return _hip.mx_flash_decode(*ops, float(scale), bool(is_causal), p_fmt, out_dtype, kv_splits)


MX_PAGE_MIN = 32                 # keys per page: a power of two >= 32, so a block of 32 along S never straddles a page
_check_kp = partial(_mx_common._check_operand, what="[P, Hkv, page, d]", least=4, most=4, needs="exactly 4 dimensions")
_check_vtp = partial(_mx_common._check_operand, what="[P, Hkv, dv, page]", least=4, most=4, needs="exactly 4 dimensions",
                     axis=" (page / 32 blocks)")


def _check_pool(fn: str, k_pool, k_pool_scales, qk_fmt: str, vt_pool, vt_pool_scales, v_fmt: str, block_table, kv_len, B=None):
    """the paged operands of ``fn``: the pool pair, ``block_table`` int32 ``[B, NP]`` and ``kv_len`` int32 ``[B]`` on the pool's device"""
    _check_kp("k_pool", k_pool, k_pool_scales, qk_fmt)
    (P, Hkv, page, _), dev = k_pool.shape, k_pool.device
    if page < MX_PAGE_MIN or page & (page - 1):
        raise ValueError(f"{fn} takes a page (k_pool's third dimension) that is a power of two >= {MX_PAGE_MIN}, got page = {page}")
    _check_vtp("vt_pool", vt_pool, vt_pool_scales, v_fmt)
    if tuple(vt_pool.shape[:2]) != (P, Hkv) or vt_pool.shape[3] != page:
        raise ValueError(f"k_pool {tuple(k_pool.shape)} [P, Hkv, page, d] and vt_pool {tuple(vt_pool.shape)} [P, Hkv, dv, page] disagree on "
                         "P, Hkv or page")
    if P < 1 or Hkv < 1:
        raise ValueError(f"{fn} takes a pool of P >= 1 pages and Hkv >= 1, got P = {P}, Hkv = {Hkv}")
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2 or \
            (B is not None and block_table.shape[0] != B) or block_table.shape[1] < 1 or block_table.device != dev:
        raise ValueError(f"block_table must be an int32 tensor of shape ({'B' if B is None else B}, NP >= 1) on {dev}, got "
                         + (f"{block_table.dtype} {tuple(block_table.shape)} on {block_table.device}"
                            if isinstance(block_table, torch.Tensor) else type(block_table).__name__))
    B = block_table.shape[0]
    if not isinstance(kv_len, torch.Tensor) or kv_len.dtype != torch.int32 or tuple(kv_len.shape) != (B,) or kv_len.device != dev:
        raise ValueError(f"kv_len must be an int32 tensor of shape ({B},) on {dev}, got "
                         + (f"{kv_len.dtype} {tuple(kv_len.shape)} on {kv_len.device}" if isinstance(kv_len, torch.Tensor)
                            else type(kv_len).__name__))
    if vt_pool.device != dev:
        raise ValueError(f"k_pool is on {dev} but vt_pool on {vt_pool.device}")


def _paged_gather(k_pool, k_pool_scales, vt_pool, vt_pool_scales, block_table):
    """the contiguous cache ``(k [B, Hkv, NP * page, d], ks, vt [B, Hkv, dv, NP * page], vts)`` that ``block_table [B, NP]`` names in the
    pool; the page of an entry outside ``[0, P)`` is zero codes under the scale byte 127"""
    (B, NP), P = block_table.shape, k_pool.shape[0]
    idx = block_table.to(torch.int64)
    ok = ((idx >= 0) & (idx < P)).view(B, NP, 1, 1, 1)
    idx = idx.clamp(0, P - 1).reshape(-1)
    pages = [torch.where(ok, t.index_select(0, idx).reshape((B, NP) + t.shape[1:]), torch.tensor(fill, dtype=torch.uint8, device=t.device))
             for t, fill in ((k_pool, 0), (k_pool_scales, 127), (vt_pool, 0), (vt_pool_scales, 127))]
    k, ks = (t.permute(0, 2, 1, 3, 4).reshape(B, t.shape[2], NP * t.shape[3], t.shape[4]) for t in pages[:2])
    vt, vts = (t.permute(0, 2, 3, 1, 4).reshape(B, t.shape[2], t.shape[3], NP * t.shape[4]) for t in pages[2:])
    return k, ks, vt, vts


def _decode_paged_def(qc, qs, qk_fmt: str, k_pool, k_pool_scales, vt_pool, vt_pool_scales, v_fmt: str, block_table, kv_len, scale: float,
                      causal: bool, p_fmt: str, out_dtype, splits: int):
    """The paged decode kernel's definition (``include/qsparse_hip.h``, "MX flash attention, paged decode"), on either device:
    ``_decode_def`` on the gathered cache, ``S = NP * page``.  ``_decode_def`` slices every sequence to ``L_b``, so the entries at or
    behind ``ceil(L_b / page)`` mean nothing here either."""
    k, ks, vt, vts = _paged_gather(k_pool, k_pool_scales, vt_pool, vt_pool_scales, block_table)
    return _decode_def(qc, qs, qk_fmt, k, ks, vt, vts, v_fmt, kv_len, scale, causal, p_fmt, out_dtype, splits)


def _shared_chunks(page: int, NP: int, NPs: int, shared_len: int):
    """``(Ls, Cs)`` of the shared-prefix decode: the shared keys -- ``shared_len`` clamped to ``[0, min(NPs, NP) * page]`` and rounded DOWN
    to a whole number of chunks of 128 and of pages -- and their chunks"""
    u = max(_CHUNK, page)
    Ls = min(max(shared_len, 0), min(NPs, NP) * page) // u * u
    return Ls, Ls // _CHUNK


def _decode_shared_def(qc, qs, qk_fmt: str, k_pool, k_pool_scales, vt_pool, vt_pool_scales, v_fmt: str, block_table, kv_len, shared_table,
                       shared_len, scale: float, causal: bool, p_fmt: str, out_dtype, splits: int, shared_splits: int):
    """The shared-prefix paged decode's definition (``include/qsparse_hip.h``, "MX flash attention, shared-prefix paged decode"), on either
    device.  The first ``Ls`` keys of every sequence are the pages of ``shared_table``, the others ``block_table``'s; the gathered cache
    is sliced to ``L_b``; each row has ``shared_splits`` runs of the chunks below ``Cs = Ls / 128`` and ``splits`` runs of the chunks from
    ``Cs`` on, each walked with ``_chunk_step`` from the empty state, and ``_combine`` takes them in that order.  It reads the lengths
    on the host: it is what the tests compare against, not what a graph captures."""
    (B, Hq, T, d), (_, Hkv, page, _), dv, NP, NPs, dev = qc.shape, k_pool.shape, vt_pool.shape[2], block_table.shape[1], shared_table.shape[0], qc.device
    S, r = NP * page, Hq // Hkv
    Ls, Cs = _shared_chunks(page, NP, NPs, int(shared_len[0]))
    merged = block_table.clone()
    merged[:, :Ls // page] = shared_table[:Ls // page]
    kc, ks, vc, vs = _paged_gather(k_pool, k_pool_scales, vt_pool, vt_pool_scales, merged)
    cps_s = -(-max(_shared_chunks(page, NP, NPs, S)[1], 1) // shared_splits)
    cps = -(-(-(-S // _CHUNK)) // splits)
    runs = [(i * cps_s, min((i + 1) * cps_s, Cs)) for i in range(shared_splits)] + [(Cs + i * cps, Cs + (i + 1) * cps) for i in range(splits)]
    tok = (torch.arange(r * T, device=dev) % T)[:, None]
    out = []
    for b, L in enumerate(min(max(int(n), 0), S) for n in kv_len.tolist()):
        q = (qc[b].reshape(Hkv, r * T, d), qs[b].reshape(Hkv, r * T, -1))
        kv = (kc[b, :, :L], ks[b, :, :L], vc[b, :, :, :L], vs[b, :, :, :-(-L // 32)])
        lim = (tok + (L - T + 1)).clamp(min=0) if causal else None
        states = []
        for lo, hi in runs:
            state = _empty_state(Hkv, r * T, dv, dev)
            for c in range(lo, min(hi, -(-L // _CHUNK))):
                state = _chunk_step(state, c, *q, qk_fmt, *kv[:2], *kv[2:], v_fmt, None, scale, lim, p_fmt)
            states.append(state)
        out.append(_combine(states, out_dtype).reshape(Hq, T, dv))
    return torch.stack(out)


def mx_flash_decode_paged(q_codes: torch.Tensor, q_scales: torch.Tensor, qk_fmt: str, k_pool: torch.Tensor, k_pool_scales: torch.Tensor,
                          vt_pool: torch.Tensor, vt_pool_scales: torch.Tensor, v_fmt: str, block_table: torch.Tensor, kv_len: torch.Tensor,
                          *, scale: float, is_causal: bool = False, p_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32,
                          kv_splits="auto", shared=None, shared_splits="auto") -> torch.Tensor:
    """``mx_flash_decode`` on a PAGED cache.  The pool is ``k_pool [P, Hkv, page, d]`` / ``k_pool_scales [P, Hkv, page, ceil(d / 32)]`` and
    ``vt_pool [P, Hkv, dv, page]`` / ``vt_pool_scales [P, Hkv, dv, page / 32]``, contiguous, ``page`` a power of two ``>= 32``.
    ``block_table`` (int32 ``[B, NP]`` on the operands' device) says where a sequence's keys live: position ``j`` of sequence ``b`` is row
    ``j % page`` of ``k_pool[block_table[b, j // page]]`` and column ``j % page`` of ``vt_pool[...]``.  Several sequences may name one page
    (a shared prefix).  The logical capacity is ``S = NP * page``; ``kv_len`` (int32 ``[B]``) is required.

    The result IS ``mx_flash_decode`` on the gathered cache, bit for bit on either device (``_decode_paged_def``): splits are counted on
    ``S = NP * page``, ``"auto"`` is ``_decode_splits(B * Hkv * ceil(R / 16), ceil(S / 128))``, ``is_causal`` is bottom-right.  The table
    and the lengths are read ON the device: the call can be captured in a graph and both rewritten in place between replays.

    With ``L_b = clamp(kv_len[b], 0, S)``, the entries ``block_table[b, n]`` with ``n * page >= L_b`` are never turned into an address and
    may hold anything.  An entry in the live range that lies outside ``[0, P)`` is not dereferenced either: its page reads as zero
    codes under the scale byte 127.  That is a guard, not a feature.

    ``shared=(shared_table, shared_len)`` -- int32 ``[NPs >= 1]`` and int32 ``[1]`` on the pool's device, both read ON the device -- says
    that every sequence BEGINS with the same keys: page ``n`` of every sequence is ``shared_table[n]`` where ``(n + 1) * page <= Ls``,
    ``Ls`` being ``shared_len[0]`` clamped to ``[0, min(NPs, NP) * page]`` and rounded down to a multiple of ``max(128, page)``;
    ``block_table`` is not looked at there, and ``kv_len`` still counts those keys.  The kernel then reads the shared keys once per 16
    query rows of the batch instead of once per sequence.  The result is ``_decode_shared_def``'s, bit for bit on either device (the
    header's "MX flash attention, shared-prefix paged decode"): ``shared_splits`` runs of the shared chunks, then ``kv_splits`` runs of
    the chunks behind them, combined in that order -- the same recurrence as the call without ``shared``, cut at other chunks, so not
    its bytes.  ``shared_splits`` is an int ``>= 1`` or ``"auto"``: ``_decode_splits(Hkv * ceil(B * R / 16), Csmax)``, a function of
    the shapes alone; without ``shared`` it is ignored.  Vt codes of the shared pages that some sequence of the batch sees must not
    be NaN, even for a sequence too short to see them.

    Supported range: that of ``mx_flash_decode`` (``r * T <= 64``, ``d, dv <= 128``, every format triple, three output dtypes); anything
    else raises ``ValueError``.  GPU tensors take one launch (``kv_splits == 1``) or two (``qs_mx_flash_decode_paged_v``, with ``shared``
    ``qs_mx_flash_decode_shared_paged_v``; no fallback and no gathered copy); CPU tensors evaluate ``_decode_paged_def`` /
    ``_decode_shared_def``."""
    _check_q4("q", q_codes, q_scales, qk_fmt)
    _mx_format(p_fmt)
    _check_dtype("out_dtype", out_dtype)
    (B, Hq, T, d), dev = q_codes.shape, q_codes.device
    _check_pool("mx_flash_decode_paged", k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, block_table, kv_len, B)
    (P, Hkv, page, _), dv, NP = k_pool.shape, vt_pool.shape[2], block_table.shape[1]
    if k_pool.device != dev:
        raise ValueError(f"q_codes is on {dev} but k_pool on {k_pool.device}")
    if Hq % Hkv != 0:
        raise ValueError(f"Hq = {Hq} is no multiple of Hkv = {Hkv}: query head h uses key/value head h // (Hq / Hkv)")
    if k_pool.shape[-1] != d:
        raise ValueError(f"q_codes {tuple(q_codes.shape)} and k_pool {tuple(k_pool.shape)} disagree on d (their last dimensions)")
    R = Hq // Hkv * T
    if R > MX_DECODE_MAX_ROWS:
        raise ValueError(f"mx_flash_decode_paged takes (Hq / Hkv) * T <= {MX_DECODE_MAX_ROWS}, got {Hq // Hkv} * {T} = {R}")
    for name, n in (("d", d), ("dv", dv)):
        if n > _hip.MX_FLASH_MAX_D or (n < 1 and name == "d"):
            raise ValueError(f"mx_flash_decode_paged takes 1 <= {name} <= {_hip.MX_FLASH_MAX_D}, got {name} = {n}")
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError(f"scale must be a float, got {type(scale).__name__}")
    if kv_splits == "auto":
        kv_splits = _decode_splits(B * Hkv * -(-R // 16), -(-NP * page // _CHUNK))
    elif isinstance(kv_splits, bool) or not isinstance(kv_splits, int) or kv_splits < 1:
        raise ValueError(f'kv_splits must be an int >= 1 or "auto", got {kv_splits!r}')
    if shared is not None:
        if not isinstance(shared, (tuple, list)) or len(shared) != 2:
            raise ValueError(f"shared must be None or a pair (shared_table, shared_len), got {type(shared).__name__}")
        for name, t, what in (("shared_table", shared[0], "(NPs >= 1,)"), ("shared_len", shared[1], "(1,)")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < 1 or \
                    (name == "shared_len" and t.shape[0] != 1) or t.device != dev:
                raise ValueError(f"{name} must be an int32 tensor of shape {what} on {dev}, got "
                                 + (f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__))
        if shared_splits == "auto":
            shared_splits = _decode_splits(Hkv * -(-B * R // 16), _shared_chunks(page, NP, shared[0].shape[0], NP * page)[1])
        elif isinstance(shared_splits, bool) or not isinstance(shared_splits, int) or shared_splits < 1:
            raise ValueError(f'shared_splits must be an int >= 1 or "auto", got {shared_splits!r}')
    if 0 in (B, Hq, T, dv):
        return q_codes.new_empty((B, Hq, T, dv), dtype=out_dtype)
    for name, t in (("k_pool", k_pool), ("k_pool_scales", k_pool_scales), ("vt_pool", vt_pool), ("vt_pool_scales", vt_pool_scales)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: the pool is addressed through block_table, not copied")
    with torch.no_grad():
        ops = (q_codes.contiguous(), q_scales.contiguous(), qk_fmt, k_pool, k_pool_scales, vt_pool, vt_pool_scales, v_fmt,
               block_table.contiguous(), kv_len.contiguous())
        if shared is not None:
            ops += (shared[0].contiguous(), shared[1].contiguous())
            fn = _hip.mx_flash_decode_shared_paged if q_codes.is_cuda else _decode_shared_def
            return fn(*ops, float(scale), bool(is_causal), p_fmt, out_dtype, kv_splits, shared_splits)
        if not q_codes.is_cuda:
            return _decode_paged_def(*ops, float(scale), bool(is_causal), p_fmt, out_dtype, kv_splits)
        return _hip.mx_flash_decode_paged(*ops, float(scale), bool(is_causal), p_fmt, out_dtype, kv_splits)


def _check_prefill(fn: str, q_codes, Hkv: int, d_k: int, dv: int, scale, k_shape):
    """the checks ``mx_flash_prefill`` and ``mx_flash_prefill_paged`` share once their operands have passed their own: the group, ``d``,
    the head sizes and ``scale``"""
    (_, Hq, _, d) = q_codes.shape
    if Hkv < 1 or Hq % Hkv != 0:
        raise ValueError(f"Hq = {Hq} is no multiple of Hkv = {Hkv}: query head h uses key/value head h // (Hq / Hkv)")
    if d_k != d:
        raise ValueError(f"q_codes {tuple(q_codes.shape)} and the keys {tuple(k_shape)} disagree on d (their last dimensions)")
    for name, n in (("d", d), ("dv", dv)):
        if n > _hip.MX_FLASH_MAX_D or (n < 1 and name == "d"):
            raise ValueError(f"{fn} takes 1 <= {name} <= {_hip.MX_FLASH_MAX_D}, got {name} = {n}")
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError(f"scale must be a float, got {type(scale).__name__}")


def mx_flash_prefill(q_codes: torch.Tensor, q_scales: torch.Tensor, qk_fmt: str, k_codes: torch.Tensor, k_scales: torch.Tensor,
                     vt_codes: torch.Tensor, vt_scales: torch.Tensor, v_fmt: str, kv_len: Optional[torch.Tensor] = None, *, scale: float,
                     is_causal: bool = False, p_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Grouped-query attention of MANY new tokens against the cache they were just appended to -- chunked prefill, prefix reuse, long
    speculative or verify runs: ``q_codes [B, Hq, T, d]`` against ``k_codes [B, Hkv, S, d]`` / ``vt_codes [B, Hkv, dv, S]``, the operands
    of ``mx_flash_decode`` with no bound on ``(Hq / Hkv) * T`` and no ``kv_splits``.  Returns ``[B, Hq, T, dv]`` in ``out_dtype``.

    ``kv_len`` (None, or int32 ``[B]`` on the operands' device) is the length AFTER the append: sequence ``b`` sees its first ``L_b =
    clamp(kv_len[b], 0, S)`` keys and nothing behind them.  It is read ON the device, so ``mx_kv_append`` and this call fit one captured
    graph.  ``is_causal`` is aligned BOTTOM-RIGHT: token ``t`` admits the keys ``j <= L_b - T + t``; a row that admits nothing --
    ``L_b - T + t < 0`` included -- is NaN.

    The result IS ``_decode_def(..., splits=1)``, bit for bit on either device.  So for ``(Hq / Hkv) * T <= 64`` it equals
    ``mx_flash_decode(kv_splits=1)``; with no ``kv_len`` and no ``is_causal`` it equals ``mx_flash_attention(rows="streamed")`` on the
    ``repeat_interleave``d cache; in general it equals that call on the repeated cache sliced to ``L_b`` with the bottom-right limit as
    an additive ``-inf`` mask -- without the copy, the host read of ``kv_len`` or the mask, reading the cache once per group and
    skipping the chunks of keys above the diagonal.

    Supported range: ``T >= 1``, any ``Hq / Hkv``, ``S >= 1``, ``1 <= d, dv <= 128``, every format triple, ``out_dtype`` float32 /
    bfloat16 / float16; anything else raises ``ValueError``.  GPU tensors take ONE launch (``qs_mx_flash_prefill_v``, no fallback); CPU
    tensors evaluate the definition.  Never differentiable; no arbitrary mask."""
    _check_q4("q", q_codes, q_scales, qk_fmt)
    _check_k4("k", k_codes, k_scales, qk_fmt)
    _check_vt4("vt", vt_codes, vt_scales, v_fmt)
    _mx_format(p_fmt)
    _check_dtype("out_dtype", out_dtype)
    (B, Hq, T, d), (_, Hkv, S, _), dv, dev = q_codes.shape, k_codes.shape, vt_codes.shape[2], q_codes.device
    if k_codes.shape[0] != B or tuple(vt_codes.shape[:2]) != (B, Hkv):
        raise ValueError(f"q_codes {tuple(q_codes.shape)}, k_codes {tuple(k_codes.shape)} and vt_codes {tuple(vt_codes.shape)} disagree on "
                         "B or Hkv")
    if vt_codes.shape[-1] != S:
        raise ValueError(f"k_codes {tuple(k_codes.shape)} [B, Hkv, S, d] and vt_codes {tuple(vt_codes.shape)} [B, Hkv, dv, S] disagree on S")
    _check_prefill("mx_flash_prefill", q_codes, Hkv, k_codes.shape[-1], dv, scale, k_codes.shape)
    if S < 1:
        raise ValueError(f"mx_flash_prefill takes S >= 1, got S = {S}")
    for name, t in (("k_codes", k_codes), ("vt_codes", vt_codes)):
        if t.device != dev:
            raise ValueError(f"q_codes is on {dev} but {name} on {t.device}")
    if kv_len is not None:
        if not isinstance(kv_len, torch.Tensor) or kv_len.dtype != torch.int32 or tuple(kv_len.shape) != (B,) or kv_len.device != dev:
            raise ValueError(f"kv_len must be an int32 tensor of shape ({B},) on {dev}, got "
                             + (f"{kv_len.dtype} {tuple(kv_len.shape)} on {kv_len.device}" if isinstance(kv_len, torch.Tensor)
                                else type(kv_len).__name__))
    if 0 in (B, Hq, T, dv):
        return q_codes.new_empty((B, Hq, T, dv), dtype=out_dtype)
    with torch.no_grad():
        ops = (q_codes.contiguous(), q_scales.contiguous(), qk_fmt, k_codes.contiguous(), k_scales.contiguous(),
               vt_codes.contiguous(), vt_scales.contiguous(), v_fmt)
        kv_len = None if kv_len is None else kv_len.contiguous()
        if not q_codes.is_cuda:
            return _decode_def(*ops, kv_len, float(scale), bool(is_causal), p_fmt, out_dtype, 1)
        return _hip.mx_flash_prefill(*ops, None, kv_len, float(scale), bool(is_causal), p_fmt, out_dtype)


def mx_flash_prefill_paged(q_codes: torch.Tensor, q_scales: torch.Tensor, qk_fmt: str, k_pool: torch.Tensor, k_pool_scales: torch.Tensor,
                           vt_pool: torch.Tensor, vt_pool_scales: torch.Tensor, v_fmt: str, block_table: torch.Tensor, kv_len: torch.Tensor,
                           *, scale: float, is_causal: bool = False, p_fmt: str = "mxfp8_e4m3",
                           out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``mx_flash_prefill`` on a PAGED cache: the pool, ``block_table`` (int32 ``[B, NP]``) and ``kv_len`` (int32 ``[B]``, required, the
    length AFTER the append) are ``mx_flash_decode_paged``'s, ``S = NP * page``.  The result IS ``mx_flash_prefill`` on the gathered
    cache -- ``_decode_paged_def(..., splits=1)`` -- bit for bit on either device.  Table and lengths are read ON the device; entries
    ``block_table[b, n]`` with ``n * page >= L_b`` are never turned into an address, a live entry outside ``[0, P)`` is not
    dereferenced and reads as zero codes under the scale byte 127.  The pools must be contiguous.  GPU tensors take ONE launch
    (``qs_mx_flash_prefill_v`` with a table; no gathered copy, no fallback); CPU tensors evaluate the definition."""
    _check_q4("q", q_codes, q_scales, qk_fmt)
    _mx_format(p_fmt)
    _check_dtype("out_dtype", out_dtype)
    (B, Hq, T, d), dev = q_codes.shape, q_codes.device
    _check_pool("mx_flash_prefill_paged", k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, block_table, kv_len, B)
    if k_pool.device != dev:
        raise ValueError(f"q_codes is on {dev} but k_pool on {k_pool.device}")
    dv = vt_pool.shape[2]
    _check_prefill("mx_flash_prefill_paged", q_codes, k_pool.shape[1], k_pool.shape[-1], dv, scale, k_pool.shape)
    if 0 in (B, Hq, T, dv):
        return q_codes.new_empty((B, Hq, T, dv), dtype=out_dtype)
    for name, t in (("k_pool", k_pool), ("k_pool_scales", k_pool_scales), ("vt_pool", vt_pool), ("vt_pool_scales", vt_pool_scales)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: the pool is addressed through block_table, not copied")
    with torch.no_grad():
        ops = (q_codes.contiguous(), q_scales.contiguous(), qk_fmt, k_pool, k_pool_scales, vt_pool, vt_pool_scales, v_fmt,
               block_table.contiguous(), kv_len.contiguous())
        if not q_codes.is_cuda:
            return _decode_paged_def(*ops, float(scale), bool(is_causal), p_fmt, out_dtype, 1)
        return _hip.mx_flash_prefill(*ops, float(scale), bool(is_causal), p_fmt, out_dtype)


def _check_cu(fn: str, cu_seqlens, B: int, dev):
    """``cu_seqlens``: int32 ``[B + 1]`` on the operands' device (its values are the device's business)"""
    if not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dtype != torch.int32 or tuple(cu_seqlens.shape) != (B + 1,) or \
            cu_seqlens.device != dev:
        raise ValueError(f"{fn}: cu_seqlens must be an int32 tensor of shape ({B + 1},) = (B + 1,) on {dev}, got "
                         + (f"{cu_seqlens.dtype} {tuple(cu_seqlens.shape)} on {cu_seqlens.device}" if isinstance(cu_seqlens, torch.Tensor)
                            else type(cu_seqlens).__name__))


def _ragged_def(qc, qs, qk_fmt: str, kc, ks, vc, vs, v_fmt: str, block_table, kv_len, cu_seqlens, scale: float, causal: bool, p_fmt: str,
                out_dtype):
    """The ragged launch's definition (``include/qsparse_hip.h``, "MX flash attention, ragged"), on either device: ``mx_flash_prefill``
    (``_paged`` with a ``block_table``) of every sequence with ``T_b > 0`` by itself, on its rows of ``qc [Ttot, Hq, d]``; rows that no
    sequence owns stay zero.  It reads ``cu_seqlens`` on the host: what the tests compare against, not what a graph captures."""
    (Ttot, Hq, _), dv = qc.shape, vc.shape[2]
    out = qc.new_zeros((Ttot, Hq, dv), dtype=out_dtype)
    cu = [min(max(int(n), 0), Ttot) for n in cu_seqlens.tolist()]
    for b, (lo, hi) in enumerate(zip(cu[:-1], cu[1:])):
        if hi <= lo:
            continue
        q = (qc[lo:hi].permute(1, 0, 2)[None], qs[lo:hi].permute(1, 0, 2)[None])
        if block_table is None:
            y = _decode_def(*q, qk_fmt, kc[b:b + 1], ks[b:b + 1], vc[b:b + 1], vs[b:b + 1], v_fmt, kv_len[b:b + 1], scale, causal, p_fmt,
                            out_dtype, 1)
        else:
            y = _decode_paged_def(*q, qk_fmt, kc, ks, vc, vs, v_fmt, block_table[b:b + 1], kv_len[b:b + 1], scale, causal, p_fmt, out_dtype, 1)
        out[lo:hi] = y[0].permute(1, 0, 2)
    return out


def _ragged(q_codes, q_scales, qk_fmt, kc, ks, vc, vs, v_fmt, block_table, kv_len, cu_seqlens, scale, is_causal, p_fmt, out_dtype):
    """what ``mx_flash_prefill_ragged`` and ``mx_flash_prefill_ragged_paged`` share behind the checks of their cache"""
    (Ttot, Hq, _), dv, B = q_codes.shape, vc.shape[2], kv_len.shape[0]
    if 0 in (B, Hq, Ttot, dv):
        return q_codes.new_zeros((Ttot, Hq, dv), dtype=out_dtype)
    with torch.no_grad():
        ops = (q_codes.contiguous(), q_scales.contiguous(), qk_fmt, kc, ks, vc, vs, v_fmt, block_table, kv_len.contiguous(),
               cu_seqlens.contiguous(), float(scale), bool(is_causal), p_fmt, out_dtype)
        return _hip.mx_flash_ragged(*ops) if q_codes.is_cuda else _ragged_def(*ops)


_check_q3 = partial(_mx_common._check_operand, what="[Ttot, Hq, d]", least=3, most=3, needs="exactly 3 dimensions")


def mx_flash_prefill_ragged(q_codes: torch.Tensor, q_scales: torch.Tensor, qk_fmt: str, k_codes: torch.Tensor, k_scales: torch.Tensor,
                            vt_codes: torch.Tensor, vt_scales: torch.Tensor, v_fmt: str, kv_len: torch.Tensor, cu_seqlens: torch.Tensor,
                            *, scale: float, is_causal: bool = False, p_fmt: str = "mxfp8_e4m3",
                            out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``mx_flash_prefill`` for a RAGGED batch: sequence ``b`` brings ``T_b`` new tokens, a decode step (``T_b = 1``), a prefill chunk of
    hundreds or none at all, in ONE launch.  The new tokens lie on one flat axis, token-major as a QKV projection writes them:
    ``q_codes [Ttot, Hq, d]`` / ``q_scales [Ttot, Hq, ceil(d / 32)]``; the result is ``[Ttot, Hq, dv]`` in ``out_dtype``.  The cache is
    ``mx_flash_prefill``'s, ``k_codes [B, Hkv, S, d]`` / ``vt_codes [B, Hkv, dv, S]``; ``kv_len`` (int32 ``[B]``, required) is the length
    AFTER the append.

    ``cu_seqlens`` (int32 ``[B + 1]`` on the operands' device, non-decreasing, ``cu_seqlens[0] == 0``) cuts the axis: sequence ``b`` owns
    the tokens ``[cu[b], cu[b + 1])``.  ``Ttot`` may exceed ``cu[B]`` -- the padding of a fixed token budget -- and tokens at or behind
    ``cu[B]`` belong to no sequence: the GPU launch does NOT write their rows of the result, whose content is unspecified (the tensor is
    ``new_empty``); the CPU path leaves them zero.  ``cu_seqlens``, ``kv_len`` (and the table) are read ON the device and never by the
    host, so the call can be captured in a graph and all of them rewritten in place between replays.  The kernel clamps every entry of
    ``cu_seqlens`` into ``[0, Ttot]`` and takes a negative length as 0: a malformed ``cu_seqlens`` gives an unspecified result, but no
    access leaves the operands.

    The result IS ``mx_flash_prefill`` called once per sequence with ``T_b > 0`` on its own rows (``_ragged_def``), bit for bit on
    either device; ``is_causal`` is bottom-right PER SEQUENCE, token ``t`` of sequence ``b`` admits the keys ``j <= L_b - T_b + t``.

    Supported range: ``mx_flash_prefill``'s -- any ``Hq / Hkv``, ``1 <= d, dv <= 128``, every format triple, three output dtypes;
    anything else raises ``ValueError`` naming the bound.  GPU tensors take ONE launch (``qs_mx_flash_ragged_v``; no fallback); CPU
    tensors evaluate the definition.  Never differentiable."""
    _check_q3("q", q_codes, q_scales, qk_fmt)
    _check_k4("k", k_codes, k_scales, qk_fmt)
    _check_vt4("vt", vt_codes, vt_scales, v_fmt)
    _mx_format(p_fmt)
    _check_dtype("out_dtype", out_dtype)
    (B, Hkv, S, _), dv, dev = k_codes.shape, vt_codes.shape[2], q_codes.device
    if tuple(vt_codes.shape[:2]) != (B, Hkv):
        raise ValueError(f"k_codes {tuple(k_codes.shape)} and vt_codes {tuple(vt_codes.shape)} disagree on B or Hkv")
    if vt_codes.shape[-1] != S:
        raise ValueError(f"k_codes {tuple(k_codes.shape)} [B, Hkv, S, d] and vt_codes {tuple(vt_codes.shape)} [B, Hkv, dv, S] disagree on S")
    _check_prefill("mx_flash_prefill_ragged", q_codes[None].transpose(1, 2), Hkv, k_codes.shape[-1], dv, scale, k_codes.shape)
    if S < 1:
        raise ValueError(f"mx_flash_prefill_ragged takes S >= 1, got S = {S}")
    for name, t in (("k_codes", k_codes), ("vt_codes", vt_codes)):
        if t.device != dev:
            raise ValueError(f"q_codes is on {dev} but {name} on {t.device}")
    if not isinstance(kv_len, torch.Tensor) or kv_len.dtype != torch.int32 or tuple(kv_len.shape) != (B,) or kv_len.device != dev:
        raise ValueError(f"kv_len must be an int32 tensor of shape ({B},) on {dev}, got "
                         + (f"{kv_len.dtype} {tuple(kv_len.shape)} on {kv_len.device}" if isinstance(kv_len, torch.Tensor)
                            else type(kv_len).__name__))
    _check_cu("mx_flash_prefill_ragged", cu_seqlens, B, dev)
    return _ragged(q_codes, q_scales, qk_fmt, k_codes.contiguous(), k_scales.contiguous(), vt_codes.contiguous(),
                   vt_scales.contiguous(), v_fmt, None, kv_len, cu_seqlens, scale, is_causal, p_fmt, out_dtype)


def mx_flash_prefill_ragged_paged(q_codes: torch.Tensor, q_scales: torch.Tensor, qk_fmt: str, k_pool: torch.Tensor, k_pool_scales: torch.Tensor,
                                  vt_pool: torch.Tensor, vt_pool_scales: torch.Tensor, v_fmt: str, block_table: torch.Tensor,
                                  kv_len: torch.Tensor, cu_seqlens: torch.Tensor, *, scale: float, is_causal: bool = False,
                                  p_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``mx_flash_prefill_ragged`` on a PAGED cache: the pool, ``block_table`` (int32 ``[B, NP]``) and ``kv_len`` (int32 ``[B]``, the length
    AFTER the append) are ``mx_flash_prefill_paged``'s, ``q_codes [Ttot, Hq, d]`` and ``cu_seqlens`` (int32 ``[B + 1]``) as there.  The
    result IS ``mx_flash_prefill_paged`` per sequence on row ``b`` of the table (``_ragged_def``), bit for bit on either device; dead
    and out-of-range table entries follow ``mx_flash_prefill_paged``'s rules.  Rows at or behind ``cu[B]``: not written by the GPU
    launch (unspecified content), zero on the CPU.  GPU tensors take ONE launch (``qs_mx_flash_ragged_v`` with a table; no gathered
    copy, no fallback); table, lengths and ``cu_seqlens`` are read on the device."""
    _check_q3("q", q_codes, q_scales, qk_fmt)
    _mx_format(p_fmt)
    _check_dtype("out_dtype", out_dtype)
    dev = q_codes.device
    _check_pool("mx_flash_prefill_ragged_paged", k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, block_table, kv_len)
    if k_pool.device != dev:
        raise ValueError(f"q_codes is on {dev} but k_pool on {k_pool.device}")
    _check_prefill("mx_flash_prefill_ragged_paged", q_codes[None].transpose(1, 2), k_pool.shape[1], k_pool.shape[-1], vt_pool.shape[2], scale,
                   k_pool.shape)
    _check_cu("mx_flash_prefill_ragged_paged", cu_seqlens, block_table.shape[0], dev)
    for name, t in (("k_pool", k_pool), ("k_pool_scales", k_pool_scales), ("vt_pool", vt_pool), ("vt_pool_scales", vt_pool_scales)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: the pool is addressed through block_table, not copied")
    return _ragged(q_codes, q_scales, qk_fmt, k_pool, k_pool_scales, vt_pool, vt_pool_scales, v_fmt,
                   block_table.contiguous(), kv_len, cu_seqlens, scale, is_causal, p_fmt, out_dtype)


__all__ = ["mx_flash_attention", "mx_flash_decode", "mx_flash_decode_paged", "mx_flash_prefill", "mx_flash_prefill_paged",
           "mx_flash_prefill_ragged", "mx_flash_prefill_ragged_paged"]
