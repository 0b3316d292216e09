"""Writing the MX KV cache that ``mx_flash_decode`` reads: ``mx_kv_append`` and the thin ``MXKVCache``.

``k_codes [B, Hkv, S, d]`` has its blocks along ``d``, so a new token is a new row.  ``vt_codes [B, Hkv, dv, S]`` has them along ``S``:
a new token lands in the open block of 32, whose scale must be renewed from ALL its values -- re-encoding from the old codes would
round twice.  So the cache keeps ``v_tail [B, Hkv, dv, 32]``, the exact float32 values of the open block, and an append re-quantizes
the touched blocks from it.  The write position is ``kv_len`` on the device: nothing is read by the host, the call can be captured in a
graph.  The definition (``include/qsparse_hip.h``, "MX KV cache append") is ``_append_def`` here; the HIP launch gives the same bits."""
from functools import partial
from typing import Optional

import torch

from qsparse_amd import _hip, _mx_common
from qsparse_amd._mx_common import _check_dtype
from qsparse_amd.mx_flash import (_check_cu, _check_pool, _paged_gather, mx_flash_decode, mx_flash_decode_paged, mx_flash_prefill,
                                  mx_flash_prefill_paged, mx_flash_prefill_ragged_paged)
from qsparse_amd.mx_rope import _rope_def
from qsparse_amd.quantize import MX_BLOCK, _mx_format, quantize_with_mx

MX_KV_MAX_D = 128           # d and dv
_check_k4 = partial(_mx_common._check_operand, what="[B, Hkv, S, d]", least=4, most=4, needs="exactly 4 dimensions", source="MXKVCache")
_check_vt4 = partial(_mx_common._check_operand, what="[B, Hkv, dv, S]", least=4, most=4, needs="exactly 4 dimensions", source="MXKVCache")


def _codes(x32: torch.Tensor, fmt: str):
    return quantize_with_mx(x32, fmt, -1, return_codes=True)[1:]


def _append_def(k_codes, k_scales, qk_fmt, vt_codes, vt_scales, v_fmt, v_tail, kv_len, k_new, v_new, q_new, rope, interleaved):
    """the definition, sequence by sequence in torch ops (reads `kv_len` on the host): the CPU path, and what the GPU tests compare with"""
    (B, Hkv, S, d), T = k_codes.shape, k_new.shape[2]
    q = None if q_new is None else q_new.to(torch.float32)
    k = k_new.to(torch.float32)
    if rope is not None:
        P = rope[0].shape[0]
        pos = (kv_len.clamp(0, S).to(torch.int64)[:, None] + torch.arange(T, device=kv_len.device)).clamp(max=P - 1)      # [B, T]
        cos, sin = (t[pos][:, None] for t in rope)                                                                       # [B, 1, T, d / 2]
        k = _rope_def(k, cos, sin, interleaved, False)
        q = None if q is None else _rope_def(q, cos, sin, interleaved, False)
    for b, L in enumerate(kv_len.clamp(0, S).tolist()):
        Lp = min(L + T, S)
        if Lp == L:
            continue
        n, lo = Lp - L, L // MX_BLOCK * MX_BLOCK
        k_codes[b, :, L:Lp], k_scales[b, :, L:Lp] = _codes(k[b, :, :n], qk_fmt)
        hist = torch.cat((v_tail[b, :, :, :L - lo], v_new[b, :, :n].to(torch.float32).transpose(-1, -2)), -1)             # [Hkv, dv, Lp - lo]
        end = min(S, -(-Lp // MX_BLOCK) * MX_BLOCK)
        codes, scales = _codes(torch.nn.functional.pad(hist, (0, end - Lp)), v_fmt)
        vt_codes[b, :, :, lo:end], vt_scales[b, :, :, lo // MX_BLOCK:-(-end // MX_BLOCK)] = codes, scales
        if Lp % MX_BLOCK:
            frm = max(L, Lp // MX_BLOCK * MX_BLOCK)
            v_tail[b, :, :, frm % MX_BLOCK:Lp % MX_BLOCK] = hist[..., frm - lo:]
    return None if q is None else tuple(_codes(q, qk_fmt))


def mx_kv_append(k_codes: torch.Tensor, k_scales: torch.Tensor, qk_fmt: str, vt_codes: torch.Tensor, vt_scales: torch.Tensor, v_fmt: str,
                 v_tail: torch.Tensor, kv_len: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, *,
                 q_new: Optional[torch.Tensor] = None, rope=None, interleaved: bool = False):
    """Append ``T`` new tokens per sequence to an MX KV cache, in place: ``k_new [B, Hkv, T, d]`` and ``v_new [B, Hkv, T, dv]`` (float32 /
    bfloat16 / float16, one dtype) go into ``k_codes [B, Hkv, S, d]`` / ``k_scales`` (blocks along ``d``, format ``qk_fmt``) and
    ``vt_codes [B, Hkv, dv, S]`` / ``vt_scales`` (blocks along ``S``, format ``v_fmt``) -- the operands of ``mx_flash_decode``.

    ``kv_len`` (int32 ``[B]`` on the operands' device) gives the length BEFORE the append, ``L_b = clamp(kv_len[b], 0, S)``.  It is read
    on the device and not changed: the caller does ``kv_len += T``.  Token ``t`` lands at position ``L_b + t``; a token at a position
    ``>= S`` is not stored.

    ``v_tail`` (float32 ``[B, Hkv, dv, 32]``, written in place) holds the exact float32 values of ``vt``'s open block: column ``j % 32``
    is position ``j`` for ``j`` in ``[32 * floor(L_b / 32), L_b)``, the other columns mean nothing.  Every block of ``vt`` that receives
    a token is quantized anew from it and the new values, so ``vt_codes[..., :L']`` / ``vt_scales[..., :ceil(L' / 32)]`` (``L' = min(L_b +
    T, S)``) are exactly ``quantize_with_mx`` along ``S`` of all ``L'`` float tokens at once; the rest of the open block becomes zero
    codes; blocks before the open one and behind the last touched one keep their bytes.  K rows equal ``quantize_with_mx`` of the row.

    ``rope`` (``None`` or ``(cos, sin)``, float32 ``[P, d / 2]`` with ``P >= S``, as ``mx_rope_table(S, d)`` gives them; ``d`` even)
    rotates token ``t`` of sequence ``b`` by table row ``min(L_b + t, P - 1)`` with ``mx_rope``'s float32 sequence (``interleaved`` as
    there) before it is quantized: ``k_new`` always, ``q_new`` when given.  ``q_new [B, Hq, T, d]`` (``Hq`` a multiple of ``Hkv``) is not
    stored: its codes ``(q_codes [B, Hq, T, d], q_scales)`` in ``qk_fmt`` are returned as new tensors, ready for ``mx_flash_decode``.

    Supported range: ``1 <= d <= 128``, ``1 <= dv <= 128``, ``T >= 1``, every format; rounding to nearest; never differentiable.
    Anything else raises ``ValueError`` naming the bound.  GPU tensors take ONE launch (``qs_mx_kv_append_v``; no fallback); CPU tensors
    evaluate ``_append_def``, which reads ``kv_len``; both give the same bits.  Returns ``None`` without ``q_new``."""
    _check_k4("k", k_codes, k_scales, qk_fmt)
    _check_vt4("vt", vt_codes, vt_scales, v_fmt)
    (B, Hkv, S, d), dv, dev = k_codes.shape, vt_codes.shape[2], k_codes.device
    if tuple(vt_codes.shape[:2]) != (B, Hkv) or vt_codes.shape[3] != S:
        raise ValueError(f"k_codes {tuple(k_codes.shape)} [B, Hkv, S, d] and vt_codes {tuple(vt_codes.shape)} [B, Hkv, dv, S] disagree on "
                         "B, Hkv or S")
    if S < 1:
        raise ValueError(f"mx_kv_append takes S >= 1, got S = {S}")
    for name, n in (("d", d), ("dv", dv)):
        if not 1 <= n <= MX_KV_MAX_D:
            raise ValueError(f"mx_kv_append takes 1 <= {name} <= {MX_KV_MAX_D}, got {name} = {n}")
    if not isinstance(v_tail, torch.Tensor) or v_tail.dtype != torch.float32 or tuple(v_tail.shape) != (B, Hkv, dv, MX_BLOCK):
        raise ValueError(f"v_tail must be a float32 tensor of shape {(B, Hkv, dv, MX_BLOCK)}, got "
                         + (f"{v_tail.dtype} {tuple(v_tail.shape)}" if isinstance(v_tail, torch.Tensor) else type(v_tail).__name__))
    if not isinstance(kv_len, torch.Tensor) or kv_len.dtype != torch.int32 or tuple(kv_len.shape) != (B,):
        raise ValueError(f"kv_len must be an int32 tensor of shape ({B},), got "
                         + (f"{kv_len.dtype} {tuple(kv_len.shape)}" if isinstance(kv_len, torch.Tensor) else type(kv_len).__name__))
    news = (("k_new", k_new, (B, Hkv), d), ("v_new", v_new, (B, Hkv), dv)) + ((("q_new", q_new, (B,), d),) if q_new is not None else ())
    for name, t, lead, last in news:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        _check_dtype(name, t.dtype)
        if t.dim() != 4 or tuple(t.shape[:len(lead)]) != lead or t.shape[3] != last or t.shape[2] != k_new.shape[2]:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {lead + (('Hq',) if len(lead) == 1 else ()) + ('T', last)} "
                             f"with k_new's T")
        if t.dtype != k_new.dtype:
            raise ValueError(f"k_new is {k_new.dtype} but {name} {t.dtype}: the new tokens share one dtype")
    T = k_new.shape[2]
    if T < 1:
        raise ValueError(f"mx_kv_append takes T >= 1, got T = {T}")
    if q_new is not None and (q_new.shape[1] < 1 or q_new.shape[1] % Hkv):
        raise ValueError(f"Hq = {q_new.shape[1]} is no multiple of Hkv = {Hkv}: query head h uses key/value head h // (Hq / Hkv)")
    if rope is not None:
        if not isinstance(rope, (tuple, list)) or len(rope) != 2:
            raise TypeError("rope must be None or a 2-tuple (cos, sin)")
        if d % 2:
            raise ValueError(f"rope needs an even d (the last dimension of k_new), got {d}")
        for name, t in zip(("cos", "sin"), rope):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != d // 2 or t.shape[0] < S:
                raise ValueError(f"{name} must be a float32 tensor [P, d / 2] = [>= {S}, {d // 2}], got "
                                 + (f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__))
        if rope[0].shape != rope[1].shape:
            raise ValueError(f"cos {tuple(rope[0].shape)} and sin {tuple(rope[1].shape)} disagree on P")
    for name, t in (("vt_codes", vt_codes), ("v_tail", v_tail), ("kv_len", kv_len)) + tuple(n[:2] for n in news) + (
            (("cos", rope[0]), ("sin", rope[1])) if rope is not None else ()):
        if t.device != dev:
            raise ValueError(f"k_codes is on {dev} but {name} on {t.device}")
    for name, t in (("k_codes", k_codes), ("k_scales", k_scales), ("vt_codes", vt_codes), ("vt_scales", vt_scales), ("v_tail", v_tail)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: it is written in place")
    if B == 0 or Hkv == 0:
        return None if q_new is None else tuple(k_codes.new_empty(q_new.shape[:3] + (n,)) for n in (d, -(-d // MX_BLOCK)))
    with torch.no_grad():
        k_new, v_new, q_new = (None if t is None else t.detach().contiguous() for t in (k_new, v_new, q_new))
        if not k_codes.is_cuda:
            return _append_def(k_codes, k_scales, qk_fmt, vt_codes, vt_scales, v_fmt, v_tail, kv_len, k_new, v_new, q_new, rope,
                               bool(interleaved))
        cos, sin = (None, None) if rope is None else (t.contiguous() for t in rope)
        return _hip.mx_kv_append(k_codes, k_scales, qk_fmt, vt_codes, vt_scales, v_fmt, v_tail, kv_len.contiguous(), k_new, v_new, q_new,
                                 cos, sin, bool(interleaved))


class MXKVCache:
    """The five buffers of an MX KV cache and its lengths: ``k_codes [B, Hkv, S, d]`` / ``k_scales``, ``vt_codes [B, Hkv, dv, S]`` /
    ``vt_scales``, ``v_tail [B, Hkv, dv, 32]`` and ``kv_len`` (int32 ``[B]``, zero).  ``append`` is ``mx_kv_append`` followed by
    ``kv_len += T``; ``attend`` is ``mx_flash_decode`` on the cache.  Both are graph-capturable; there is no other logic."""

    def __init__(self, B: int, Hkv: int, S: int, d: int, dv: int, qk_fmt: str = "mxfp8_e4m3", v_fmt: str = "mxfp8_e4m3", device=None):
        _mx_format(qk_fmt), _mx_format(v_fmt)
        nb = lambda n: (n + MX_BLOCK - 1) // MX_BLOCK
        z = partial(torch.zeros, dtype=torch.uint8, device=device)
        self.qk_fmt, self.v_fmt = qk_fmt, v_fmt
        self.k_codes, self.k_scales = z((B, Hkv, S, d)), z((B, Hkv, S, nb(d)))
        self.vt_codes, self.vt_scales = z((B, Hkv, dv, S)), z((B, Hkv, dv, nb(S)))
        self.v_tail = torch.zeros((B, Hkv, dv, MX_BLOCK), dtype=torch.float32, device=device)
        self.kv_len = torch.zeros(B, dtype=torch.int32, device=device)

    def append(self, k: torch.Tensor, v: torch.Tensor, q: Optional[torch.Tensor] = None, rope=None, interleaved: bool = False):
        out = mx_kv_append(self.k_codes, self.k_scales, self.qk_fmt, self.vt_codes, self.vt_scales, self.v_fmt, self.v_tail, self.kv_len,
                           k, v, q_new=q, rope=rope, interleaved=interleaved)
        self.kv_len += k.shape[2]
        return out

    def attend(self, q_codes: torch.Tensor, q_scales: torch.Tensor, **kw) -> torch.Tensor:
        return mx_flash_decode(q_codes, q_scales, self.qk_fmt, self.k_codes, self.k_scales, self.vt_codes, self.vt_scales, self.v_fmt,
                               self.kv_len, **kw)

    def prefill(self, q_codes: torch.Tensor, q_scales: torch.Tensor, **kw) -> torch.Tensor:
        """``mx_flash_prefill`` on the cache: any number of new tokens, behind the ``append`` that stored them"""
        return mx_flash_prefill(q_codes, q_scales, self.qk_fmt, self.k_codes, self.k_scales, self.vt_codes, self.vt_scales, self.v_fmt,
                                self.kv_len, **kw)


def _append_paged_def(k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, v_tail, block_table, kv_len, k_new, v_new, q_new, rope,
                      interleaved):
    """the paged append's definition (``include/qsparse_hip.h``, "MX KV cache append, paged"): gather the cache the table names,
    ``_append_def`` on it, and scatter back the pages that hold a position in ``[L_b, L'_b)`` and whose entry lies in ``[0, P)``.  Reads
    ``kv_len`` and the table on the host: the CPU path, and what the GPU tests compare with"""
    pools = (k_pool, k_pool_scales, vt_pool, vt_pool_scales)
    (P, _, page, _), (B, NP), T = k_pool.shape, block_table.shape, k_new.shape[2]
    k, ks, vt, vts = _paged_gather(*pools, block_table)
    out = _append_def(k, ks, qk_fmt, vt, vts, v_fmt, v_tail, kv_len, k_new, v_new, q_new, rope, interleaved)
    S = NP * page
    for b, L in enumerate(kv_len.clamp(0, S).tolist()):
        for n in range(L // page, -(-min(L + T, S) // page)):
            e = int(block_table[b, n])
            if 0 <= e < P:
                k_pool[e], k_pool_scales[e] = k[b, :, n * page:(n + 1) * page], ks[b, :, n * page:(n + 1) * page]
                vt_pool[e], vt_pool_scales[e] = vt[b, ..., n * page:(n + 1) * page], vts[b, ..., n * page // MX_BLOCK:(n + 1) * page // MX_BLOCK]
    return out


def mx_kv_append_paged(k_pool: torch.Tensor, k_pool_scales: torch.Tensor, qk_fmt: str, vt_pool: torch.Tensor, vt_pool_scales: torch.Tensor,
                       v_fmt: str, v_tail: torch.Tensor, block_table: torch.Tensor, kv_len: torch.Tensor, k_new: torch.Tensor,
                       v_new: torch.Tensor, *, q_new: Optional[torch.Tensor] = None, rope=None, interleaved: bool = False):
    """``mx_kv_append`` into the PAGED cache that ``mx_flash_decode_paged`` reads, in place: the pool ``k_pool [P, Hkv, page, d]`` /
    ``vt_pool [P, Hkv, dv, page]`` with their scales, ``block_table`` (int32 ``[B, NP]``) and ``kv_len`` (int32 ``[B]``) as there; ``v_tail
    [B, Hkv, dv, 32]`` float32 stays per sequence and is not paged.

    It is ``mx_kv_append``'s rule with ``S = NP * page`` and positions translated through the table (``_append_paged_def``; bit for bit
    on either device): K row ``L_b + t`` goes to row ``(L_b + t) % page`` of its page; every 32-block of ``vt`` that receives a position is
    quantized again from ``v_tail`` plus the new values, inside its page; ``v_tail`` is updated as there; tokens at ``>= S`` are dropped;
    ``rope`` tables (``P_rope >= S`` rows) are indexed by the logical position; ``q_new`` comes back as codes.  A token whose page entry is
    outside ``[0, P)`` is not stored and its ``vt`` block is skipped, while ``v_tail`` advances as if it had been.  Every byte of the
    pool outside the touched rows and blocks keeps its value.  One call must not write one page for two sequences -- the caller's
    duty; the result for that page is unspecified, but no access leaves the pool.

    GPU tensors take ONE launch (``qs_mx_kv_append_paged_v``; no fallback); the table and ``kv_len`` are read on the device and not
    changed, so the call can be captured in a graph."""
    _check_pool("mx_kv_append_paged", k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, block_table, kv_len)
    (P, Hkv, page, d), dv, (B, NP), dev = k_pool.shape, vt_pool.shape[2], block_table.shape, k_pool.device
    S = NP * page
    for name, n in (("d", d), ("dv", dv)):
        if not 1 <= n <= MX_KV_MAX_D:
            raise ValueError(f"mx_kv_append_paged takes 1 <= {name} <= {MX_KV_MAX_D}, got {name} = {n}")
    if not isinstance(v_tail, torch.Tensor) or v_tail.dtype != torch.float32 or tuple(v_tail.shape) != (B, Hkv, dv, MX_BLOCK):
        raise ValueError(f"v_tail must be a float32 tensor of shape {(B, Hkv, dv, MX_BLOCK)}, got "
                         + (f"{v_tail.dtype} {tuple(v_tail.shape)}" if isinstance(v_tail, torch.Tensor) else type(v_tail).__name__))
    news = (("k_new", k_new, (B, Hkv), d), ("v_new", v_new, (B, Hkv), dv)) + ((("q_new", q_new, (B,), d),) if q_new is not None else ())
    for name, t, lead, last in news:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        _check_dtype(name, t.dtype)
        if t.dim() != 4 or tuple(t.shape[:len(lead)]) != lead or t.shape[3] != last or t.shape[2] != k_new.shape[2]:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {lead + (('Hq',) if len(lead) == 1 else ()) + ('T', last)} "
                             f"with k_new's T")
        if t.dtype != k_new.dtype:
            raise ValueError(f"k_new is {k_new.dtype} but {name} {t.dtype}: the new tokens share one dtype")
    T = k_new.shape[2]
    if T < 1:
        raise ValueError(f"mx_kv_append_paged takes T >= 1, got T = {T}")
    if q_new is not None and (q_new.shape[1] < 1 or q_new.shape[1] % Hkv):
        raise ValueError(f"Hq = {q_new.shape[1]} is no multiple of Hkv = {Hkv}: query head h uses key/value head h // (Hq / Hkv)")
    if rope is not None:
        if not isinstance(rope, (tuple, list)) or len(rope) != 2:
            raise TypeError("rope must be None or a 2-tuple (cos, sin)")
        if d % 2:
            raise ValueError(f"rope needs an even d (the last dimension of k_new), got {d}")
        for name, t in zip(("cos", "sin"), rope):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != d // 2 or t.shape[0] < S:
                raise ValueError(f"{name} must be a float32 tensor [P, d / 2] = [>= {S}, {d // 2}], got "
                                 + (f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__))
        if rope[0].shape != rope[1].shape:
            raise ValueError(f"cos {tuple(rope[0].shape)} and sin {tuple(rope[1].shape)} disagree on P")
    for name, t in (("v_tail", v_tail),) + tuple(n[:2] for n in news) + ((("cos", rope[0]), ("sin", rope[1])) if rope is not None else ()):
        if t.device != dev:
            raise ValueError(f"k_pool is on {dev} but {name} on {t.device}")
    for name, t in (("k_pool", k_pool), ("k_pool_scales", k_pool_scales), ("vt_pool", vt_pool), ("vt_pool_scales", vt_pool_scales),
                    ("v_tail", v_tail)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: it is written in place")
    if B == 0:
        return None if q_new is None else tuple(k_pool.new_empty(q_new.shape[:3] + (n,)) for n in (d, -(-d // MX_BLOCK)))
    with torch.no_grad():
        k_new, v_new, q_new = (None if t is None else t.detach().contiguous() for t in (k_new, v_new, q_new))
        if not k_pool.is_cuda:
            return _append_paged_def(k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, v_tail, block_table, kv_len, k_new,
                                     v_new, q_new, rope, bool(interleaved))
        cos, sin = (None, None) if rope is None else (t.contiguous() for t in rope)
        return _hip.mx_kv_append_paged(k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, v_tail, block_table.contiguous(),
                                       kv_len.contiguous(), k_new, v_new, q_new, cos, sin, bool(interleaved))


def _append_ragged_paged_def(k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, v_tail, block_table, kv_len, cu_seqlens, k_new,
                             v_new, q_new, rope, interleaved):
    """the ragged append's definition (``include/qsparse_hip.h``, "MX KV cache append, ragged"): ``_append_paged_def`` once per sequence
    with ``T_b > 0``, on row ``b`` of ``block_table``, ``kv_len`` and ``v_tail`` and on its tokens permuted to head-major; q's codes go
    back token-major, rows that no sequence owns stay zero.  Reads ``cu_seqlens`` on the host"""
    Ttot, d = k_new.shape[0], k_new.shape[2]
    out = None if q_new is None else tuple(k_pool.new_zeros(q_new.shape[:2] + (n,)) for n in (d, -(-d // MX_BLOCK)))
    cu = [min(max(int(n), 0), Ttot) for n in cu_seqlens.tolist()]
    for b, (lo, hi) in enumerate(zip(cu[:-1], cu[1:])):
        if hi <= lo:
            continue
        k, v, q = (None if t is None else t[lo:hi].permute(1, 0, 2)[None].contiguous() for t in (k_new, v_new, q_new))
        got = _append_paged_def(k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, v_tail[b:b + 1], block_table[b:b + 1],
                                kv_len[b:b + 1], k, v, q, rope, interleaved)
        if got is not None:
            for dst, src in zip(out, got):
                dst[lo:hi] = src[0].permute(1, 0, 2)
    return out


def mx_kv_append_ragged_paged(k_pool: torch.Tensor, k_pool_scales: torch.Tensor, qk_fmt: str, vt_pool: torch.Tensor,
                              vt_pool_scales: torch.Tensor, v_fmt: str, v_tail: torch.Tensor, block_table: torch.Tensor, kv_len: torch.Tensor,
                              k_new: torch.Tensor, v_new: torch.Tensor, cu_seqlens: torch.Tensor, *, q_new: Optional[torch.Tensor] = None,
                              rope=None, interleaved: bool = False):
    """``mx_kv_append_paged`` for a RAGGED batch, in place and in ONE launch: sequence ``b`` appends ``T_b`` tokens, one, hundreds or
    none.  The new tokens are flat and token-major, as a QKV projection writes them -- ``k_new [Ttot, Hkv, d]``, ``v_new [Ttot, Hkv,
    dv]``, optional ``q_new [Ttot, Hq, d]`` -- and ``cu_seqlens`` (int32 ``[B + 1]`` on the operands' device, non-decreasing, ``cu[0] ==
    0``) says which sequence owns the tokens ``[cu[b], cu[b + 1])``.  The pool, ``v_tail``, ``block_table`` and ``kv_len`` are
    ``mx_kv_append_paged``'s; ``kv_len`` is the length BEFORE the append and is not changed.

    It IS ``mx_kv_append_paged`` called once per sequence with ``T_b > 0`` on row ``b`` of ``block_table``, ``kv_len`` and ``v_tail``
    (``_append_ragged_paged_def``), bit for bit on either device: ``v_tail``, the re-quantization of every touched 32-block of ``vt``
    from exact float32 values, dropping tokens at positions ``>= S``, the dead-entry guard and ``rope`` (table row ``min(L_b + t, P -
    1)``) hold per sequence.  A sequence with ``T_b == 0`` is untouched, its ``v_tail`` included.  ``Ttot`` may exceed ``cu[B]``: tokens
    at or behind ``cu[B]`` are stored nowhere.  ``q_new`` comes back as codes, token-major: ``(q_codes [Ttot, Hq, d], q_scales)``, the
    operands of ``mx_flash_prefill_ragged_paged``; their rows at or behind ``cu[B]`` are unspecified on the GPU and zero on the CPU.

    ``cu_seqlens``, ``kv_len`` and the table are read ON the device, never by the host: the call can be captured in a graph.  Every entry
    of ``cu_seqlens`` is clamped into ``[0, Ttot]`` and a negative length is 0; a malformed ``cu_seqlens`` gives an unspecified result,
    but no access leaves the operands.  Range: ``mx_kv_append_paged``'s (``1 <= d, dv <= 128``); anything else raises ``ValueError``
    naming the bound.  GPU tensors take ``qs_mx_kv_append_ragged_v`` (no fallback); there is no contiguous-cache form."""
    fn = "mx_kv_append_ragged_paged"
    _check_pool(fn, k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, block_table, kv_len)
    (P, Hkv, page, d), dv, (B, NP), dev = k_pool.shape, vt_pool.shape[2], block_table.shape, k_pool.device
    S = NP * page
    for name, n in (("d", d), ("dv", dv)):
        if not 1 <= n <= MX_KV_MAX_D:
            raise ValueError(f"{fn} takes 1 <= {name} <= {MX_KV_MAX_D}, got {name} = {n}")
    if not isinstance(v_tail, torch.Tensor) or v_tail.dtype != torch.float32 or tuple(v_tail.shape) != (B, Hkv, dv, MX_BLOCK):
        raise ValueError(f"v_tail must be a float32 tensor of shape {(B, Hkv, dv, MX_BLOCK)}, got "
                         + (f"{v_tail.dtype} {tuple(v_tail.shape)}" if isinstance(v_tail, torch.Tensor) else type(v_tail).__name__))
    _check_cu(fn, cu_seqlens, B, dev)
    news = (("k_new", k_new, Hkv, d), ("v_new", v_new, Hkv, dv)) + ((("q_new", q_new, None, d),) if q_new is not None else ())
    for name, t, heads, last in news:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        _check_dtype(name, t.dtype)
        if t.dim() != 3 or (heads is not None and t.shape[1] != heads) or t.shape[2] != last or t.shape[0] != k_new.shape[0]:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected ('Ttot', {'Hq' if heads is None else heads}, {last}) with k_new's Ttot")
        if t.dtype != k_new.dtype:
            raise ValueError(f"k_new is {k_new.dtype} but {name} {t.dtype}: the new tokens share one dtype")
    if q_new is not None and (q_new.shape[1] < 1 or q_new.shape[1] % Hkv):
        raise ValueError(f"Hq = {q_new.shape[1]} is no multiple of Hkv = {Hkv}: query head h uses key/value head h // (Hq / Hkv)")
    if rope is not None:
        if not isinstance(rope, (tuple, list)) or len(rope) != 2:
            raise TypeError("rope must be None or a 2-tuple (cos, sin)")
        if d % 2:
            raise ValueError(f"rope needs an even d (the last dimension of k_new), got {d}")
        for name, t in zip(("cos", "sin"), rope):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != d // 2 or t.shape[0] < S:
                raise ValueError(f"{name} must be a float32 tensor [P, d / 2] = [>= {S}, {d // 2}], got "
                                 + (f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__))
        if rope[0].shape != rope[1].shape:
            raise ValueError(f"cos {tuple(rope[0].shape)} and sin {tuple(rope[1].shape)} disagree on P")
    for name, t in (("v_tail", v_tail),) + tuple(n[:2] for n in news) + ((("cos", rope[0]), ("sin", rope[1])) if rope is not None else ()):
        if t.device != dev:
            raise ValueError(f"k_pool is on {dev} but {name} on {t.device}")
    for name, t in (("k_pool", k_pool), ("k_pool_scales", k_pool_scales), ("vt_pool", vt_pool), ("vt_pool_scales", vt_pool_scales),
                    ("v_tail", v_tail)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: it is written in place")
    if B == 0 or k_new.shape[0] == 0:
        return None if q_new is None else tuple(k_pool.new_zeros(q_new.shape[:2] + (n,)) for n in (d, -(-d // MX_BLOCK)))
    with torch.no_grad():
        k_new, v_new, q_new = (None if t is None else t.detach().contiguous() for t in (k_new, v_new, q_new))
        if not k_pool.is_cuda:
            return _append_ragged_paged_def(k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, v_tail, block_table, kv_len,
                                            cu_seqlens, k_new, v_new, q_new, rope, bool(interleaved))
        cos, sin = (None, None) if rope is None else (t.contiguous() for t in rope)
        return _hip.mx_kv_append_ragged(k_pool, k_pool_scales, qk_fmt, vt_pool, vt_pool_scales, v_fmt, v_tail, block_table.contiguous(),
                                        kv_len.contiguous(), cu_seqlens.contiguous(), k_new, v_new, q_new, cos, sin, bool(interleaved))


class MXPagedKVCache:
    """The buffers of a paged MX KV cache: the pool ``k_pool [P, Hkv, page, d]`` / ``k_pool_scales``, ``vt_pool [P, Hkv, dv, page]`` /
    ``vt_pool_scales``, and per sequence ``v_tail [B, Hkv, dv, 32]``, ``kv_len`` (int32 ``[B]``, zero) and ``block_table`` (int32 ``[B,
    NP]``, filled with ``-1``: the caller writes page numbers into it).  ``append`` is ``mx_kv_append_paged`` followed by ``kv_len +=
    T``; ``attend`` is ``mx_flash_decode_paged``.  ``append_ragged`` / ``prefill_ragged`` are the same pair for a batch whose sequences
    bring different numbers of tokens (flat token-major operands and ``cu_seqlens``).  All are graph-capturable; there is no allocator
    and no other logic."""

    def __init__(self, P: int, B: int, NP: int, Hkv: int, page: int, d: int, dv: int, qk_fmt: str = "mxfp8_e4m3",
                 v_fmt: str = "mxfp8_e4m3", device=None):
        _mx_format(qk_fmt), _mx_format(v_fmt)
        if page < MX_BLOCK or page & (page - 1):
            raise ValueError(f"MXPagedKVCache takes a page that is a power of two >= {MX_BLOCK}, got page = {page}")
        z = partial(torch.zeros, dtype=torch.uint8, device=device)
        self.qk_fmt, self.v_fmt = qk_fmt, v_fmt
        self.k_pool, self.k_pool_scales = z((P, Hkv, page, d)), z((P, Hkv, page, -(-d // MX_BLOCK)))
        self.vt_pool, self.vt_pool_scales = z((P, Hkv, dv, page)), z((P, Hkv, dv, page // MX_BLOCK))
        self.v_tail = torch.zeros((B, Hkv, dv, MX_BLOCK), dtype=torch.float32, device=device)
        self.kv_len = torch.zeros(B, dtype=torch.int32, device=device)
        self.block_table = torch.full((B, NP), -1, dtype=torch.int32, device=device)

    def append(self, k: torch.Tensor, v: torch.Tensor, q: Optional[torch.Tensor] = None, rope=None, interleaved: bool = False):
        out = mx_kv_append_paged(self.k_pool, self.k_pool_scales, self.qk_fmt, self.vt_pool, self.vt_pool_scales, self.v_fmt, self.v_tail,
                                 self.block_table, self.kv_len, k, v, q_new=q, rope=rope, interleaved=interleaved)
        self.kv_len += k.shape[2]
        return out

    def attend(self, q_codes: torch.Tensor, q_scales: torch.Tensor, **kw) -> torch.Tensor:
        """``mx_flash_decode_paged`` on the cache; keywords are forwarded, ``shared=(shared_table, shared_len)`` among them for a batch
        whose sequences begin with the same pages"""
        return mx_flash_decode_paged(q_codes, q_scales, self.qk_fmt, self.k_pool, self.k_pool_scales, self.vt_pool, self.vt_pool_scales,
                                     self.v_fmt, self.block_table, self.kv_len, **kw)

    def prefill(self, q_codes: torch.Tensor, q_scales: torch.Tensor, **kw) -> torch.Tensor:
        """``mx_flash_prefill_paged`` on the cache: any number of new tokens, behind the ``append`` that stored them"""
        return mx_flash_prefill_paged(q_codes, q_scales, self.qk_fmt, self.k_pool, self.k_pool_scales, self.vt_pool, self.vt_pool_scales,
                                      self.v_fmt, self.block_table, self.kv_len, **kw)

    def append_ragged(self, k: torch.Tensor, v: torch.Tensor, cu_seqlens: torch.Tensor, q: Optional[torch.Tensor] = None, rope=None,
                      interleaved: bool = False):
        """``mx_kv_append_ragged_paged`` followed by ``kv_len += cu_seqlens[1:] - cu_seqlens[:-1]``, a device op with no host read"""
        out = mx_kv_append_ragged_paged(self.k_pool, self.k_pool_scales, self.qk_fmt, self.vt_pool, self.vt_pool_scales, self.v_fmt,
                                        self.v_tail, self.block_table, self.kv_len, k, v, cu_seqlens, q_new=q, rope=rope,
                                        interleaved=interleaved)
        self.kv_len += cu_seqlens[1:] - cu_seqlens[:-1]
        return out

    def prefill_ragged(self, q_codes: torch.Tensor, q_scales: torch.Tensor, cu_seqlens: torch.Tensor, **kw) -> torch.Tensor:
        """``mx_flash_prefill_ragged_paged`` on the cache, behind the ``append_ragged`` that stored the tokens"""
        return mx_flash_prefill_ragged_paged(q_codes, q_scales, self.qk_fmt, self.k_pool, self.k_pool_scales, self.vt_pool,
                                             self.vt_pool_scales, self.v_fmt, self.block_table, self.kv_len, cu_seqlens, **kw)


__all__ = ["mx_kv_append", "MXKVCache", "mx_kv_append_paged", "MXPagedKVCache", "mx_kv_append_ragged_paged"]
