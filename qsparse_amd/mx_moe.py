"""The glue of a mixture-of-experts layer between its products on MX codes, as three calls: ``mx_moe_route`` (top-k selection, the
gates and the stable sort of the ``T k`` expert ids), ``mx_moe_dispatch_quantize`` (every token quantized ONCE and written to the ``k``
rows the sort gave it) and ``mx_moe_combine`` (every token's ``k`` expert rows times its gates, summed).  ``MXMoEFeedForward(...,
routing="fused")`` runs them in place of its chain of torch ops.

Each call has a definition function (``_route_def``, ``_dispatch_def``, ``_combine_def``; ``include/qsparse_hip.h``, "MX MoE routing" /
"dispatch" / "combine") that is also its CPU path.  The definitions are fixed float32 sequences, so GPU tensors -- which take the HIP
kernels ``qs_mx_moe_route_v``, ``qs_mx_moe_dispatch_v`` and ``qs_mx_moe_combine_v``, with no fallback -- give the same bits.  Nothing is
read by the host: all three can be captured in a graph."""
from typing import Optional

import torch

from qsparse_amd import _hip
from qsparse_amd._mx_common import MXActivation, _check_dtype, _check_operand
from qsparse_amd.mx_softmax import _exp_def
from qsparse_amd.quantize import MX_BLOCK, _mx_format, quantize_with_mx

MX_MOE_MAX_EXPERTS, MX_MOE_MAX_TOP_K = 1024, 32


def _route_def(logits: torch.Tensor, top_k: int):
    """the definition of ``mx_moe_route`` in torch ops: the CPU path, and what the GPU tests compare with"""
    (T, E), k, dev = logits.shape, top_k, logits.device
    x = logits.to(torch.float32)
    # the total order as one int64 key per element: the order-preserving image of the float (a NaN at the top, -0 as +0) in the high
    # bits, E - 1 - e below it: among equal values the LOWER index has the larger key, and no two keys of a row are equal
    x = torch.where(x == 0, torch.zeros_like(x), x)
    bits = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    image = torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000)
    image = torch.where(x != x, torch.full_like(image, 0xFFFFFFFF), image)
    key = image * 2048 + (E - 1 - torch.arange(E, device=dev))
    experts = torch.sort(key, -1, descending=True).indices[:, :k]
    top = torch.gather(x, 1, experts)
    e = _exp_def(top - top[:, :1])
    Z = torch.nn.functional.pad(e, (0, MX_MOE_MAX_TOP_K - k))     # the balanced tree over 32 slots, +0 behind slot k - 1
    while Z.shape[1] > 1:
        Z = Z[:, 0::2] + Z[:, 1::2]
    gates = e / Z
    gates = torch.where(gates != gates, torch.full_like(gates, float("nan")), gates)      # (the quiet NaN 0x7fc00000)
    ids = experts.reshape(-1)
    order = torch.argsort(ids, stable=True)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(T * k, device=dev)
    offs = (ids.unsqueeze(1) == torch.arange(E, device=dev)).sum(0).cumsum(0)
    return gates, experts.to(torch.int32), offs.to(torch.int32), order.to(torch.int32), inv.reshape(T, k).to(torch.int32)


def mx_moe_route(logits: torch.Tensor, top_k: int):
    """Top-``k`` routing of ``logits [T, E]`` (float32, bfloat16 or float16, widened exactly to float32; ``stride(1) == 1``).  Returns
    ``(gates, experts, offs, order, inv)``:

    * ``experts`` int32 ``[T, k]``: slot ``j`` of token ``t`` is the ``j``-th expert under a TOTAL order -- a NaN ranks before every
      number (``torch.topk``'s rule), otherwise the larger value first with ``-0 == +0``; equal values, and NaNs among themselves, go to
      the lower expert index (the tie rule torch leaves open);
    * ``gates`` float32 ``[T, k]``: the softmax over the kept logits as a fixed float32 sequence -- ``u_j = top_j - top_0``, ``e_j =
      E(u_j)`` with ``mx_softmax_quantize``'s written-out exponential, ``Z`` the balanced pairwise tree over 32 zero-padded slots (``(e_0 + e_1) + (e_2 + e_3)`` ...: its
      error grows with ``log2 k``, not with ``k``), ``e_j / Z``.  A kept NaN, or
      ``top_0 = +-inf``, makes the token's gates NaN; a kept ``-inf`` behind a finite ``top_0`` has gate 0;
    * ``order`` int32 ``[T k]``: the stable sort of the flat ids ``t k + j`` by expert; ``inv`` int32 ``[T, k]`` its inverse
      (``order[inv[t, j]] == t k + j``); ``offs`` int32 ``[E]`` the cumulative end of every expert, what ``mx_grouped_matmul`` takes.

    On logits without ties ``experts``, ``order`` and ``offs`` are ``torch.topk``, ``argsort(stable=True)`` and the comparison-sum of
    ``MXMoEFeedForward``'s default forward.  Range: ``1 <= E <= 1024``, ``1 <= top_k <= min(E, 32)``, ``T >= 0``, ``T k < 2^31``; anything
    else raises ``ValueError``.  GPU tensors take the HIP kernels (one launch for ``T <= 64``, else three; a deterministic counting sort
    without atomics; no fallback), CPU tensors ``_route_def``: the same bits."""
    if not isinstance(logits, torch.Tensor):
        raise TypeError(f"logits must be a tensor, got {type(logits).__name__}")
    _check_dtype("logits.dtype", logits.dtype)
    if logits.dim() != 2:
        raise ValueError(f"logits must be [T, E], got shape {tuple(logits.shape)}")
    T, E = logits.shape
    if not 1 <= E <= MX_MOE_MAX_EXPERTS:
        raise ValueError(f"mx_moe_route takes 1 <= E <= {MX_MOE_MAX_EXPERTS}, got E = {E}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= min(E, MX_MOE_MAX_TOP_K):
        raise ValueError(f"top_k must be an int in [1, min(E, {MX_MOE_MAX_TOP_K})] = [1, {min(E, MX_MOE_MAX_TOP_K)}], got {top_k!r}")
    if T * top_k >= 2 ** 31:
        raise ValueError(f"mx_moe_route takes T * top_k < 2^31, got {T} * {top_k}")
    if T > 1 and logits.stride(1) != 1 and E > 1:
        raise ValueError(f"logits must have stride(1) == 1, got strides {logits.stride()}")
    with torch.no_grad():
        logits = logits.detach()
        if not logits.is_cuda:
            return _route_def(logits, top_k)
        return _hip.mx_moe_route(logits, top_k)


def _valid_rows(inv: torch.Tensor, rows: int):
    flat = inv.reshape(-1).to(torch.int64)
    return flat, (flat >= 0) & (flat < rows)


def _dispatch_def(x, inv: torch.Tensor, fmt: str):
    """the definition of ``mx_moe_dispatch_quantize``: the CPU path (rows that no entry of ``inv`` names are zero here)"""
    T, k = inv.shape
    if isinstance(x, MXActivation):
        codes_t, scales_t = x.codes, x.scales
    elif x.numel():
        codes_t, scales_t = quantize_with_mx(x, fmt, -1, return_codes=True)[1:]
    else:
        codes_t, scales_t = (x.new_empty((T, n), dtype=torch.uint8) for n in (x.shape[1], -(-x.shape[1] // MX_BLOCK)))
    flat, ok = _valid_rows(inv, T * k)
    token = torch.arange(T, device=inv.device).repeat_interleave(k)
    codes, scales = (t.new_zeros((T * k, t.shape[1])) for t in (codes_t, scales_t))
    codes[flat[ok]], scales[flat[ok]] = codes_t[token[ok]], scales_t[token[ok]]
    return codes, scales


def _check_inv(inv, T: int, device):
    if not isinstance(inv, torch.Tensor) or inv.dtype != torch.int32 or inv.dim() != 2 or inv.shape[0] != T:
        raise ValueError(f"inv must be an int32 tensor [T, k] with T = {T}, got "
                         + (f"{inv.dtype} {tuple(inv.shape)}" if isinstance(inv, torch.Tensor) else type(inv).__name__))
    k = inv.shape[1]
    if not 1 <= k <= MX_MOE_MAX_TOP_K or T * k >= 2 ** 31:
        raise ValueError(f"inv [T, k] needs 1 <= k <= {MX_MOE_MAX_TOP_K} and T * k < 2^31, got shape {tuple(inv.shape)}")
    if inv.device != device:
        raise ValueError(f"the rows are on {device} but inv on {inv.device}")
    return k


def mx_moe_dispatch_quantize(x, inv: torch.Tensor, fmt: Optional[str] = None):
    """Quantize every row of ``x [T, D]`` (float32, bfloat16 or float16; ``stride(1) == 1``, rows may be strided) once and write it to
    the ``k`` rows ``inv[t, :]`` (int32 ``[T, k]``, as ``mx_moe_route`` returns it) of the expert-sorted buffer.  Returns ``(codes uint8
    [T k, D], scales uint8 [T k, ceil(D / 32)])``: rows ``inv[t, j]`` hold the bytes of ``quantize_with_mx(x[t], fmt, -1,
    return_codes=True)`` -- bit for bit what ``MXGroupedLinear`` computes from the ``k``-fold float copy of the rows, which never exists
    here.  Every format of ``MX_FORMATS``, rounding to nearest.

    ``x`` may be an ``MXActivation``: its codes and scale bytes are copied to the ``k`` rows, and ``fmt`` must be ``None`` or its format.
    An ``inv`` entry outside ``[0, T k)`` is not dereferenced and nothing is stored for it; rows that no entry names are UNSPECIFIED (as
    ``torch.empty`` gave them on the GPU).  GPU tensors take one HIP launch (``qs_mx_moe_dispatch_v``; no fallback)."""
    taken = isinstance(x, MXActivation)
    if taken:
        if fmt is not None and fmt != x.fmt:
            raise ValueError(f"fmt={fmt!r} but the MXActivation holds {x.fmt!r}: its bytes are copied, not converted")
        if x.channels_last:
            raise ValueError("mx_moe_dispatch_quantize got an MXActivation with channels_last=True: the codes of a convolution")
        _check_operand("x", x.codes, x.scales, x.fmt, what="[T, D]", least=2, most=2, needs="2 dimensions")
        fmt, rows = x.fmt, x.codes
    else:
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"x must be a tensor or an MXActivation, got {type(x).__name__}")
        if fmt is None:
            raise ValueError("fmt is needed for a float x")
        _mx_format(fmt)
        _check_dtype("x.dtype", x.dtype)
        if x.dim() != 2:
            raise ValueError(f"x must be [T, D], got shape {tuple(x.shape)}")
        if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
            x = x.contiguous()
        rows = x
    _check_inv(inv, rows.shape[0], rows.device)
    with torch.no_grad():
        inv = inv.contiguous()
        if not rows.is_cuda:
            return _dispatch_def(x if taken else x.detach(), inv, fmt)
        if taken:
            return _hip.mx_moe_dispatch(None, x.codes.contiguous(), x.scales.contiguous(), inv, fmt)
        return _hip.mx_moe_dispatch(x.detach(), None, None, inv, fmt)


def _combine_def(y: torch.Tensor, inv: torch.Tensor, gates: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """the definition of ``mx_moe_combine``: float32 products and sums one by one, ascending in ``j``; the CPU path"""
    (T, k), D = inv.shape, y.shape[1]
    flat, ok = _valid_rows(inv, T * k)
    y32 = torch.where(ok[:, None], y[flat.clamp(0, max(T * k - 1, 0))].to(torch.float32), torch.zeros((), device=y.device)).reshape(T, k, D)
    acc = gates[:, 0, None] * y32[:, 0]
    for j in range(1, k):
        acc = acc + gates[:, j, None] * y32[:, j]
    return acc.to(out_dtype)


def mx_moe_combine(y: torch.Tensor, inv: torch.Tensor, gates: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``out[t] = ((g_0 y_0) + (g_1 y_1)) + ...`` with ``y_j = y[inv[t, j]]`` and ``g_j = gates[t, j]``: ``y [T k, D]`` (float32,
    bfloat16 or float16) the expert-sorted rows, ``inv`` int32 ``[T, k]`` and ``gates`` float32 ``[T, k]`` as ``mx_moe_route`` returns
    them.  Every product and every sum is rounded to float32 on its own (no FMA), ascending in ``j``, with one final rounding to
    ``out_dtype``; returns ``[T, D]``.  An ``inv`` entry outside ``[0, T k)`` contributes its row as ``+0`` and is not dereferenced.  GPU
    tensors take one HIP launch (``qs_mx_moe_combine_v``: a token's ``k`` rows meet in registers, no atomics; no fallback)."""
    if not isinstance(y, torch.Tensor):
        raise TypeError(f"y must be a tensor, got {type(y).__name__}")
    _check_dtype("y.dtype", y.dtype)
    _check_dtype("out_dtype", out_dtype)
    if y.dim() != 2:
        raise ValueError(f"y must be [T k, D], got shape {tuple(y.shape)}")
    if not isinstance(inv, torch.Tensor) or inv.dim() != 2:
        raise ValueError("inv must be an int32 tensor [T, k]")
    k = _check_inv(inv, inv.shape[0], y.device)
    T = inv.shape[0]
    if y.shape[0] != T * k:
        raise ValueError(f"y has {y.shape[0]} rows, expected T k = {T * k} for inv {tuple(inv.shape)}")
    if not isinstance(gates, torch.Tensor) or gates.dtype != torch.float32 or tuple(gates.shape) != (T, k):
        raise ValueError(f"gates must be a float32 tensor of shape {(T, k)}")
    if gates.device != y.device:
        raise ValueError(f"y is on {y.device} but gates on {gates.device}")
    with torch.no_grad():
        y, inv, gates = y.detach().contiguous(), inv.contiguous(), gates.detach().contiguous()
        if not y.is_cuda:
            return _combine_def(y, inv, gates, out_dtype)
        return _hip.mx_moe_combine(y, inv, gates, out_dtype)


__all__ = ["mx_moe_route", "mx_moe_dispatch_quantize", "mx_moe_combine"]
