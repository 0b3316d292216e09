"""Training through batched matrix products on MX codes: ``mx_quantize_2way_batched``, ``mx_bmm_train``, ``mx_attention_train`` and the
layer ``MXTrainMultiheadAttention``.

``mx_linear`` trains a product whose second operand is a weight.  In attention BOTH operands of a product are activations with leading
dimensions (image, head), and all three products of a step -- forward, gradient of either operand -- are batched: ``mx_bmm`` computes
every one of them, what they need is each tensor as MX codes with blocks of 32 along its last axis and, transposed, along its
second-to-last one.  ``mx_quantize_2way_batched`` hands out both from one read of a ``[..., R, C]`` tensor (``qs_mx_quant2_batched_v``:
one launch for all slices, strided input read where it lies); ``mx_bmm_train`` is ``torch.bmm`` built on it, ``mx_attention_train`` two
of those around a float32 softmax.  The checks and the autograd scaffold are ``_mx_common.py``'s, shared with ``mx_linear`` and
``mx_conv2d_train``."""
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from qsparse_amd import _hip
from qsparse_amd._mx_common import _check_dtype, _check_train_entry, _MXTrainMixin, _quantize_grad, _save_train_ctx
from qsparse_amd.mx_bmm import MX_ATTENTION_SOFTMAX, MXMultiheadAttention, _attention_mask, mx_bmm
from qsparse_amd.mx_gemm import MXTrainLinear
from qsparse_amd.mx_softmax import mx_softmax_backward_quantize, mx_softmax_quantize
from qsparse_amd.quantize import MX_BLOCK, _mx_aten, _mx_check_rounding, _mx_format, _mx_sr_words

_LAYOUTS = ("nk", "kn")


def _slice_strides(x: torch.Tensor):
    """(G0, G1, (stride g0, stride g1, row stride)) in elements if the memory of `x` [..., R, C] is what qs_mx_quant2_batched_v
    addresses -- unit stride along C, rows that do not overlap, leading dimensions that collapse to at most two stride levels -- else
    None.  A dimension of extent 1 has no stride to speak of"""
    R, C = x.shape[-2:]
    if C > 1 and x.stride(-1) != 1:
        return None
    row = x.stride(-2) if R > 1 else C
    if row < C:
        return None
    levels = []                                        # (extent, stride), outermost first, adjacent levels merged where they are dense
    for n, s in zip(x.shape[:-2], x.stride()[:-2]):
        if n == 1:
            continue
        if levels and levels[-1][1] == n * s:
            levels[-1] = (levels[-1][0] * n, s)
        else:
            levels.append((n, s))
    if len(levels) > 2:
        return None
    levels = [(1, 0)] * (2 - len(levels)) + levels
    return levels[0][0], levels[1][0], (levels[0][1], levels[1][1], row)


def mx_quantize_2way_batched(x: torch.Tensor, row_fmt: Optional[str] = None, col_fmt: Optional[str] = None, rounding: str = "nearest",
                             seed: int = 0, step: Optional[torch.Tensor] = None):
    """``mx_quantize_2way`` for every slice of a float32 / bfloat16 / float16 tensor ``x [..., R, C]`` with at least 3 dimensions:
    returns ``(row_codes [..., R, C], row_scales [..., R, ceil(C / 32)], col_codes [..., C, R], col_scales [..., C, ceil(R / 32)])`` --
    the row pair is the codes and scales of ``quantize_with_mx(x, row_fmt, -1, return_codes=True)``, the col pair those of
    ``quantize_with_mx(x.transpose(-1, -2).contiguous(), col_fmt, -1, return_codes=True)``, bit for bit; slice by slice both are
    ``mx_quantize_2way`` of the slice.  A pair whose format is ``None`` is not computed and comes back as ``(None, None)``; at least one
    format must be given.  The outputs are contiguous and never differentiable.

    GPU tensors take the HIP kernel (``qs_mx_quant2_batched_v``; no fallback): ONE launch that reads every slice once.  ``x`` is read
    where it lies when its last stride is 1 and its leading dimensions collapse to at most two stride levels -- a ``[B, T, h,
    d].transpose(1, 2)``, a ``chunk`` of a packed projection -- and through ``contiguous()`` otherwise.  CPU tensors evaluate the
    definition.

    ``rounding="stochastic"`` (``seed``, ``step`` as in ``quantize_with_mx``): the row pair is the stochastic one-way quantizer on ``x``
    with ``stream=0``, the col pair the one on ``x.transpose(-1, -2).contiguous()`` with ``stream=1``: a code's random word is indexed by
    its row-major position in the whole output it belongs to."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a tensor, got {type(x).__name__}")
    if x.dim() == 2:
        raise ValueError(f"mx_quantize_2way_batched needs [..., R, C] with at least one leading dimension, got shape {tuple(x.shape)}: "
                         "a 2-d tensor is mx_quantize_2way")
    if x.dim() < 3:
        raise ValueError(f"mx_quantize_2way_batched needs at least 3 dimensions [..., R, C], got shape {tuple(x.shape)}")
    _check_dtype("x", x.dtype)
    if row_fmt is None and col_fmt is None:
        raise ValueError("mx_quantize_2way_batched needs row_fmt, col_fmt or both")
    for fmt in (row_fmt, col_fmt):
        if fmt is not None:
            _mx_format(fmt)
    _mx_check_rounding(rounding, step, x)
    x = x.detach()
    lead, (R, C) = tuple(x.shape[:-2]), x.shape[-2:]
    nb = lambda n: (n + MX_BLOCK - 1) // MX_BLOCK
    shapes = (lead + (R, C), lead + (R, nb(C)), lead + (C, R), lead + (C, nb(R)))
    if x.is_cuda:
        plan = _slice_strides(x)
        if plan is None:
            x = x.contiguous()
            plan = _slice_strides(x)
        out = _hip.mx_quant2_batched(x, plan[0], plan[1], R, C, plan[2], row_fmt, col_fmt, rounding, seed, step)
        return tuple(None if t is None else t.view(shape) for t, shape in zip(out, shapes))
    if x.numel() == 0:                                 # (the CPU quantizer takes no empty tensor)
        return tuple(None if fmt is None else x.new_empty(shape, dtype=torch.uint8)
                     for shape, fmt in zip(shapes, (row_fmt, row_fmt, col_fmt, col_fmt)))
    sr = rounding == "stochastic"
    rc = rs = cc = cs = None
    last = x.dim() - 1
    if row_fmt is not None:
        _, rc, rs = _mx_aten(x, row_fmt, last, torch.float32, True, _mx_sr_words(x.shape, seed, step, 0) if sr else None)
        rc, rs = rc.contiguous(), rs.contiguous()
    if col_fmt is not None:
        xt = x.transpose(-1, -2)
        _, cc, cs = _mx_aten(xt, col_fmt, last, torch.float32, True, _mx_sr_words(xt.shape, seed, step, 1) if sr else None)
        cc, cs = cc.contiguous(), cs.contiguous()
    return rc, rs, cc, cs


class _MXBmmFunction(torch.autograd.Function):
    """the table of `mx_bmm_train` on MX codes; every quantizer straight-through.  `need_da` / `need_db`: that gradient can be asked
    for -- decided by mx_bmm_train, where the grad mode is still the caller's (as mx_linear's `need_col`)"""

    @staticmethod
    def forward(ctx, a, b, bias, kn, a_fmt, b_fmt, grad_fmt, out_dtype, need_da, need_db, grad_rounding, seed, step):
        a_row, a_rs, a_col, a_cs = mx_quantize_2way_batched(a, a_fmt, a_fmt if need_db else None)
        # b with blocks along K for the forward, with blocks along N for da: the row and the col pair of [N, K], the reverse of [K, N]
        if kn:
            b_n, b_ns, b_k, b_ks = mx_quantize_2way_batched(b, b_fmt if need_da else None, b_fmt)
        else:
            b_k, b_ks, b_n, b_ns = mx_quantize_2way_batched(b, b_fmt, b_fmt if need_da else None)
        b32 = None if bias is None else bias.detach().to(torch.float32)
        y = mx_bmm(a_row, a_rs, a_fmt, b_k, b_ks, b_fmt, b32, out_dtype)
        # both operands as the codes their gradient products multiply: 1 + 1/32 bytes per element (None where nobody asks)
        ctx.save_for_backward(a_col, a_cs, b_n, b_ns)
        _save_train_ctx(ctx, (a_fmt, b_fmt, grad_fmt), (grad_rounding, seed, step), None, a, bias)
        ctx.kn, ctx.b_dtype, ctx.bias_dim = kn, b.dtype, None if bias is None else bias.dim()
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        a_col, a_cs, b_n, b_ns = ctx.saved_tensors
        a_fmt, b_fmt, grad_fmt = ctx.fmts
        need_da, need_db, need_bias = ctx.needs_input_grad[:3]
        need_da, need_db = need_da and b_n is not None, need_db and a_col is not None
        da = db = dbias = None
        if need_da or need_db:
            g_row, g_rs, g_col, g_cs = _quantize_grad(ctx, lambda *sr: mx_quantize_2way_batched(dy, grad_fmt if need_da else None,
                                                                                                 grad_fmt if need_db else None, *sr))
        if need_da:
            da = mx_bmm(g_row, g_rs, grad_fmt, b_n, b_ns, b_fmt, None, ctx.x_dtype)
        if need_db and ctx.kn:
            db = mx_bmm(a_col, a_cs, a_fmt, g_col, g_cs, grad_fmt, None, ctx.b_dtype)
        elif need_db:
            db = mx_bmm(g_col, g_cs, grad_fmt, a_col, a_cs, a_fmt, None, ctx.b_dtype)
        if need_bias:
            dbias = dy.sum(-2, dtype=torch.float32)
            if ctx.bias_dim == 1:
                dbias = dbias.reshape(-1, dbias.shape[-1]).sum(0)
            dbias = dbias.to(ctx.bias_dtype)
        return da, db, dbias, None, None, None, None, None, None, None, None, None, None


def mx_bmm_train(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None, *, b_layout: str = "nk",
                 a_fmt: str = "mxfp8_e4m3", b_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", out_dtype: Optional[torch.dtype] = None,
                 grad_rounding: str = "nearest", seed: int = 0, step: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``torch.bmm`` whose three batched products run on MX codes (``mx_bmm``), differentiable in ``a``, ``b`` and ``bias``.  ``a`` is
    ``[..., M, K]``, ``b`` is ``[..., N, K]`` (``b_layout="nk"``: the result is ``a b^T``) or ``[..., K, N]`` (``"kn"``: ``a b``) with
    the leading dimensions of ``a`` (at least one; nothing is broadcast), both float32 / bfloat16 / float16 and not necessarily the
    same; ``bias`` is ``[N]`` (shared by the slices) or ``[..., N]``.  The result is ``[..., M, N]`` in ``out_dtype``, by default
    ``a.dtype``.  With ``Q(t)`` the MX codes of ``t`` with blocks of 32 along its LAST axis, in ``a_fmt`` / ``b_fmt`` for the operands
    and ``grad_fmt`` for the incoming gradient ``dy``, per slice:

                  "nk"                                    "kn"
        y     =   Q(a) Q(b)^T + bias                      Q(a) Q(b^T)^T + bias
        da    =   Q(dy) Q(b^T)^T                          Q(dy) Q(b)^T
        db    =   Q(dy^T) Q(a^T)^T      [N, K]            Q(a^T) Q(dy^T)^T      [K, N]
        dbias =   sum of dy over M in float32 (and over the slices for a shared ``[N]`` bias)

    -- the straight-through rule of ``quantize_with_mx`` at every quantizer, as ``mx_linear``.  ``Q(t)`` and ``Q(t^T)`` are the row and
    the col pair of ONE ``mx_quantize_2way_batched(t)``: the forward calls it once on ``a`` and once on ``b`` and keeps, as codes, the
    pairs the backward multiplies; the backward calls it once on ``dy``.  A pair nobody needs is not computed (no col pair of ``a``
    unless ``b`` requires grad; nothing is kept under ``torch.no_grad()``), a gradient nobody asks for is ``None``.  No operand is
    transposed in memory, and a strided one (``mx_quantize_2way_batched``) is not copied.  GPU tensors run HIP kernels only, without a
    host synchronisation (a step can be graph-captured); CPU tensors evaluate the same formulas on ``mx_bmm``'s CPU path.

    ``grad_rounding="stochastic"`` rounds the two forms of ``dy`` and nothing else stochastically (``seed``, ``step`` as in
    ``mx_linear``); ``step`` is advanced by one in place after a backward that quantizes ``dy``."""
    if b_layout not in _LAYOUTS:
        raise ValueError(f"unknown b_layout {b_layout!r}: one of {_LAYOUTS}")
    _check_train_entry(a, b, bias, (a_fmt, b_fmt, grad_fmt), grad_rounding, step, None, names=("a", "b"))
    out_dtype = a.dtype if out_dtype is None else out_dtype
    _check_dtype("out_dtype", out_dtype)
    kn = b_layout == "kn"
    if a.dim() < 3 or b.dim() < 3:
        raise ValueError(f"a needs [..., M, K] and b [..., {'K, N' if kn else 'N, K'}] with at least 3 dimensions, got shapes "
                         f"{tuple(a.shape)} and {tuple(b.shape)}: one weight [N, K] for every row of a is mx_linear")
    lead = tuple(a.shape[:-2])
    if tuple(b.shape[:-2]) != lead:
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} disagree on their leading dimensions (nothing is broadcast)")
    (M, K), (N, Kb) = a.shape[-2:], (b.shape[-2:][::-1] if kn else b.shape[-2:])
    if Kb != K:
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} disagree on K with b_layout={b_layout!r}")
    if min(M, N, K) < 1:
        raise ValueError("mx_bmm_train needs M, N, K >= 1: each is the contraction length of one of the three products")
    if bias is not None and tuple(bias.shape) not in ((N,), lead + (N,)):
        raise ValueError(f"bias has shape {tuple(bias.shape)}, expected ({N},) or {lead + (N,)}")
    grad = torch.is_grad_enabled()
    return _MXBmmFunction.apply(a, b, bias, kn, a_fmt, b_fmt, grad_fmt, out_dtype, grad and a.requires_grad, grad and b.requires_grad,
                                grad_rounding, seed, step)


class _MXFusedAttentionFunction(torch.autograd.Function):
    """the table of `mx_attention_train(softmax="fused")` on MX codes: ONE function over (q, k, v), because ds has to reach the dq / dk
    products as codes.  `need_q` / `need_k` / `need_v`: that gradient can be asked for -- decided by mx_attention_train, where the
    grad mode is still the caller's"""

    @staticmethod
    def forward(ctx, q, k, v, attn_mask, is_causal, scale, qk_fmt, p_fmt, v_fmt, grad_fmt, need_q, need_k, need_v, grad_rounding, seed,
                step, rope, rope_interleaved):
        need_ds = need_q or need_k
        if rope is None:
            q_row, q_rs, q_col, q_cs = mx_quantize_2way_batched(q, qk_fmt, qk_fmt if need_k else None)
            k_row, k_rs, k_col, k_cs = mx_quantize_2way_batched(k, qk_fmt, qk_fmt if need_q else None)
        else:
            from qsparse_amd.mx_rope import mx_rope_quantize       # (it imports this module)
            q_row, q_rs, q_col, q_cs = mx_rope_quantize(q, rope[0], rope[1], row_fmt=qk_fmt, col_fmt=qk_fmt if need_k else None,
                                                        interleaved=rope_interleaved)
            k_row, k_rs, k_col, k_cs = mx_rope_quantize(k, rope[2], rope[3], row_fmt=qk_fmt, col_fmt=qk_fmt if need_q else None,
                                                        interleaved=rope_interleaved)
        s = mx_bmm(q_row, q_rs, qk_fmt, k_row, k_rs, qk_fmt)
        p = mx_softmax_quantize(s, attn_mask, scale=scale, is_causal=is_causal, fmt=p_fmt, col_fmt=p_fmt if need_v else None,
                                return_stats=True)
        p_col, p_cs = p[2:4] if need_v else (None, None)
        m, Z = p[-2:]
        # v [.., S, dv] as the "kn" layout takes it: the col pair (blocks along S) for the forward, the row pair (along dv) for dp
        v_n, v_ns, v_k, v_ks = mx_quantize_2way_batched(v, v_fmt if need_ds else None, v_fmt)
        o = mx_bmm(p[0], p[1], p_fmt, v_k, v_ks, v_fmt, None, q.dtype)
        if need_ds or need_v:       # s, the row statistics and the code pairs the backward multiplies (None where nobody asks)
            ctx.save_for_backward(s if need_ds else None, m if need_ds else None, Z if need_ds else None, q_col, q_cs, k_col, k_cs, p_col,
                                  p_cs, v_n, v_ns)
        ctx.fmts, ctx.sr = (qk_fmt, p_fmt, v_fmt, grad_fmt), (grad_rounding, seed, step)
        ctx.mask, ctx.is_causal, ctx.scale = attn_mask, is_causal, scale          # (the mask is held by reference)
        ctx.dtypes = (q.dtype, k.dtype, v.dtype)
        ctx.rope, ctx.rope_interleaved = rope, rope_interleaved                   # (the tables are held by reference)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, do):
        s, m, Z, q_col, q_cs, k_col, k_cs, p_col, p_cs, v_n, v_ns = ctx.saved_tensors
        qk_fmt, p_fmt, v_fmt, grad_fmt = ctx.fmts
        rounding, seed, step = ctx.sr
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        need_q, need_k, need_v = need_q and k_col is not None, need_k and q_col is not None, need_v and p_col is not None
        need_ds = need_q or need_k
        dq = dk = dv = None
        if need_ds or need_v:
            g_row, g_rs, g_col, g_cs = _quantize_grad(ctx, lambda *sr: mx_quantize_2way_batched(do, grad_fmt if need_ds else None,
                                                                                                 grad_fmt if need_v else None, *sr))
        if need_v:
            dv = mx_bmm(p_col, p_cs, p_fmt, g_col, g_cs, grad_fmt, None, ctx.dtypes[2])
        if need_ds:
            dp = mx_bmm(g_row, g_rs, grad_fmt, v_n, v_ns, v_fmt)
            ds_row, ds_rs, ds_col, ds_cs = mx_softmax_backward_quantize(
                dp, s, m, Z, ctx.mask, scale=ctx.scale, is_causal=ctx.is_causal, row_fmt=grad_fmt if need_q else None,
                col_fmt=grad_fmt if need_k else None, rounding=rounding, seed=seed + 1, step=step)
            if rounding == "stochastic" and step is not None:
                step.add_(1)
        rope = ctx.rope
        if need_q:
            dq = mx_bmm(ds_row, ds_rs, grad_fmt, k_col, k_cs, qk_fmt, None, ctx.dtypes[0] if rope is None else torch.float32)
        if need_k:
            dk = mx_bmm(ds_col, ds_cs, grad_fmt, q_col, q_cs, qk_fmt, None, ctx.dtypes[1] if rope is None else torch.float32)
        if rope is not None:        # the products gave the gradients of the ROTATED q and k, in float32: back through the rotation
            from qsparse_amd.mx_rope import mx_rope
            if need_q:
                dq = mx_rope(dq, rope[0], rope[1], interleaved=ctx.rope_interleaved, inverse=True, out_dtype=ctx.dtypes[0])
            if need_k:
                dk = mx_rope(dk, rope[2], rope[3], interleaved=ctx.rope_interleaved, inverse=True, out_dtype=ctx.dtypes[1])
        return (dq, dk, dv) + (None,) * 15


def mx_attention_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor] = None,
                       is_causal: bool = False, scale: Optional[float] = None, *, qk_fmt: str = "mxfp8_e4m3", p_fmt: str = "mxfp8_e4m3",
                       v_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest", seed: int = 0,
                       step: Optional[torch.Tensor] = None, softmax: str = "torch", rope=None,
                       rope_interleaved: bool = False) -> torch.Tensor:
    """Scaled dot-product attention that TRAINS through its two matrix products on MX codes.  ``q [..., T, d]``, ``k [..., S, d]``,
    ``v [..., S, dv]`` as ``mx_attention`` takes them; the result is ``[..., T, dv]`` in ``q.dtype``.  It is DEFINED as this composition
    of public differentiable calls and is bit for bit that composition, forward and backward, on either device:

        1. ``s = mx_bmm_train(q, k, a_fmt=qk_fmt, b_fmt=qk_fmt, out_dtype=torch.float32, seed=seed + 1, ...)``
        2. ``s = s * scale`` (``d ** -0.5`` by default), then ``s = s + mask`` by ``mx_attention``'s mask rules
        3. ``p = torch.softmax(s, -1)`` in float32
        4. ``o = mx_bmm_train(p, v, b_layout="kn", a_fmt=p_fmt, b_fmt=v_fmt, out_dtype=q.dtype, seed=seed, ...)``

    with ``grad_fmt``, ``grad_rounding`` and ``step`` handed to both.  Autograd supplies the softmax backward on the float32 ``p``
    (which it keeps: 4 bytes per element); ``v`` is never transposed in memory -- the ``"kn"`` forward multiplies its col pair, blocks
    along ``S``.  A stochastic step advances ``step`` by two.  The forward value is bit for bit ``mx_attention(q, k, v, ...,
    out_dtype=q.dtype)``.  No dropout.

    ``softmax="fused"`` (keyword; the default ``"torch"`` is the composition above, bit for bit as it always was) is ONE autograd
    function over ``(q, k, v)`` in which no float ``p`` and no float ``ds`` ever exists.  It is DEFINED as this composition of public
    calls, with ``Q2`` = ``mx_quantize_2way_batched``, and equals it bit for bit on either device.  Forward:

        1. ``Q2(q, qk_fmt, qk_fmt)`` and ``Q2(k, qk_fmt, qk_fmt)``: the row pairs (blocks along ``d``) for the forward, the col pairs
           (along ``T`` / ``S``) for ``dk`` / ``dq`` -- a col pair only where the OTHER operand requires grad
        2. ``s = mx_bmm(q_row, k_row)`` in float32
        3. ``p_row, [p_col,] m, Z = mx_softmax_quantize(s, attn_mask, scale=scale, is_causal=is_causal, fmt=p_fmt, col_fmt=p_fmt if v
           requires grad else None, return_stats=True)``
        4. ``Q2(v, v_fmt, v_fmt)``: the col pair (blocks along ``S``) for the forward, the row pair (along ``dv``) for ``dp`` where
           ``q`` or ``k`` requires grad; ``v`` is never transposed in memory
        5. ``o = mx_bmm(p_row, v_col)`` to ``q.dtype``: bit for bit ``mx_attention(..., softmax="fused", out_dtype=q.dtype)``

    It keeps ``s``, ``m``, ``Z`` and the code pairs the backward multiplies; the mask is held by reference.  Backward, from ``dO``:

        6. ``Q2(dO, grad_fmt, grad_fmt, grad_rounding, seed, step)``
        7. ``dv = mx_bmm(p_col, dO_col)`` to ``v.dtype``;  ``dp = mx_bmm(dO_row, v_row)`` in float32
        8. ``ds_row, ds_col = mx_softmax_backward_quantize(dp, s, m, Z, attn_mask, scale=scale, is_causal=is_causal, row_fmt=grad_fmt,
           col_fmt=grad_fmt, rounding=grad_rounding, seed=seed + 1, step=step)`` -- with the ``step`` that 6. has advanced
        9. ``dq = mx_bmm(ds_row, k_col)`` to ``q.dtype``;  ``dk = mx_bmm(ds_col, q_col)`` to ``k.dtype``

    Pairs and gradients nobody asks for are not computed (only ``dv``: no call 8., no col pairs of ``q`` / ``k``).  A stochastic step
    advances ``step`` by one after 6. and by one after 8.: by two.  ``attn_mask`` gets no gradient, and a floating one that requires
    grad is refused.

    ``rope`` / ``rope_interleaved`` (keywords; ``None`` changes no call, launch or bit) are ``mx_attention``'s: a 2-tuple ``(cos,
    sin)`` (needs ``T == S``) or a 4-tuple ``(cos_q, sin_q, cos_k, sin_k)`` of ``mx_rope`` tables.  With ``softmax="torch"`` the call
    is DEFINED as the first composition above on ``mx_rope(q, cos_q, sin_q, interleaved=rope_interleaved, out_dtype=torch.float32)``
    and ``mx_rope(k, cos_k, sin_k, ...)`` -- differentiable calls, nothing is fused -- with the result still in ``q.dtype``.  With
    ``softmax="fused"`` it is the second composition with these steps replaced, ``RQ`` = ``mx_rope_quantize``:

        1. ``RQ(q, cos_q, sin_q, row_fmt=qk_fmt, col_fmt=qk_fmt, interleaved=rope_interleaved)`` and ``RQ(k, cos_k, sin_k, ...)`` -- a
           col pair only where the OTHER operand requires grad, as before; the rotated ``q`` / ``k`` are never written
        9. ``dq_rot = mx_bmm(ds_row, k_col)`` and ``dk_rot = mx_bmm(ds_col, q_col)`` **to float32**, then ``dq = mx_rope(dq_rot, cos_q,
           sin_q, interleaved=rope_interleaved, inverse=True, out_dtype=q.dtype)`` and ``dk = mx_rope(dk_rot, cos_k, sin_k, ...,
           inverse=True, out_dtype=k.dtype)``: one rounding to the input's dtype, as the ``"torch"`` composition gives

    The tables get no gradient; one that requires grad is refused."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dim() < 3:
            raise ValueError(f"{name} needs at least 3 dimensions [..., {'T' if name == 'q' else 'S'}, d], got shape {tuple(t.shape)}")
    if k.shape[-2] != v.shape[-2]:
        raise ValueError(f"k {tuple(k.shape)} and v {tuple(v.shape)} disagree on S (their second-to-last dimensions)")
    if softmax not in MX_ATTENTION_SOFTMAX:
        raise ValueError(f"unknown softmax {softmax!r}: one of {MX_ATTENTION_SOFTMAX}")
    out_dtype = q.dtype
    if rope is not None:
        from qsparse_amd.mx_rope import _attention_rope, mx_rope       # (it imports this module)
        if k.shape[-1] != q.shape[-1]:
            raise ValueError(f"q {tuple(q.shape)} and k {tuple(k.shape)} disagree on d (their last dimensions)")
        rope = _attention_rope(rope, q.shape[-2], k.shape[-2], q.shape[-1], q.device)
    if softmax == "fused":
        return _attention_train_fused(q, k, v, attn_mask, is_causal, scale, qk_fmt, p_fmt, v_fmt, grad_fmt, grad_rounding, seed, step,
                                      rope, bool(rope_interleaved))
    if rope is not None:
        q = mx_rope(q, rope[0], rope[1], interleaved=rope_interleaved, out_dtype=torch.float32)
        k = mx_rope(k, rope[2], rope[3], interleaved=rope_interleaved, out_dtype=torch.float32)
    mask = _attention_mask(attn_mask, is_causal, q.shape[-2], k.shape[-2], q.device)
    sr = dict(grad_fmt=grad_fmt, grad_rounding=grad_rounding, step=step)
    s = mx_bmm_train(q, k, a_fmt=qk_fmt, b_fmt=qk_fmt, out_dtype=torch.float32, seed=seed + 1, **sr)
    s = s * (q.shape[-1] ** -0.5 if scale is None else scale)
    if mask is not None:
        s = s + mask
    return mx_bmm_train(torch.softmax(s, -1), v, b_layout="kn", a_fmt=p_fmt, b_fmt=v_fmt, out_dtype=out_dtype, seed=seed, **sr)


def _attention_train_fused(q, k, v, attn_mask, is_causal, scale, qk_fmt, p_fmt, v_fmt, grad_fmt, grad_rounding, seed, step, rope=None,
                           rope_interleaved=False):
    """the checks of `mx_attention_train(softmax="fused")` beyond the shared ones, then the autograd function"""
    for name, t in (("q", q), ("k", k), ("v", v)):
        _check_dtype(name, t.dtype)
        if t.device != q.device:
            raise ValueError(f"q is on {q.device} but {name} on {t.device}")
    for fmt in (qk_fmt, p_fmt, v_fmt, grad_fmt):
        _mx_format(fmt)
    _mx_check_rounding(grad_rounding, step, q)
    lead, d = tuple(q.shape[:-2]), q.shape[-1]
    if tuple(k.shape[:-2]) != lead or tuple(v.shape[:-2]) != lead:
        raise ValueError(f"q {tuple(q.shape)}, k {tuple(k.shape)} and v {tuple(v.shape)} disagree on their leading dimensions (nothing "
                         "is broadcast)")
    if k.shape[-1] != d:
        raise ValueError(f"q {tuple(q.shape)} and k {tuple(k.shape)} disagree on d (their last dimensions)")
    if min(q.shape[-2], k.shape[-2], d, v.shape[-1]) < 1:
        raise ValueError("mx_attention_train needs T, S, d, dv >= 1: each is the contraction length of one of its products")
    if attn_mask is not None and is_causal:
        raise ValueError("give attn_mask or is_causal, not both")
    if scale is not None and (isinstance(scale, bool) or not isinstance(scale, (int, float))):
        raise TypeError(f"scale must be a float, got {type(scale).__name__}")
    grad = torch.is_grad_enabled()
    if isinstance(attn_mask, torch.Tensor) and grad and attn_mask.requires_grad:
        raise RuntimeError('mx_attention_train(softmax="fused") has no gradient for attn_mask: a mask that requires grad is refused')
    _attention_mask(attn_mask, False, q.shape[-2], k.shape[-2], q.device)       # (its checks, where the caller can still read them)
    return _MXFusedAttentionFunction.apply(q, k, v, attn_mask, bool(is_causal), float(d ** -0.5 if scale is None else scale), qk_fmt,
                                           p_fmt, v_fmt, grad_fmt, grad and q.requires_grad, grad and k.requires_grad,
                                           grad and v.requires_grad, grad_rounding, seed, step, rope, rope_interleaved)


class MXTrainMultiheadAttention(_MXTrainMixin, nn.Module):
    """A self-attention ``nn.MultiheadAttention`` that trains on MX codes throughout: two ``MXTrainLinear`` s -- the packed ``in_proj``
    ``[3 E, E]`` and ``out_proj`` ``[E, E]`` -- around ``mx_attention_train`` over ``[B, h, T, d]``.  ``forward(x, attn_mask=None,
    is_causal=False)`` takes ``x`` ``[T, B, E]`` (``[B, T, E]`` with ``batch_first``) and returns ``(output, None)``.  ``q``, ``k`` and
    ``v`` are strided views of the packed projection's output -- the quantizer reads the heads where they lie, nothing is copied.  It
    refuses what ``MXMultiheadAttention`` refuses (``need_weights``, ``key_padding_mask``; ``kdim`` / ``vdim``, ``add_bias_kv``,
    ``add_zero_attn`` in ``from_float``) and attention dropout, which it does not have.

    ``grad_rounding="stochastic"`` goes to both linear layers (each with a counter of its own, ``MXTrainLinear``) and to the attention,
    for which the layer owns ``sr_seed`` and a non-persistent int64 buffer ``sr_step`` that a step advances by two.  ``softmax``
    (``"torch"`` or ``"fused"``) is ``mx_attention_train``'s keyword; ``to_inference()`` hands it on, so a fused training layer converts
    to an ``MXMultiheadAttention`` with the same forward bits.  ``forward``'s ``rope`` / ``rope_interleaved`` are
    ``mx_attention_train``'s: call arguments, not state, so ``to_inference()`` has nothing to carry."""

    def __init__(self, in_proj: MXTrainLinear, out_proj: MXTrainLinear, num_heads: int, batch_first: bool = False, *,
                 qk_fmt: str = "mxfp8_e4m3", p_fmt: str = "mxfp8_e4m3", v_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2",
                 grad_rounding: str = "nearest", seed: Optional[int] = None, softmax: str = "torch"):
        super().__init__()
        if not isinstance(in_proj, MXTrainLinear) or not isinstance(out_proj, MXTrainLinear):
            raise TypeError("in_proj and out_proj must be MXTrainLinear layers")
        E = out_proj.in_features
        if in_proj.in_features != E or in_proj.out_features != 3 * E or out_proj.out_features != E:
            raise ValueError(f"in_proj must be [3 E, E] and out_proj [E, E], got [{in_proj.out_features}, {in_proj.in_features}] and "
                             f"[{out_proj.out_features}, {out_proj.in_features}]")
        if isinstance(num_heads, bool) or not isinstance(num_heads, int) or num_heads < 1 or E % num_heads:
            raise ValueError(f"num_heads must be an int >= 1 that divides embed_dim {E}, got {num_heads!r}")
        if softmax not in MX_ATTENTION_SOFTMAX:
            raise ValueError(f"unknown softmax {softmax!r}: one of {MX_ATTENTION_SOFTMAX}")
        self._init_mx(dict(qk_fmt=qk_fmt, p_fmt=p_fmt, v_fmt=v_fmt, grad_fmt=grad_fmt), grad_rounding, seed, in_proj.weight)
        self.softmax = softmax
        self.in_proj, self.out_proj = in_proj, out_proj
        self.embed_dim, self.num_heads, self.batch_first = E, num_heads, bool(batch_first)

    def extra_repr(self) -> str:
        sr = f", grad_rounding={self.grad_rounding!r}" if self.grad_rounding != "nearest" else ""
        sm = f", softmax={self.softmax!r}" if self.softmax != "torch" else ""
        return (f"embed_dim={self.embed_dim}, num_heads={self.num_heads}, batch_first={self.batch_first}, qk_fmt={self.qk_fmt!r}, "
                f"p_fmt={self.p_fmt!r}, v_fmt={self.v_fmt!r}, grad_fmt={self.grad_fmt!r}{sr}{sm}")

    @classmethod
    def from_float(cls, mha: nn.MultiheadAttention, x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", *,
                   qk_fmt: str = "mxfp8_e4m3", p_fmt: str = "mxfp8_e4m3", v_fmt: str = "mxfp8_e4m3", grad_rounding: str = "nearest",
                   seed: Optional[int] = None, softmax: str = "torch"):
        """a layer on ``mha``'s own parameters (shared, not copied): ``in_proj_weight`` / ``in_proj_bias`` and ``out_proj``'s"""
        if not isinstance(mha, nn.MultiheadAttention):
            raise TypeError(f"MXTrainMultiheadAttention.from_float needs an nn.MultiheadAttention, got {type(mha).__name__}")
        if not mha._qkv_same_embed_dim:
            raise ValueError("kdim / vdim other than embed_dim are not supported: MXTrainMultiheadAttention is self-attention on one packed "
                             "in_proj")
        if mha.bias_k is not None or mha.bias_v is not None:
            raise ValueError("add_bias_kv=True is not supported")
        if mha.add_zero_attn:
            raise ValueError("add_zero_attn=True is not supported")
        if mha.dropout:
            raise ValueError(f"dropout={mha.dropout} is not supported: mx_attention_train has no dropout")
        E = mha.embed_dim
        opts = dict(x_fmt=x_fmt, w_fmt=w_fmt, grad_fmt=grad_fmt, grad_rounding=grad_rounding)
        packed = SimpleNamespace(weight=mha.in_proj_weight, bias=mha.in_proj_bias, training=mha.training)
        in_proj = MXTrainLinear(E, 3 * E, bias=mha.in_proj_bias is not None, device="meta", seed=seed, **opts)._adopt(packed)
        out_proj = MXTrainLinear.from_linear(mha.out_proj, seed=None if seed is None else seed + 1, **opts)
        layer = cls(in_proj, out_proj, mha.num_heads, mha.batch_first, qk_fmt=qk_fmt, p_fmt=p_fmt, v_fmt=v_fmt, grad_fmt=grad_fmt,
                    grad_rounding=grad_rounding, seed=None if seed is None else seed + 2, softmax=softmax)
        return layer.train(mha.training)

    def forward(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor] = None, is_causal: bool = False, *, need_weights: bool = False,
                key_padding_mask: Optional[torch.Tensor] = None, rope=None, rope_interleaved: bool = False):
        if need_weights:
            raise ValueError("need_weights=True is not offered: the attention weights exist only inside mx_attention_train")
        if key_padding_mask is not None:
            raise ValueError("key_padding_mask is not offered: fold it into attn_mask")
        if x.dim() != 3 or x.shape[-1] != self.embed_dim:
            raise ValueError(f"x must be {'[B, T, E]' if self.batch_first else '[T, B, E]'} with E = {self.embed_dim}, got shape {tuple(x.shape)}")
        h, E = self.num_heads, self.embed_dim
        xb = x if self.batch_first else x.transpose(0, 1)
        B, T = xb.shape[:2]
        q, k, v = (t.view(B, T, h, E // h).transpose(1, 2) for t in self.in_proj(xb).chunk(3, -1))      # views: nothing is copied
        seed, step = self._mx_sr()
        o = mx_attention_train(q, k, v, attn_mask, is_causal, qk_fmt=self.qk_fmt, p_fmt=self.p_fmt, v_fmt=self.v_fmt,
                               grad_fmt=self.grad_fmt, grad_rounding=self.grad_rounding, seed=seed, step=step, softmax=self.softmax,
                               rope=rope, rope_interleaved=rope_interleaved)
        y = self.out_proj(o.transpose(1, 2).reshape(B, T, E))
        return (y if self.batch_first else y.transpose(0, 1)), None

    def to_inference(self) -> MXMultiheadAttention:
        """the ``MXMultiheadAttention`` on the current weights, in this layer's attention formats and ``softmax`` setting"""
        return MXMultiheadAttention(self.in_proj.to_inference(), self.out_proj.to_inference(), self.num_heads, self.batch_first,
                                    qk_fmt=self.qk_fmt, p_fmt=self.p_fmt, v_fmt=self.v_fmt, softmax=self.softmax)


__all__ = ["mx_quantize_2way_batched", "mx_bmm_train", "mx_attention_train", "MXTrainMultiheadAttention"]
