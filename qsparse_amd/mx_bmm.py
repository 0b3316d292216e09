"""Batched matrix products on MX codes: ``mx_bmm``, the attention built on it (``mx_attention``) and the inference-side layer
``MXMultiheadAttention``.

``mx_matmul`` multiplies an activation by ONE weight ``[N, K]``.  ``mx_bmm`` multiplies slice by slice -- ``a_codes [..., M, K]`` by
``b_codes [..., N, K]`` with equal leading dimensions, neither operand shared -- in one launch (``qs_mx_bmm_v``): the ``Q . K^T`` and
``P . V`` of attention, one small product per (image, head), or a linear layer per expert.  Slice by slice it computes bit for bit
what ``mx_matmul`` computes.  The argument checks are ``_mx_common.py``'s."""
from functools import partial
from typing import Optional

import torch
import torch.nn as nn

from qsparse_amd import _hip, _mx_common
from qsparse_amd._mx_common import _check_codes_out, _check_dtype, _codes_out_cpu
from qsparse_amd.mx_gemm import MXLinear
from qsparse_amd.quantize import _mx_format, mx_dequantize, quantize_with_mx

_check_a = partial(_mx_common._check_operand, what="[..., M, K]", least=3, most=None, needs="at least 3 dimensions")
_check_b = partial(_mx_common._check_operand, what="[..., N, K]", least=3, most=None, needs="at least 3 dimensions")


def mx_bmm(a_codes: torch.Tensor, a_scales: torch.Tensor, a_fmt: str, b_codes: torch.Tensor, b_scales: torch.Tensor, b_fmt: str,
           bias: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32, *, out_fmt: Optional[str] = None,
           act: Optional[str] = None):
    """``A[g] . B[g]^T (+ bias)`` on MX codes for every slice ``g``.  ``a_codes`` ``[..., M, K]`` and ``b_codes`` ``[..., N, K]`` are
    uint8 codes of the formats ``a_fmt`` / ``b_fmt`` (``MX_FORMATS``; they may differ) with blocks along K and EQUAL leading dimensions
    (at least one; nothing is broadcast -- one ``[N, K]`` weight for every row is ``mx_matmul``), ``a_scales`` ``[..., M, ceil(K /
    32)]`` and ``b_scales`` ``[..., N, ceil(K / 32)]`` their E8M0 bytes, ``bias`` float32 ``[N]`` (shared by the slices) or ``[..., N]``
    with the operands' leading dimensions.  Returns ``[..., M, N]`` in ``out_dtype`` (float32, bfloat16 or float16):

        y[g, m, n] = round( sum_k val(a[g, m, k]) 2^(sa[g, m, k / 32] - 127) val(b[g, n, k]) 2^(sb[g, n, k / 32] - 127) + bias[g or -, n] )

    Slice ``g`` of the result is bit for bit ``mx_matmul`` of slice ``g`` of the operands, on either device.  A scale byte 0xFF makes
    every output that reads it NaN, in its slice only.  GPU tensors take the HIP kernel (one launch for all slices; there is no
    fallback: without the library the call raises), CPU tensors evaluate the expression above in float64, slice by slice, and round
    once.

    ``out_fmt`` / ``act`` (keywords) are ``mx_matmul``'s: with ``out_fmt`` the return is ``(codes uint8 [..., M, N], scales uint8 [...,
    M, ceil(N / 32)])``, the codes of ``quantize_with_mx(act(y), out_fmt, -1, return_codes=True)`` with ``y`` the float32 result,
    written by the product's epilogue on the GPU (``qs_mx_bmm_q_v``); ``act`` is ``None`` or ``"relu"`` and needs ``out_fmt``, and
    ``out_dtype`` stays at its default.  There is no ``split_k``."""
    _check_codes_out("mx_bmm", out_fmt, act, out_dtype)
    _check_a("a", a_codes, a_scales, a_fmt)
    if isinstance(b_codes, torch.Tensor) and b_codes.dim() == 2:
        raise ValueError(f"b_codes must be [..., N, K] with the leading dimensions of a_codes, got shape {tuple(b_codes.shape)}: one "
                         "weight [N, K] shared by every row of a is mx_matmul")
    _check_b("b", b_codes, b_scales, b_fmt)
    lead = tuple(a_codes.shape[:-2])
    if tuple(b_codes.shape[:-2]) != lead:
        raise ValueError(f"a_codes {tuple(a_codes.shape)} and b_codes {tuple(b_codes.shape)} disagree on their leading dimensions "
                         "(nothing is broadcast)")
    (M, K), N = a_codes.shape[-2:], b_codes.shape[-2]
    if b_codes.shape[-1] != K:
        raise ValueError(f"a_codes {tuple(a_codes.shape)} and b_codes {tuple(b_codes.shape)} disagree on K (their last dimensions)")
    if K < 1:
        raise ValueError("mx_bmm needs K >= 1")
    if b_codes.device != a_codes.device:
        raise ValueError(f"a_codes is on {a_codes.device} but b_codes on {b_codes.device}")
    _check_dtype("out_dtype", out_dtype)
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
            raise TypeError("bias must be a float32 tensor")
        if tuple(bias.shape) not in ((N,), lead + (N,)):
            raise ValueError(f"bias has shape {tuple(bias.shape)}, expected ({N},) or {lead + (N,)}")
        if bias.device != a_codes.device:
            raise ValueError(f"a_codes is on {a_codes.device} but bias on {bias.device}")
    G = 1
    for n in lead:
        G *= n
    if bias is not None and bias.dim() > 1:
        bias = bias.reshape(G, N)
    a3, sa3 = a_codes.reshape(G, M, K), a_scales.reshape(G, M, a_scales.shape[-1])
    b3, sb3 = b_codes.reshape(G, N, K), b_scales.reshape(G, N, b_scales.shape[-1])
    if a_codes.is_cuda:
        ops = (a3.contiguous(), sa3.contiguous(), a_fmt, b3.contiguous(), sb3.contiguous(), b_fmt, None if bias is None else bias.contiguous())
        if out_fmt is not None:
            codes, scales = _hip.mx_bmm_q(*ops, out_fmt, act)
            return codes.reshape(lead + (M, N)), scales.reshape(lead + (M, scales.shape[-1]))
        return _hip.mx_bmm(*ops, out_dtype).reshape(lead + (M, N))
    y = torch.empty((G, M, N), dtype=out_dtype)
    for g in range(G):               # slice by slice, the expression of mx_matmul's CPU path: the same bits
        yg = mx_dequantize(a3[g], sa3[g], a_fmt, -1, torch.float64) @ mx_dequantize(b3[g], sb3[g], b_fmt, -1, torch.float64).t()
        if bias is not None:
            yg = yg + (bias[g] if bias.dim() > 1 else bias).to(torch.float64)
        y[g] = yg.to(out_dtype)
    y = y.reshape(lead + (M, N))
    if out_fmt is not None and y.numel() == 0:      # (the CPU quantizer takes no empty tensor)
        return y.new_empty(y.shape, dtype=torch.uint8), y.new_empty(lead + (M, (N + 31) // 32), dtype=torch.uint8)
    return y if out_fmt is None else _codes_out_cpu(y, out_fmt, act)


MX_ATTENTION_SOFTMAX = ("torch", "fused")


def _attention_mask(attn_mask, is_causal: bool, T: int, S: int, device):
    """the additive float32 mask of `mx_attention`, or None"""
    if attn_mask is not None and is_causal:
        raise ValueError("give attn_mask or is_causal, not both")
    if is_causal:
        attn_mask = torch.ones(T, S, dtype=torch.bool, device=device).tril()      # top-left aligned, as F.scaled_dot_product_attention
    if attn_mask is None:
        return None
    if not isinstance(attn_mask, torch.Tensor):
        raise TypeError(f"attn_mask must be a tensor, got {type(attn_mask).__name__}")
    if attn_mask.dim() < 2 or tuple(attn_mask.shape[-2:]) != (T, S):
        raise ValueError(f"attn_mask has shape {tuple(attn_mask.shape)}, expected [..., {T}, {S}] (broadcast over the leading dimensions)")
    if attn_mask.device != device:
        raise ValueError(f"q is on {device} but attn_mask on {attn_mask.device}")
    if attn_mask.dtype == torch.bool:
        return torch.zeros(attn_mask.shape, dtype=torch.float32, device=device).masked_fill(~attn_mask, float("-inf"))
    if not attn_mask.is_floating_point():
        raise TypeError(f"attn_mask must be a boolean or a floating-point tensor, got {attn_mask.dtype}")
    return attn_mask.to(torch.float32)


def mx_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor] = None, is_causal: bool = False,
                 scale: Optional[float] = None, *, qk_fmt: str = "mxfp8_e4m3", p_fmt: str = "mxfp8_e4m3", v_fmt: str = "mxfp8_e4m3",
                 out_dtype: torch.dtype = torch.float32, softmax: str = "torch", rope=None, rope_interleaved: bool = False) -> torch.Tensor:
    """Inference-side scaled dot-product attention whose two matrix products run on MX codes.  ``q [..., T, d]``, ``k [..., S, d]``
    and ``v [..., S, dv]`` are float32 / bfloat16 / float16 tensors with equal leading dimensions (at least one); the result is
    ``[..., T, dv]`` in ``out_dtype``.  It is DEFINED as this composition of public calls, and is bit for bit that composition on
    either device:

        1. ``q`` and ``k`` -> ``quantize_with_mx(., qk_fmt, -1, return_codes=True)``: blocks along ``d``
        2. ``s = mx_bmm(q, k)`` in float32: ``[..., T, S]``
        3. ``s = s * scale`` (float32, in torch), ``scale`` defaulting to ``d ** -0.5``
        4. ``s = s + mask``: ``attn_mask`` ``[..., T, S]`` broadcast over the leading dimensions -- a float mask is added, a boolean
           one adds ``-inf`` where it is False -- or, with ``is_causal``, the boolean lower triangle aligned top-left (as
           ``F.scaled_dot_product_attention`` takes it).  Giving both raises
        5. ``p = softmax(s, -1)`` in float32
        6. ``p`` -> ``quantize_with_mx(p, p_fmt, -1, return_codes=True)``: blocks along ``S``
        7. ``v.transpose(-1, -2).contiguous()`` -> ``quantize_with_mx(., v_fmt, -1, return_codes=True)``: blocks along ``S``.  This
           is one layout pass over ``v``: the product wants K (here ``S``) innermost and takes no strided operand
        8. ``mx_bmm(p, v^T)`` to ``out_dtype``

    ``softmax="fused"`` (keyword; the default ``"torch"`` is the composition above, bit for bit as it always was) replaces steps 3 - 6
    by ONE call, ``mx_softmax_quantize(s, attn_mask, scale=scale, is_causal=is_causal, fmt=p_fmt)``: on the GPU one launch that reads
    ``s`` once and writes only ``p``'s codes, with ``is_causal`` handed down so that no ``[T, S]`` mask tensor is built.  With
    ``"fused"`` the result is DEFINED as that composition, bit for bit on either device; its ``p`` comes from ``mx_softmax_quantize``'s
    own written-out exponential, not from ``torch.softmax``, so the two settings usually agree but are not each other's definition.

    ``rope`` (keyword; ``None`` changes no call, launch or bit) rotates ``q`` and ``k`` in front of their quantizer, in either softmax
    mode: a 2-tuple ``(cos, sin)`` of ``mx_rope`` tables ``[T, d / 2]`` rotates both and needs ``T == S``, a 4-tuple ``(cos_q, sin_q,
    cos_k, sin_k)`` takes ``[T, d / 2]`` and ``[S, d / 2]`` tables (decoding against a longer key sequence); ``rope_interleaved`` is
    ``mx_rope``'s ``interleaved``.  Step 1 then is the row pair of ``mx_rope_quantize(q, cos_q, sin_q, row_fmt=qk_fmt,
    interleaved=rope_interleaved)`` and of ``mx_rope_quantize(k, cos_k, sin_k, ...)``: on the GPU one launch each that reads ``q`` /
    ``k`` where it lies and never writes the rotated tensor.

    No dropout and no gradient: a tensor that requires grad while gradients are enabled is refused -- the training side of attention
    is not offered.  A row of the mask that admits no key gives NaN, as softmax does."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        _check_dtype(name, t.dtype)
        if t.dim() < 3:
            raise ValueError(f"{name} needs at least 3 dimensions [..., {'T' if name == 'q' else 'S'}, d], got shape {tuple(t.shape)}")
        if t.device != q.device:
            raise ValueError(f"q is on {q.device} but {name} on {t.device}")
        if torch.is_grad_enabled() and t.requires_grad:
            raise RuntimeError(f"mx_attention is inference-side: {name} requires grad.  The training side of attention on MX codes is "
                               "not offered; call it under torch.no_grad()")
    for fmt in (qk_fmt, p_fmt, v_fmt):
        _mx_format(fmt)
    _check_dtype("out_dtype", out_dtype)
    if softmax not in MX_ATTENTION_SOFTMAX:
        raise ValueError(f"unknown softmax {softmax!r}: one of {MX_ATTENTION_SOFTMAX}")
    lead, (T, d), S = tuple(q.shape[:-2]), q.shape[-2:], k.shape[-2]
    if tuple(k.shape[:-2]) != lead or tuple(v.shape[:-2]) != lead:
        raise ValueError(f"q {tuple(q.shape)}, k {tuple(k.shape)} and v {tuple(v.shape)} disagree on their leading dimensions (nothing "
                         "is broadcast)")
    if k.shape[-1] != d:
        raise ValueError(f"q {tuple(q.shape)} and k {tuple(k.shape)} disagree on d (their last dimensions)")
    if v.shape[-2] != S:
        raise ValueError(f"k {tuple(k.shape)} and v {tuple(v.shape)} disagree on S (their second-to-last dimensions)")
    if d < 1 or S < 1:
        raise ValueError("mx_attention needs d >= 1 and S >= 1")
    fused = softmax == "fused"
    if fused and attn_mask is not None and is_causal:
        raise ValueError("give attn_mask or is_causal, not both")
    if rope is not None:
        from qsparse_amd.mx_rope import _attention_rope, mx_rope_quantize      # (it takes the batched quantizer, which imports this module)
        rope = _attention_rope(rope, T, S, d, q.device)
    with torch.no_grad():
        mask = None if fused else _attention_mask(attn_mask, is_causal, T, S, q.device)
        if rope is None:
            _, qc, qsc = quantize_with_mx(q.detach(), qk_fmt, -1, return_codes=True)
            _, kc, ksc = quantize_with_mx(k.detach(), qk_fmt, -1, return_codes=True)
        else:
            qc, qsc = mx_rope_quantize(q, rope[0], rope[1], row_fmt=qk_fmt, interleaved=rope_interleaved)[:2]
            kc, ksc = mx_rope_quantize(k, rope[2], rope[3], row_fmt=qk_fmt, interleaved=rope_interleaved)[:2]
        s = mx_bmm(qc, qsc, qk_fmt, kc, ksc, qk_fmt)
        if fused:
            from qsparse_amd.mx_softmax import mx_softmax_quantize     # (it takes `_attention_mask` from this module)
            pc, psc = mx_softmax_quantize(s, attn_mask, scale=d ** -0.5 if scale is None else scale, is_causal=is_causal, fmt=p_fmt)
        else:
            s = s * (d ** -0.5 if scale is None else scale)
            if mask is not None:
                s = s + mask
            _, pc, psc = quantize_with_mx(torch.softmax(s, -1), p_fmt, -1, return_codes=True)
        _, vc, vsc = quantize_with_mx(v.detach().transpose(-1, -2).contiguous(), v_fmt, -1, return_codes=True)
        return mx_bmm(pc, psc, p_fmt, vc, vsc, v_fmt, None, out_dtype)


class MXMultiheadAttention(nn.Module):
    """A self-attention ``nn.MultiheadAttention`` for inference on MX codes: two ``MXLinear`` s -- the packed ``in_proj`` ``[3 E, E]``
    and ``out_proj`` ``[E, E]`` -- around ``mx_attention`` over ``[B, h, T, d]``.  ``forward(x, attn_mask=None, is_causal=False)``
    takes ``x`` ``[T, B, E]`` (``[B, T, E]`` with ``batch_first``) and returns ``(output, None)``, the pair ``nn.MultiheadAttention``
    returns without its weights; the mask goes to ``mx_attention`` as it is (``[T, T]`` or anything that broadcasts to ``[B, h, T,
    T]``).  It is a thin composition -- ``in_proj(x)``, split, ``mx_attention``, merge, ``out_proj`` -- and equals it bit for bit.
    ``need_weights`` and ``key_padding_mask`` are not offered.  ``softmax`` (``"torch"`` or ``"fused"``) is ``mx_attention``'s keyword,
    stored and passed on; ``forward``'s ``rope`` / ``rope_interleaved`` are ``mx_attention``'s too, call arguments and not state."""

    def __init__(self, in_proj: MXLinear, out_proj: MXLinear, num_heads: int, batch_first: bool = False, *, qk_fmt: str = "mxfp8_e4m3",
                 p_fmt: str = "mxfp8_e4m3", v_fmt: str = "mxfp8_e4m3", softmax: str = "torch"):
        super().__init__()
        if not isinstance(in_proj, MXLinear) or not isinstance(out_proj, MXLinear):
            raise TypeError("in_proj and out_proj must be MXLinear layers")
        E = out_proj.in_features
        if in_proj.in_features != E or in_proj.out_features != 3 * E or out_proj.out_features != E:
            raise ValueError(f"in_proj must be [3 E, E] and out_proj [E, E], got [{in_proj.out_features}, {in_proj.in_features}] and "
                             f"[{out_proj.out_features}, {out_proj.in_features}]")
        if in_proj.out_fmt is not None or in_proj.out_dtype is not torch.float32:
            raise ValueError("in_proj must return float32 (no out_fmt, out_dtype=torch.float32): mx_attention quantizes q, k and v itself")
        if isinstance(num_heads, bool) or not isinstance(num_heads, int) or num_heads < 1 or E % num_heads:
            raise ValueError(f"num_heads must be an int >= 1 that divides embed_dim {E}, got {num_heads!r}")
        for fmt in (qk_fmt, p_fmt, v_fmt):
            _mx_format(fmt)
        if softmax not in MX_ATTENTION_SOFTMAX:
            raise ValueError(f"unknown softmax {softmax!r}: one of {MX_ATTENTION_SOFTMAX}")
        self.softmax = softmax
        self.in_proj, self.out_proj = in_proj, out_proj
        self.embed_dim, self.num_heads, self.batch_first = E, num_heads, bool(batch_first)
        self.qk_fmt, self.p_fmt, self.v_fmt = qk_fmt, p_fmt, v_fmt

    def extra_repr(self) -> str:
        return (f"embed_dim={self.embed_dim}, num_heads={self.num_heads}, batch_first={self.batch_first}, qk_fmt={self.qk_fmt!r}, "
                f"p_fmt={self.p_fmt!r}, v_fmt={self.v_fmt!r}")

    @classmethod
    def from_float(cls, mha: nn.MultiheadAttention, act_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", *, qk_fmt: str = "mxfp8_e4m3",
                   p_fmt: str = "mxfp8_e4m3", v_fmt: str = "mxfp8_e4m3", softmax: str = "torch"):
        """from a float self-attention module: both weights quantized with ``quantize_with_mx(w, w_fmt, 1, return_codes=True)``"""
        if not isinstance(mha, nn.MultiheadAttention):
            raise TypeError(f"MXMultiheadAttention.from_float needs an nn.MultiheadAttention, got {type(mha).__name__}")
        if not mha._qkv_same_embed_dim:
            raise ValueError("kdim / vdim other than embed_dim are not supported: MXMultiheadAttention is self-attention on one packed in_proj")
        if mha.bias_k is not None or mha.bias_v is not None:
            raise ValueError("add_bias_kv=True is not supported")
        if mha.add_zero_attn:
            raise ValueError("add_zero_attn=True is not supported")
        with torch.no_grad():
            layers = []
            for w, b in ((mha.in_proj_weight, mha.in_proj_bias), (mha.out_proj.weight, mha.out_proj.bias)):
                _, codes, scales = quantize_with_mx(w.detach(), w_fmt, 1, return_codes=True)
                layers.append(MXLinear(codes, scales, w_fmt, None if b is None else b.detach(), act_fmt))
        return cls(*layers, mha.num_heads, mha.batch_first, qk_fmt=qk_fmt, p_fmt=p_fmt, v_fmt=v_fmt, softmax=softmax)

    def forward(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor] = None, is_causal: bool = False, *, need_weights: bool = False,
                key_padding_mask: Optional[torch.Tensor] = None, rope=None, rope_interleaved: bool = False):
        if need_weights:
            raise ValueError("need_weights=True is not offered: the attention weights exist only as MX codes inside mx_attention")
        if key_padding_mask is not None:
            raise ValueError("key_padding_mask is not offered: fold it into attn_mask")
        if x.dim() != 3 or x.shape[-1] != self.embed_dim:
            raise ValueError(f"x must be {'[B, T, E]' if self.batch_first else '[T, B, E]'} with E = {self.embed_dim}, got shape {tuple(x.shape)}")
        h, E = self.num_heads, self.embed_dim
        xb = x if self.batch_first else x.transpose(0, 1)
        B, T = xb.shape[:2]
        q, k, v = (t.reshape(B, T, h, E // h).transpose(1, 2) for t in self.in_proj(xb).chunk(3, -1))
        o = mx_attention(q, k, v, attn_mask, is_causal, qk_fmt=self.qk_fmt, p_fmt=self.p_fmt, v_fmt=self.v_fmt, softmax=self.softmax,
                         rope=rope, rope_interleaved=rope_interleaved)
        y = self.out_proj(o.transpose(1, 2).reshape(B, T, E))
        return (y if self.batch_first else y.transpose(0, 1)), None


__all__ = ["mx_bmm", "mx_attention", "MXMultiheadAttention"]
