"""RMSNorm / LayerNorm in front of the MX quantizer: ``mx_norm_quantize``, the inference layers ``MXRMSNorm`` / ``MXLayerNorm`` and the
training pair ``mx_norm_linear`` / ``MXTrainNormLinear``.

The QKV projection and the (gated) MLP's up projection read the output of a normalisation.  ``mx_norm_quantize`` hands that output
out as MX codes -- the row pair a forward product multiplies and, for training, the transposed col pair the weight gradient needs --
without the float tensor in between: on the GPU ``qs_mx_norm_quant_v`` (a statistics launch and a quantizing launch, no fallback), on
the CPU the definition below in torch ops.  The definition (``include/qsparse_hip.h``, "MX normalising quantizer") is float32 without
contraction and fixes the order of the row sums as a function of ``C`` alone, so both paths give the same bytes.

The argument checks follow ``_mx_common.py``; the training layer's options, counter and autocast are ``_MXTrainMixin``'s."""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from qsparse_amd import _hip
from qsparse_amd._mx_common import (MXActivation, _check_bias_shape, _check_dtype, _check_train_entry, _MXTrainMixin, _quantize_grad,
                                    _save_train_ctx)
from qsparse_amd.mx_gemm import MXLinear, mx_matmul, mx_quantize_2way
from qsparse_amd.quantize import _mx_format, quantize_with_mx

MX_NORMS = ("rms", "layer")
_PASS, _PARTIALS = 512, 128     # a row is summed in passes of 512 elements: 128 partial sums of quads


def _row_sum(t: torch.Tensor) -> torch.Tensor:
    """sum over the last axis of float32 ``t [R, C]`` in the definition's order: zero padding to a multiple of 512, quad sums, 128
    strided partial sums in ascending order, a pairwise tree -- element-wise additions on slices only"""
    R, C = t.shape
    K = -(-C // _PASS)
    q = F.pad(t, (0, K * _PASS - C)).view(R, K, _PARTIALS, 4)
    q = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    P = torch.zeros(R, _PARTIALS, dtype=torch.float32, device=t.device)
    for k in range(K):
        P = P + q[:, k]
    s = _PARTIALS // 2
    while s >= 1:
        P = P[:, :s] + P[:, s:2 * s]
        s //= 2
    return P[:, 0]


def _norm_xhat(x2: torch.Tensor, rstd: torch.Tensor, mean: Optional[torch.Tensor]) -> torch.Tensor:
    """xhat = (x - mean) * rstd, float32, as the forward forms it"""
    x32 = x2.to(torch.float32)
    return (x32 if mean is None else x32 - mean[:, None]) * rstd[:, None]


def _mx_norm_y(x2: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], norm: str, eps: float):
    """the definition in torch float32 ops on ``x2 [R, C]`` (``weight`` / ``bias`` float32 ``[C]`` or None): returns ``(y, rstd,
    mean | None)``, ``y`` the float32 tensor the quantizer is defined on -- the CPU path of ``mx_norm_quantize``, and what tests compare
    the GPU against"""
    x32 = x2.to(torch.float32)
    cf = torch.tensor(float(x2.shape[1]), dtype=torch.float32, device=x2.device)
    e = torch.tensor(eps, dtype=torch.float32, device=x2.device)
    mean = None
    if norm == "layer":
        mean = _row_sum(x32) / cf
        d = x32 - mean[:, None]
        ms = _row_sum(d * d) / cf
    else:
        ms = _row_sum(x32 * x32) / cf
    # the correctly rounded float32 sqrt: ATen's vectorised float32 sqrt on the CPU is not (its last bit differs between machines), the
    # float64 one rounded once more is -- no float32 lies within a float64 ulp of the midpoint of two float32 square roots
    rstd = torch.ones_like(ms) / torch.sqrt((ms + e).to(torch.float64)).to(torch.float32)
    rstd = torch.where(torch.isfinite(ms), rstd, torch.full_like(ms, float("nan")))
    y = _norm_xhat(x2, rstd, mean)
    if weight is not None:
        y = y * weight
    if bias is not None:
        y = y + bias
    return y, rstd, mean


def _check_norm_args(x, weight, bias, norm, eps):
    """the operands of ``mx_norm_quantize``; returns (weight, bias) as detached float32 tensors (or None)"""
    if norm not in MX_NORMS:
        raise ValueError(f"unknown norm {norm!r}: one of {MX_NORMS}")
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a tensor, got {type(x).__name__}")
    _check_dtype("x", x.dtype)
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"mx_norm_quantize needs x [..., C] with C >= 1, got shape {tuple(x.shape)}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)):
        raise TypeError(f"eps must be a float, got {type(eps).__name__}")
    if not 0.0 <= eps < float("inf"):
        raise ValueError(f"eps must be finite and >= 0, got {eps}")
    out = []
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None:
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
            _check_dtype(name, t.dtype)
            if tuple(t.shape) != (x.shape[-1],):
                raise ValueError(f"{name} has shape {tuple(t.shape)}, expected ({x.shape[-1]},): the normalisation runs over the last "
                                 f"dimension of x {tuple(x.shape)}")
            if t.device != x.device:
                raise ValueError(f"x is on {x.device} but {name} on {t.device}")
            t = t.detach().to(torch.float32).contiguous()
        out.append(t)
    return out


def _norm_results(lead, rc, rs, cc, cs, rstd, mean, col_fmt, return_stats):
    """the flat tuple ``mx_norm_quantize`` returns, from the results on ``[R, C]``: the row pair and the statistics shaped by ``lead``"""
    out = (rc.reshape(lead + (rc.shape[-1],)), rs.reshape(lead + (rs.shape[-1],)))
    if col_fmt is not None:
        out += (cc, cs)
    if return_stats:
        out += (rstd.reshape(lead), None if mean is None else mean.reshape(lead))
    return out


def mx_norm_quantize(x: torch.Tensor, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, *, norm: str = "rms",
                     eps: float = 1e-6, fmt: str = "mxfp8_e4m3", col_fmt: Optional[str] = None, return_stats: bool = False):
    """MX codes of ``y = norm(x) * weight (+ bias)`` over the last dimension of ``x [..., C]`` (float32 / bfloat16 / float16), the float
    ``y`` never written.  ``norm`` is ``"rms"`` or ``"layer"``; ``weight`` / ``bias`` are ``[C]`` or None (ones / none).  Returns

        (codes [..., C], scales [..., ceil(C / 32)])      the codes and scales of ``quantize_with_mx(y, fmt, -1, return_codes=True)``
        + (col_codes [C, R], col_scales [C, ceil(R / 32)])  with ``col_fmt``: the col pair of ``mx_quantize_2way(y2, None, col_fmt)``,
                                                          ``y2`` being ``y`` with its leading dimensions flattened to ``R``
        + (rstd [...], mean [...] | None)                 with ``return_stats``: float32, what a backward keeps (mean: layer mode)

    as one flat tuple.  All arithmetic is float32:

        rms     ms = sum(x_i * x_i) / C                     y_i = (x_i * rstd) * w_i (+ b_i)
        layer   mean = sum(x_i) / C,  d_i = x_i - mean,     y_i = (d_i * rstd) * w_i (+ b_i)
                ms = sum(d_i * d_i) / C
        rstd = 1 / sqrt(ms + eps)

    with the row sums in one fixed order that depends on ``C`` alone (zero padding to a multiple of 512, sums of aligned quads,
    128 strided partial sums, a pairwise tree), so the bytes are the same on the CPU and on the GPU, for every dtype and shape of the
    leading dimensions.  A row that holds a NaN or an Inf (``ms`` not finite) is NaN as a whole: scale byte 0xFF in every block it
    touches, in both pairs.  Rounding is to nearest; the outputs are never differentiable.  GPU tensors take the HIP kernels (no
    fallback), CPU tensors the torch expression of the definition."""
    weight, bias = _check_norm_args(x, weight, bias, norm, eps)
    _mx_format(fmt)
    if col_fmt is not None:
        _mx_format(col_fmt)
    C = x.shape[-1]
    lead = tuple(x.shape[:-1])
    x2 = x.detach().reshape(-1, C)
    if x.is_cuda:
        rc, rs, cc, cs, rstd, mean = _hip.mx_norm_quant(x2.contiguous(), weight, bias, norm, eps, fmt, col_fmt)
    else:
        y, rstd, mean = _mx_norm_y(x2, weight, bias, norm, float(eps))
        _, rc, rs = quantize_with_mx(y, fmt, -1, return_codes=True)
        cc, cs = mx_quantize_2way(y, None, col_fmt)[2:] if col_fmt is not None else (None, None)
    return _norm_results(lead, rc, rs, cc, cs, rstd, mean, col_fmt, return_stats)


def _check_residual(x, residual):
    """the second operand of the add-norm forms: a tensor of x's shape and device, of any of the three dtypes"""
    if not isinstance(residual, torch.Tensor):
        raise TypeError(f"residual must be a tensor, got {type(residual).__name__}")
    _check_dtype("residual", residual.dtype)
    if residual.shape != x.shape:
        raise ValueError(f"residual has shape {tuple(residual.shape)}, expected x's {tuple(x.shape)}")
    if residual.device != x.device:
        raise ValueError(f"x is on {x.device} but residual on {residual.device}")


def mx_add_norm_quantize(x: torch.Tensor, residual: torch.Tensor, weight: Optional[torch.Tensor] = None,
                         bias: Optional[torch.Tensor] = None, *, norm: str = "rms", eps: float = 1e-6, fmt: str = "mxfp8_e4m3",
                         col_fmt: Optional[str] = None, return_stats: bool = False):
    """The residual add of a pre-norm block and ``mx_norm_quantize`` behind it: ``x [..., C]`` is the output of the previous branch,
    ``residual`` (same shape and device; float32 / bfloat16 / float16, not necessarily ``x``'s dtype) the stream.  Returns

        (h,) + mx_norm_quantize(h, weight, bias, norm=norm, eps=eps, fmt=fmt, col_fmt=col_fmt, return_stats=return_stats)

    with ``h = (x.float() + residual.float()).to(residual.dtype)``, the new stream: ONE float32 addition, rounded once to the stream's
    dtype.  The normalisation sees that rounded ``h``, so every output is bit for bit the composition's.  On the GPU it is the two
    launches of ``qs_mx_add_norm_quant_v`` (no fallback): the statistics launch reads ``x`` and ``residual``, writes ``h`` and sums the
    rounded values; the quantizing launch is ``mx_norm_quantize``'s on ``h`` -- the ``torch.add`` pass and one read of ``h`` less.  A
    NaN or an Inf in either operand is kept in ``h`` and makes the row NaN as a whole.  ``h`` is a new tensor (the stream is not
    updated in place).  Nothing here is differentiable (``mx_add_norm_linear`` is)."""
    weight, bias = _check_norm_args(x, weight, bias, norm, eps)
    _check_residual(x, residual)
    _mx_format(fmt)
    if col_fmt is not None:
        _mx_format(col_fmt)
    if not x.is_cuda:
        h = (x.detach().to(torch.float32) + residual.detach().to(torch.float32)).to(residual.dtype)
        return (h,) + mx_norm_quantize(h, weight, bias, norm=norm, eps=eps, fmt=fmt, col_fmt=col_fmt, return_stats=return_stats)
    C = x.shape[-1]
    lead = tuple(x.shape[:-1])
    h, rc, rs, cc, cs, rstd, mean = _hip.mx_add_norm_quant(x.detach().reshape(-1, C).contiguous(), residual.detach().reshape(-1, C).contiguous(),
                                                           weight, bias, norm, eps, fmt, col_fmt)
    return (h.reshape(x.shape),) + _norm_results(lead, rc, rs, cc, cs, rstd, mean, col_fmt, return_stats)


def _eps_of(eps, x: torch.Tensor) -> float:
    """``nn.RMSNorm``'s rule for ``eps=None``: the machine epsilon of the input's dtype"""
    return float(torch.finfo(x.dtype).eps) if eps is None else float(eps)


def _norm_kind(module) -> str:
    if isinstance(module, nn.RMSNorm):
        return "rms"
    if isinstance(module, nn.LayerNorm):
        return "layer"
    raise TypeError(f"needs an nn.RMSNorm or nn.LayerNorm, got {type(module).__name__}")


def _last_dim(normalized_shape) -> int:
    shape = (normalized_shape,) if isinstance(normalized_shape, int) else tuple(normalized_shape)
    if len(shape) != 1:
        raise ValueError(f"normalized_shape {shape} has {len(shape)} dimensions: the MX norms run over the last dimension only")
    return int(shape[0])


class _MXNorm(nn.Module):
    """what ``MXRMSNorm`` and ``MXLayerNorm`` share: the parameters under the float module's names, ``from_float``, ``forward``"""
    norm = None
    _float = None

    def __init__(self, normalized_shape, eps, elementwise_affine: bool = True, bias: bool = True, out_fmt: str = "mxfp8_e4m3",
                 device=None, dtype=None):
        super().__init__()
        _mx_format(out_fmt)
        C = _last_dim(normalized_shape)
        self.normalized_shape, self.eps, self.elementwise_affine, self.out_fmt = (C,), eps, elementwise_affine, out_fmt
        kw = dict(device=device, dtype=dtype)
        self.register_parameter("weight", nn.Parameter(torch.ones(C, **kw)) if elementwise_affine else None)
        if self.norm == "layer":
            self.register_parameter("bias", nn.Parameter(torch.zeros(C, **kw)) if elementwise_affine and bias else None)

    @classmethod
    def from_float(cls, module: nn.Module, out_fmt: str = "mxfp8_e4m3"):
        """the layer on ``module``'s own parameters (shared, not copied); ``module`` is the float class this one stands for"""
        if not isinstance(module, cls._float):
            raise TypeError(f"{cls.__name__}.from_float needs an nn.{cls._float.__name__}, got {type(module).__name__}")
        _last_dim(module.normalized_shape)
        self = cls(module.normalized_shape, module.eps, elementwise_affine=False, out_fmt=out_fmt)
        self.elementwise_affine = module.elementwise_affine
        self.weight = module.weight
        if cls.norm == "layer":
            self.bias = module.bias
        return self.train(module.training)

    def extra_repr(self) -> str:
        return f"{self.normalized_shape}, eps={self.eps}, elementwise_affine={self.elementwise_affine}, out_fmt={self.out_fmt!r}"

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None):
        """the ``MXActivation`` of ``norm(x)``; with ``residual`` (the stream of a pre-norm block) ``(MXActivation of norm(h), h)``,
        ``h = x + residual`` in ``residual``'s dtype -- ``mx_add_norm_quantize``; ``eps=None`` then follows ``h``'s dtype"""
        for t in (x, residual):
            if isinstance(t, torch.Tensor) and torch.is_grad_enabled() and t.requires_grad:
                raise RuntimeError(f"{type(self).__name__} is an inference layer: its input requires grad.  Train with MXTrainNormLinear "
                                   "or call it under torch.no_grad()")
        if isinstance(x, torch.Tensor) and x.dim() >= 1 and x.shape[-1] != self.normalized_shape[0]:
            raise ValueError(f"x {tuple(x.shape)} does not end in normalized_shape {self.normalized_shape}")
        stream = x if residual is None else residual
        kw = dict(norm=self.norm, eps=_eps_of(self.eps, stream) if isinstance(stream, torch.Tensor) else 0.0, fmt=self.out_fmt)
        with torch.no_grad():
            if residual is None:
                codes, scales = mx_norm_quantize(x, self.weight, getattr(self, "bias", None), **kw)
                return MXActivation(codes, scales, self.out_fmt)
            h, codes, scales = mx_add_norm_quantize(x, residual, self.weight, getattr(self, "bias", None), **kw)
        return MXActivation(codes, scales, self.out_fmt), h


class MXRMSNorm(_MXNorm):
    """``nn.RMSNorm`` over the last dimension whose ``forward`` returns an ``MXActivation`` -- the codes and scales of
    ``mx_norm_quantize(x, weight, norm="rms", eps=eps, fmt=out_fmt)`` -- which ``MXLinear``, ``MXGLULinear`` and
    ``MXMultiheadAttention``'s ``in_proj`` take in place of a float tensor.  The ``state_dict`` is ``nn.RMSNorm``'s;
    ``elementwise_affine=False`` has no weight; ``eps=None`` is the machine epsilon of the input's dtype, as in torch."""
    norm, _float = "rms", nn.RMSNorm

    def __init__(self, normalized_shape, eps: Optional[float] = None, elementwise_affine: bool = True, out_fmt: str = "mxfp8_e4m3",
                 device=None, dtype=None):
        super().__init__(normalized_shape, eps, elementwise_affine, False, out_fmt, device, dtype)


class MXLayerNorm(_MXNorm):
    """``nn.LayerNorm`` over the last dimension whose ``forward`` returns an ``MXActivation`` (see ``MXRMSNorm``): the codes and scales
    of ``mx_norm_quantize(x, weight, bias, norm="layer", eps=eps, fmt=out_fmt)``.  The ``state_dict`` is ``nn.LayerNorm``'s;
    ``elementwise_affine=False`` and ``bias=False`` are supported."""
    norm, _float = "layer", nn.LayerNorm

    def __init__(self, normalized_shape, eps: float = 1e-5, elementwise_affine: bool = True, bias: bool = True,
                 out_fmt: str = "mxfp8_e4m3", device=None, dtype=None):
        super().__init__(normalized_shape, eps, elementwise_affine, bias, out_fmt, device, dtype)


def _norm_backward(dxhat: torch.Tensor, xhat: torch.Tensor, rstd: torch.Tensor, norm_weight: Optional[torch.Tensor], norm: str,
                   need_dx: bool = True, need_dw: bool = True, need_db: bool = True):
    """the normalisation's own backward in torch float32 ops (the formulas of ``mx_norm_linear``): ``dxhat [R, C]`` is the gradient
    with respect to the norm's output, ``xhat`` ``_norm_xhat``; returns (dx, d norm_weight, d norm_bias), None where not needed"""
    dx = dw = db = None
    if need_dx:
        g = dxhat if norm_weight is None else dxhat * norm_weight.to(torch.float32)
        inner = g - xhat * (g * xhat).mean(-1, keepdim=True)
        if norm == "layer":
            inner = inner - g.mean(-1, keepdim=True)
        dx = rstd[:, None] * inner
    if need_dw:
        dw = (dxhat * xhat).sum(0)
    if need_db:
        db = dxhat.sum(0)
    return dx, dw, db


_COL_TILE, _COL_PARTS = 128, 16     # a column is summed in row tiles of 128: 16 strided partial sums, then 128 over the tiles


def _halve(P: torch.Tensor) -> torch.Tensor:
    """the pairwise tree over the first axis: the upper half added to the lower until one slice is left"""
    s = P.shape[0] // 2
    while s >= 1:
        P = P[:s] + P[s:2 * s]
        s //= 2
    return P[0]


def _col_sum(t: torch.Tensor) -> torch.Tensor:
    """sum over the first axis of float32 ``t [R, C]`` in the definition's order (include/qsparse_hip.h, "MX norm backward"): zero
    padding to a multiple of 128 rows; per row tile 16 strided partial sums in ascending order and a pairwise tree; over the tiles
    128 strided partial sums and a pairwise tree -- element-wise additions on slices only, a function of ``R`` alone"""
    R, C = t.shape
    T = -(-R // _COL_TILE)
    u = F.pad(t, (0, 0, 0, T * _COL_TILE - R)).view(T, _COL_TILE // _COL_PARTS, _COL_PARTS, C)
    S = torch.zeros(T, _COL_PARTS, C, dtype=torch.float32, device=t.device)
    for m in range(_COL_TILE // _COL_PARTS):
        S = S + u[:, m]
    v = _halve(S.transpose(0, 1))                                       # [T, C]: the tile sums
    K = -(-T // _PARTIALS)
    v = F.pad(v, (0, 0, 0, K * _PARTIALS - T)).view(K, _PARTIALS, C)
    P = torch.zeros(_PARTIALS, C, dtype=torch.float32, device=t.device)
    for k in range(K):
        P = P + v[k]
    return _halve(P)


def _mx_norm_backward_f32(dxhat2: torch.Tensor, x2: torch.Tensor, rstd: torch.Tensor, mean: Optional[torch.Tensor],
                          weight: Optional[torch.Tensor], need_dx: bool = True, need_dw: bool = True, need_db: bool = True):
    """the definition of the norm's backward in torch float32 ops on ``[R, C]`` tensors (``mean`` None: rms mode): returns (dx float32,
    BEFORE its one rounding to x's dtype, dweight, dbias), None where not needed -- the CPU path of ``mx_norm_backward``"""
    d32 = dxhat2.to(torch.float32)
    xhat = _norm_xhat(x2, rstd, mean)
    dx = dw = db = None
    if need_dx:
        cf = torch.tensor(float(x2.shape[1]), dtype=torch.float32, device=x2.device)
        g = d32 if weight is None else d32 * weight
        inner = g - xhat * (_row_sum(g * xhat) / cf)[:, None]
        if mean is not None:
            inner = inner - (_row_sum(g) / cf)[:, None]
        dx = rstd[:, None] * inner
    if need_dw:
        dw = _col_sum(d32 * xhat)
    if need_db:
        db = _col_sum(d32)
    return dx, dw, db


def mx_norm_backward(dxhat: torch.Tensor, x: torch.Tensor, rstd: torch.Tensor, mean: Optional[torch.Tensor] = None,
                     weight: Optional[torch.Tensor] = None, *, norm: str = "rms", need_dx: bool = True, need_dweight: bool = True,
                     need_dbias: bool = True, dresidual: Optional[torch.Tensor] = None):
    """The backward of the normalisation ``y = norm(x) * weight (+ bias)`` that ``mx_norm_quantize`` computes, over the last dimension
    of ``x [..., C]``: ``dxhat [..., C]`` (float32 / bfloat16 / float16) is the gradient with respect to ``y``, ``rstd`` / ``mean``
    (float32, shaped ``x.shape[:-1]``; ``mean`` in layer mode only) are ``mx_norm_quantize(..., return_stats=True)``'s, ``weight`` is
    ``[C]`` or None (ones).  Returns ``(dx, dweight, dbias)`` -- ``dx`` shaped and typed as ``x``, the other two float32 ``[C]`` -- with
    None where ``need_dx`` / ``need_dweight`` / ``need_dbias`` is False; an output that is asked for does not depend on the others.
    All arithmetic is float32, ``xhat`` as the forward forms it:

        xhat = (x - mean) * rstd   (x * rstd in rms mode),   g = dxhat * weight
        c1 = sum_C(g * xhat) / C,   c2 = sum_C(g) / C
        rms     dx = rstd * (g - xhat * c1)
        layer   dx = rstd * ((g - xhat * c1) - c2)                      rounded once to x's dtype
        dweight = sum_R(dxhat * xhat),   dbias = sum_R(dxhat)

    with every sum in one fixed order: the row sums in ``mx_norm_quantize``'s (a function of ``C`` alone), the column sums in row tiles
    of 128 -- 16 strided partial sums and a pairwise tree per tile, 128 strided partial sums and a pairwise tree over the tiles (a
    function of ``R`` alone).  So the bits are the same on the CPU and on the GPU, on every run (no atomics), for every dtype and
    whatever is asked for; they are NOT those of torch's own reductions.  NaN and Inf propagate: a row whose ``rstd`` is NaN has a NaN
    ``dx`` and makes ``dweight`` NaN.  GPU tensors take the HIP kernels of ``qs_mx_norm_bwd_v`` (no fallback), CPU tensors the torch
    expression of the definition.  Nothing here is differentiable.

    ``dresidual`` (shape, dtype and device of ``x``; needs ``need_dx``) is the gradient that reaches the norm's input by the residual
    stream of a pre-norm block: ``dx = (the float32 value above) + dresidual.float()``, one more float32 addition IN FRONT of the one
    rounding to ``x``'s dtype -- not ``dx`` rounded and then added.  On the GPU it is loaded and added by the kernel that writes ``dx``
    (``qs_mx_norm_bwd_res_v``), in place of a ``torch.add`` pass over ``[..., C]``.  ``dweight`` and ``dbias`` do not see it."""
    weight, _ = _check_norm_args(x, weight, None, norm, 0.0)
    if not isinstance(dxhat, torch.Tensor):
        raise TypeError(f"dxhat must be a tensor, got {type(dxhat).__name__}")
    _check_dtype("dxhat", dxhat.dtype)
    if dxhat.shape != x.shape:
        raise ValueError(f"dxhat has shape {tuple(dxhat.shape)}, expected x's {tuple(x.shape)}")
    if norm == "layer" and mean is None:
        raise ValueError("norm='layer' needs mean: the second statistic of mx_norm_quantize(..., return_stats=True)")
    stats = (("rstd", rstd),) + ((("mean", mean),) if norm == "layer" else ())
    for name, t in stats:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.shape != x.shape[:-1]:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(x.shape[:-1])}: one value per row of x {tuple(x.shape)}")
    if dresidual is not None:
        if not isinstance(dresidual, torch.Tensor):
            raise TypeError(f"dresidual must be a tensor, got {type(dresidual).__name__}")
        if dresidual.dtype != x.dtype:
            raise TypeError(f"dresidual must have x's dtype {x.dtype}, got {dresidual.dtype}")
        if dresidual.shape != x.shape:
            raise ValueError(f"dresidual has shape {tuple(dresidual.shape)}, expected x's {tuple(x.shape)}")
        if not need_dx:
            raise ValueError("dresidual is added to dx: it needs need_dx=True")
        stats += (("dresidual", dresidual),)
    for name, t in (("dxhat", dxhat),) + stats:
        if t.device != x.device:
            raise ValueError(f"x is on {x.device} but {name} on {t.device}")
    C = x.shape[-1]
    x2, d2 = x.detach().reshape(-1, C), dxhat.detach().reshape(-1, C)
    rstd1 = rstd.detach().reshape(-1)
    mean1 = mean.detach().reshape(-1) if norm == "layer" else None
    r2 = None if dresidual is None else dresidual.detach().reshape(-1, C)
    if x.is_cuda:
        dx, dw, db = _hip.mx_norm_bwd(d2.contiguous(), x2.contiguous(), rstd1.contiguous(), None if mean1 is None else mean1.contiguous(),
                                      weight, norm, need_dx, need_dweight, need_dbias, None if r2 is None else r2.contiguous())
    else:
        dx, dw, db = _mx_norm_backward_f32(d2, x2, rstd1, mean1, weight, need_dx, need_dweight, need_dbias)
        if r2 is not None:
            dx = dx + r2.to(torch.float32)
        dx = None if dx is None else dx.to(x.dtype)
    return None if dx is None else dx.reshape(x.shape), dw, db


MX_NORM_BACKWARDS = ("torch", "fused")


def _check_norm_backward(norm_backward):
    if norm_backward not in MX_NORM_BACKWARDS:
        raise ValueError(f"unknown norm_backward {norm_backward!r}: one of {MX_NORM_BACKWARDS}")


def _norm_linear_forward(ctx, h, res, norm_weight, norm_bias, weight, bias, norm, x_fmt, w_fmt, grad_fmt, need_col, grad_rounding, seed,
                         step, wgrad_split_k, norm_backward):
    """what the forwards of ``mx_norm_linear`` and ``mx_add_norm_linear`` share behind the normalising quantizer: ``res`` is its result
    (``return_stats=True``) for the norm's input ``h [R, K]``.  The product, and what the backward keeps; returns ``y [R, N]`` in
    ``h.dtype``"""
    x_row, x_rs = res[:2]
    x_col, x_cs = res[2:4] if need_col else (None, None)
    rstd, mean = res[-2:]
    w_row, w_rs, _, _ = mx_quantize_2way(weight, w_fmt, None)
    b32 = None if bias is None else bias.detach().to(torch.float32)
    y = mx_matmul(x_row, x_rs, x_fmt, w_row, w_rs, w_fmt, b32, h.dtype)
    ctx.save_for_backward(h, norm_weight, weight, rstd, mean, x_col, x_cs)
    _save_train_ctx(ctx, (x_fmt, w_fmt, grad_fmt), (grad_rounding, seed, step), wgrad_split_k, h, bias)
    ctx.norm, ctx.norm_backward = norm, norm_backward
    ctx.norm_dtypes = tuple(None if t is None else t.dtype for t in (norm_weight, norm_bias))
    return y


def _norm_linear_backward(ctx, dy, needs, dh_in=None):
    """the backward the two functions share.  ``needs``: (the norm's input, norm_weight, norm_bias, weight, bias); ``dh_in`` (None, or
    shaped and typed as the norm's input ``h [R, K]``) is what reaches ``h`` from its other users and is added to the norm's float32
    input gradient in front of its one rounding.  Returns (dh [R, K] in h's dtype, d norm_weight, d norm_bias, dW, db)"""
    h, norm_weight, weight, rstd, mean, x_col, x_cs = ctx.saved_tensors
    x_fmt, w_fmt, grad_fmt = ctx.fmts
    need_dx, need_dnw, need_dnb, need_dw, need_db = needs
    need_dxhat = need_dx or need_dnw or need_dnb
    N, K = weight.shape
    dy2 = dy.reshape(-1, N).contiguous()
    h2 = h.reshape(-1, K)
    dx = dnw = dnb = dw = db = None
    if need_dxhat or need_dw:
        g_row, g_rs, g_col, g_cs = _quantize_grad(ctx, lambda *sr: mx_quantize_2way(dy2, grad_fmt if need_dxhat else None,
                                                                                     grad_fmt if need_dw else None, *sr))
    if need_dxhat:
        _, _, w_col, w_cs = mx_quantize_2way(weight, None, w_fmt)
        dxhat = mx_matmul(g_row, g_rs, grad_fmt, w_col, w_cs, w_fmt, None, torch.float32)
        dres = dh_in if need_dx else None
        if ctx.norm_backward == "fused":
            dx, dnw, dnb = mx_norm_backward(dxhat, h2, rstd, mean, norm_weight, norm=ctx.norm, need_dx=need_dx, need_dweight=need_dnw,
                                            need_dbias=need_dnb, dresidual=dres)
        else:
            dx, dnw, dnb = _norm_backward(dxhat, _norm_xhat(h2, rstd, mean), rstd, norm_weight, ctx.norm, need_dx, need_dnw, need_dnb)
            if dres is not None:
                dx = dx + dres.to(torch.float32)
        dx = None if dx is None else dx.to(ctx.x_dtype)
        dnw = None if dnw is None else dnw.to(ctx.norm_dtypes[0])
        dnb = None if dnb is None else dnb.to(ctx.norm_dtypes[1])
    if need_dw:
        dw = mx_matmul(g_col, g_cs, grad_fmt, x_col, x_cs, x_fmt, None, weight.dtype, split_k=ctx.wgrad_split_k)
    if need_db:
        db = dy2.sum(0, dtype=torch.float32).to(ctx.bias_dtype)
    return dx, dnw, dnb, dw, db


class _MXNormLinearFunction(torch.autograd.Function):
    """y = Q(norm(x)) Q(W)^T + b; the linear part's three products as ``_MXLinearFunction``'s, the norm's backward in float32"""

    @staticmethod
    def forward(ctx, x, norm_weight, norm_bias, weight, bias, norm, eps, x_fmt, w_fmt, grad_fmt, need_col, grad_rounding="nearest",
                seed=0, step=None, wgrad_split_k=1, norm_backward="torch"):
        N, K = weight.shape
        x2 = x.reshape(-1, K)
        res = mx_norm_quantize(x2, norm_weight, norm_bias, norm=norm, eps=eps, fmt=x_fmt, col_fmt=x_fmt if need_col else None,
                               return_stats=True)
        y = _norm_linear_forward(ctx, x, res, norm_weight, norm_bias, weight, bias, norm, x_fmt, w_fmt, grad_fmt, need_col, grad_rounding,
                                 seed, step, wgrad_split_k, norm_backward)
        return y.reshape(x.shape[:-1] + (N,))

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x = ctx.saved_tensors[0]
        dx, dnw, dnb, dw, db = _norm_linear_backward(ctx, dy, ctx.needs_input_grad[:5])
        return (None if dx is None else dx.reshape(x.shape), dnw, dnb, dw, db) + (None,) * 11


class _MXAddNormLinearFunction(torch.autograd.Function):
    """h = x + residual, y = Q(norm(h)) Q(W)^T + b: two outputs; the backward is ``_MXNormLinearFunction``'s with the gradient that
    reaches ``h`` from its other users added to the norm's input gradient in front of its one rounding"""

    @staticmethod
    def forward(ctx, x, residual, norm_weight, norm_bias, weight, bias, norm, eps, x_fmt, w_fmt, grad_fmt, need_col, grad_rounding, seed,
                step, wgrad_split_k, norm_backward):
        N, K = weight.shape
        res = mx_add_norm_quantize(x.reshape(-1, K), residual.reshape(-1, K), norm_weight, norm_bias, norm=norm, eps=eps, fmt=x_fmt,
                                   col_fmt=x_fmt if need_col else None, return_stats=True)
        h = res[0]
        y = _norm_linear_forward(ctx, h, res[1:], norm_weight, norm_bias, weight, bias, norm, x_fmt, w_fmt, grad_fmt, need_col,
                                 grad_rounding, seed, step, wgrad_split_k, norm_backward)
        ctx.in_dtype, ctx.in_shape = x.dtype, x.shape
        ctx.set_materialize_grads(False)        # (an h nobody else used has no incoming gradient: no tensor of zeros is added)
        return y.reshape(x.shape[:-1] + (N,)), h.reshape(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, dh_in):
        need_x, need_res = ctx.needs_input_grad[:2]
        h, weight = ctx.saved_tensors[0], ctx.saved_tensors[2]
        if dy is None:                          # (only h was used: the product's gradients are those of a zero dy)
            dy = torch.zeros(ctx.in_shape[:-1] + (weight.shape[0],), dtype=h.dtype, device=h.device)
        if dh_in is not None:
            dh_in = dh_in.reshape(h.shape).contiguous()
        dh, dnw, dnb, dw, db = _norm_linear_backward(ctx, dy, (need_x or need_res,) + tuple(ctx.needs_input_grad[2:6]), dh_in)
        dh = None if dh is None else dh.reshape(ctx.in_shape)
        dx = dh.to(ctx.in_dtype) if need_x else None
        return (dx, dh if need_res else None, dnw, dnb, dw, db) + (None,) * 11


def _check_norm_linear(x, norm_weight, norm_bias, weight, bias, norm, eps, fmts, grad_rounding, step, wgrad_split_k, norm_backward) -> bool:
    """the operands and options of ``mx_norm_linear``; returns whether the forward has to produce the col pair"""
    _check_train_entry(x, weight, bias, fmts, grad_rounding, step, wgrad_split_k)
    if weight.dim() != 2:
        raise ValueError(f"weight must be [N, K], got shape {tuple(weight.shape)}")
    if x.dim() < 1 or x.shape[-1] != weight.shape[1]:
        raise ValueError(f"x {tuple(x.shape)} and weight {tuple(weight.shape)} disagree on K (their last dimensions)")
    _check_norm_args(x, norm_weight, norm_bias, norm, eps)
    _check_bias_shape(bias, weight.shape[0])
    _check_norm_backward(norm_backward)
    return torch.is_grad_enabled() and weight.requires_grad


def mx_norm_linear(x: torch.Tensor, norm_weight: Optional[torch.Tensor], norm_bias: Optional[torch.Tensor], weight: torch.Tensor,
                   bias: Optional[torch.Tensor] = None, *, norm: str = "rms", eps: float = 1e-6, x_fmt: str = "mxfp8_e4m3",
                   w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest", seed: int = 0,
                   step: Optional[torch.Tensor] = None, wgrad_split_k="auto", norm_backward: str = "torch") -> torch.Tensor:
    """``mx_linear(norm(x) * norm_weight (+ norm_bias), weight, bias)`` without the float tensor between the two, differentiable in
    all five tensors.  ``x`` is ``[..., K]``, ``norm_weight`` / ``norm_bias`` ``[K]`` or None, ``weight`` ``[N, K]``, ``bias`` ``[N]``;
    the result is ``[..., N]`` in ``x.dtype``.  The forward is ONE ``mx_norm_quantize`` call -- the row pair for the product, the
    statistics and, only when a weight gradient can be asked for, the col pair -- and ``mx_matmul``; its bits are ``mx_linear``'s
    on the definition's float32 ``y``.  The backward keeps ``x``, ``rstd``, ``mean`` and the col pair.  With ``dy`` the incoming
    gradient and ``Q`` as in ``mx_linear``:

        dW    = Q_g(dy^T) Q_x(y^T)^T,   db = sum over rows of dy             ``mx_linear``'s, bit for bit
        dxhat = Q_g(dy) Q_w(W^T)^T                                           float32: the gradient with respect to the norm's output
        xhat  = (x - mean) * rstd                                            (x * rstd in rms mode), float32
        g     = dxhat * norm_weight
        rms     dx = rstd * (g - xhat * mean_C(g * xhat))
        layer   dx = rstd * ((g - xhat * mean_C(g * xhat)) - mean_C(g))
        d norm_weight = sum_R(dxhat * xhat),   d norm_bias = sum_R(dxhat)

    With ``norm_backward="torch"`` (the default) the normalisation's backward is torch float32 ops on ``[R, K]`` tensors -- not fused;
    its sums are torch's own ``mean(-1)`` / ``sum(0)``.  ``norm_backward="fused"`` hands it to ``mx_norm_backward``: the same formulas
    in up to three HIP launches on the GPU, with the sums in that function's fixed order -- other last bits than torch's, the same on
    the CPU and the GPU.  The forward, ``dW`` and ``db`` do not depend on it.  Either way each result is cast once to its tensor's
    dtype.  Gradients nobody asks for are not computed; without grad the col pair is not produced.  ``grad_rounding``, ``seed``,
    ``step`` and ``wgrad_split_k`` are ``mx_linear``'s and touch the two forms of ``dy`` and the ``dW`` product alone."""
    need_col = _check_norm_linear(x, norm_weight, norm_bias, weight, bias, norm, eps, (x_fmt, w_fmt, grad_fmt), grad_rounding, step,
                                  wgrad_split_k, norm_backward)
    return _MXNormLinearFunction.apply(x, norm_weight, norm_bias, weight, bias, norm, float(eps), x_fmt, w_fmt, grad_fmt, need_col,
                                       grad_rounding, seed, step, wgrad_split_k, norm_backward)


class MXTrainNormLinear(_MXTrainMixin, nn.Module):
    """A normalisation and the linear layer behind it as one training layer: ``forward`` is ``mx_norm_linear``.  The parameters are
    ``norm_weight`` / ``norm_bias`` (``[in_features]``; None where the norm has none) and ``weight`` / ``bias`` as ``nn.Linear``'s.
    ``norm`` is ``"rms"`` or ``"layer"``; ``eps=None`` is the machine epsilon of the input's dtype (``nn.RMSNorm``'s rule).  The
    ``norm_backward`` is ``mx_norm_linear``'s: ``"torch"`` (the default) or ``"fused"``, the HIP kernels of ``mx_norm_backward``.  The
    options, the stochastic-rounding seed and counter and the autocast behaviour are ``MXTrainLinear``'s."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, norm: str = "rms", eps: Optional[float] = 1e-6,
                 elementwise_affine: bool = True, norm_bias: bool = True, device=None, dtype=None, x_fmt: str = "mxfp8_e4m3",
                 w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest", seed: Optional[int] = None,
                 wgrad_split_k="auto", norm_backward: str = "torch"):
        super().__init__()
        if norm not in MX_NORMS:
            raise ValueError(f"unknown norm {norm!r}: one of {MX_NORMS}")
        _check_norm_backward(norm_backward)
        self.in_features, self.out_features, self.norm, self.eps = in_features, out_features, norm, eps
        self.norm_backward = norm_backward
        lin = nn.Linear(in_features, out_features, bias=bias, device=device, dtype=dtype)
        self.weight, self.bias = lin.weight, lin.bias
        kw = dict(device=device, dtype=dtype)
        self.register_parameter("norm_weight", nn.Parameter(torch.ones(in_features, **kw)) if elementwise_affine else None)
        self.register_parameter("norm_bias", nn.Parameter(torch.zeros(in_features, **kw))
                                if elementwise_affine and norm_bias and norm == "layer" else None)
        self._init_mx(dict(x_fmt=x_fmt, w_fmt=w_fmt, grad_fmt=grad_fmt), grad_rounding, seed)
        self._init_split(wgrad_split_k)

    @classmethod
    def from_float(cls, norm_module: nn.Module, linear: nn.Linear, x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3",
                   grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest", seed: Optional[int] = None, wgrad_split_k="auto",
                   norm_backward: str = "torch"):
        """a layer on the two modules' own parameters (shared, not copied): ``linear(norm_module(x))``"""
        norm = _norm_kind(norm_module)
        if not isinstance(linear, nn.Linear):
            raise TypeError(f"MXTrainNormLinear.from_float needs an nn.Linear, got {type(linear).__name__}")
        if _last_dim(norm_module.normalized_shape) != linear.in_features:
            raise ValueError(f"normalized_shape {tuple(norm_module.normalized_shape)} does not match in_features {linear.in_features}")
        self = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, norm=norm, eps=norm_module.eps,
                   elementwise_affine=False, device="meta", x_fmt=x_fmt, w_fmt=w_fmt, grad_fmt=grad_fmt, grad_rounding=grad_rounding,
                   seed=seed, wgrad_split_k=wgrad_split_k, norm_backward=norm_backward)._adopt(linear)
        self.norm_weight, self.norm_bias = norm_module.weight, getattr(norm_module, "bias", None)
        return self

    def extra_repr(self) -> str:
        sr = f", grad_rounding={self.grad_rounding!r}" if self.grad_rounding != "nearest" else ""
        split = f", wgrad_split_k={self.wgrad_split_k!r}" if self.wgrad_split_k != "auto" else ""
        nb = f", norm_backward={self.norm_backward!r}" if self.norm_backward != "torch" else ""
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, norm={self.norm!r}, "
                f"eps={self.eps}, x_fmt={self.x_fmt!r}, w_fmt={self.w_fmt!r}, grad_fmt={self.grad_fmt!r}{sr}{split}{nb}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x, seed, step = self._mx_input(x)
        return mx_norm_linear(x, self.norm_weight, self.norm_bias, self.weight, self.bias, norm=self.norm, eps=_eps_of(self.eps, x),
                              x_fmt=self.x_fmt, w_fmt=self.w_fmt, grad_fmt=self.grad_fmt, grad_rounding=self.grad_rounding, seed=seed,
                              step=step, wgrad_split_k=self.wgrad_split_k, norm_backward=self.norm_backward)

    def to_inference(self, out_dtype: torch.dtype = torch.float32) -> nn.Sequential:
        """``nn.Sequential(MXRMSNorm | MXLayerNorm, MXLinear)`` on the current parameters: the norm (sharing this layer's) hands the
        codes the training forward multiplies to an ``MXLinear`` that holds the weight's row pair -- the same bits as this layer's
        forward for an input of dtype ``out_dtype``"""
        cls = MXRMSNorm if self.norm == "rms" else MXLayerNorm
        head = cls(self.in_features, self.eps, elementwise_affine=False, out_fmt=self.x_fmt)
        head.elementwise_affine = self.norm_weight is not None
        head.weight = self.norm_weight
        if self.norm == "layer":
            head.bias = self.norm_bias
        codes, scales, _, _ = mx_quantize_2way(self.weight, self.w_fmt, None)
        return nn.Sequential(head, MXLinear(codes, scales, self.w_fmt, None if self.bias is None else self.bias.detach(), self.x_fmt,
                                            out_dtype))


def mx_add_norm_linear(x: torch.Tensor, residual: torch.Tensor, norm_weight: Optional[torch.Tensor], norm_bias: Optional[torch.Tensor],
                       weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, norm: str = "rms", eps: float = 1e-6,
                       x_fmt: str = "mxfp8_e4m3", w_fmt: str = "mxfp8_e4m3", grad_fmt: str = "mxfp8_e5m2", grad_rounding: str = "nearest",
                       seed: int = 0, step: Optional[torch.Tensor] = None, wgrad_split_k="auto", norm_backward: str = "fused"):
    """The head of a pre-norm block as one differentiable function: ``h = x + residual`` (``x`` the previous branch's output,
    ``residual`` the stream, same shape; ``h`` in ``residual.dtype``, one float32 addition rounded once) and
    ``y = mx_norm_linear(h, norm_weight, norm_bias, weight, bias, ...)``.  Returns ``(y, h)``: ``y [..., N]`` in ``h``'s dtype with
    ``mx_norm_linear(h, ...)``'s bits, and the new stream for the next add.  The forward is ``mx_add_norm_quantize`` and ``mx_matmul``.
    The backward receives ``dy`` and ``dh_in``, what reaches ``h`` from its other users (None when nobody used it):

        dh = (mx_norm_linear's float32 input gradient) + dh_in        rounded once to h's dtype

    With ``norm_backward="fused"`` (the default HERE: nothing pins this function to torch's reduction order) that is
    ``mx_norm_backward(..., dresidual=dh_in)``, the addition in the kernel that writes ``dx``; with ``"torch"`` it is
    ``_norm_backward`` in float32, ``+ dh_in.float()``, one cast.  The gradient of ``residual`` is ``dh``, that of ``x`` is ``dh``
    too (``dh.to(x.dtype)`` where the dtypes differ: a torch op).  ``dW``, ``db``, ``d norm_weight`` and ``d norm_bias`` are exactly
    ``mx_norm_linear``'s, as are the remaining options."""
    need_col = _check_norm_linear(x, norm_weight, norm_bias, weight, bias, norm, eps, (x_fmt, w_fmt, grad_fmt), grad_rounding, step,
                                  wgrad_split_k, norm_backward)
    _check_residual(x, residual)
    return _MXAddNormLinearFunction.apply(x, residual, norm_weight, norm_bias, weight, bias, norm, float(eps), x_fmt, w_fmt, grad_fmt,
                                          need_col, grad_rounding, seed, step, wgrad_split_k, norm_backward)


class MXAddNormLinear(nn.Module):
    """What ``MXTrainAddNormLinear.to_inference()`` returns: ``forward(x, residual) -> (y, h)`` from an ``MXRMSNorm`` / ``MXLayerNorm``
    called with the residual (``norm``) and the ``MXLinear`` behind it (``linear``)"""

    def __init__(self, norm: nn.Module, linear: nn.Module):
        super().__init__()
        self.norm, self.linear = norm, linear

    def forward(self, x: torch.Tensor, residual: torch.Tensor):
        act, h = self.norm(x, residual)
        return self.linear(act), h


class MXTrainAddNormLinear(MXTrainNormLinear):
    """``MXTrainNormLinear`` with the residual add of a pre-norm block in front: ``forward(x, residual) -> (y, h)`` is
    ``mx_add_norm_linear``.  The constructor, ``from_float``, the parameters and the ``state_dict`` are ``MXTrainNormLinear``'s, except
    that ``norm_backward`` defaults to ``"fused"``."""

    def __init__(self, *args, norm_backward: str = "fused", **kw):
        super().__init__(*args, norm_backward=norm_backward, **kw)

    @classmethod
    def from_float(cls, norm_module: nn.Module, linear: nn.Linear, *args, norm_backward: str = "fused", **kw):
        return super().from_float(norm_module, linear, *args, norm_backward=norm_backward, **kw)

    def forward(self, x: torch.Tensor, residual: torch.Tensor):
        x, seed, step = self._mx_input(x)
        return mx_add_norm_linear(x, residual, self.norm_weight, self.norm_bias, self.weight, self.bias, norm=self.norm,
                                  eps=_eps_of(self.eps, residual), x_fmt=self.x_fmt, w_fmt=self.w_fmt, grad_fmt=self.grad_fmt,
                                  grad_rounding=self.grad_rounding, seed=seed, step=step, wgrad_split_k=self.wgrad_split_k,
                                  norm_backward=self.norm_backward)

    def to_inference(self, out_dtype: torch.dtype = torch.float32) -> MXAddNormLinear:
        """``MXAddNormLinear`` on the current parameters: the same ``(y, h)`` bits as this layer's forward for a stream of dtype
        ``out_dtype``"""
        head, linear = super().to_inference(out_dtype)
        return MXAddNormLinear(head, linear)


__all__ = ["mx_norm_quantize", "mx_add_norm_quantize", "mx_norm_backward", "MXRMSNorm", "MXLayerNorm", "mx_norm_linear",
           "mx_add_norm_linear", "MXTrainNormLinear", "MXTrainAddNormLinear", "MXAddNormLinear", "MX_NORMS", "MX_NORM_BACKWARDS"]
