"""Matrix products on MX codes: ``mx_matmul`` and the inference-side layer ``MXLinear``.

``quantize_with_mx(..., block_dim=-1, return_codes=True)`` and ``export_integer`` hand out the bytes of an MX tensor -- one code
per element, one E8M0 scale per block of 32 along K.  ``mx_matmul`` computes ``A . B^T`` directly on those bytes: on the GPU
through the block-scaled MFMA of gfx950 (``qs_mx_matmul_v``: FP8 / FP6 / FP4 operands of either format on either side, float32
accumulation), on the CPU by evaluating the definition in float64.  Training keeps using the simulated layers
(``quantize(nn.Linear(...), callback=MXQuantizer(...))``); ``MXLinear`` is what such a layer becomes for inference."""
from typing import Optional

import torch
import torch.nn as nn

from qsparse_amd import _hip
from qsparse_amd.quantize import MX_BLOCK, MX_FORMATS, MXQuantizer, _mx_format, mx_dequantize, quantize_with_mx

_OUT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _check_operand(name: str, codes: torch.Tensor, scales: torch.Tensor, fmt: str):
    _mx_format(fmt)
    for what, t in ((f"{name}_codes", codes), (f"{name}_scales", scales)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.uint8:
            raise TypeError(f"{what} must be uint8 (the bytes quantize_with_mx(..., return_codes=True) returns), got {t.dtype}")
    if codes.dim() < 2 and name == "b" or codes.dim() < 1:
        raise ValueError(f"{name}_codes needs {'2 dimensions [N, K]' if name == 'b' else 'at least one dimension [..., K]'}, "
                         f"got shape {tuple(codes.shape)}")
    K = codes.shape[-1]
    want = tuple(codes.shape[:-1]) + ((K + MX_BLOCK - 1) // MX_BLOCK,)
    if tuple(scales.shape) != want:
        raise ValueError(f"{name}_scales has shape {tuple(scales.shape)}, expected {want}: one E8M0 byte per block of {MX_BLOCK} "
                         f"along the last dimension of {name}_codes {tuple(codes.shape)}")
    if scales.device != codes.device:
        raise ValueError(f"{name}_codes is on {codes.device} but {name}_scales on {scales.device}")


def mx_matmul(a_codes: torch.Tensor, a_scales: torch.Tensor, a_fmt: str, b_codes: torch.Tensor, b_scales: torch.Tensor, b_fmt: str,
              bias: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``A . B^T (+ bias)`` on MX codes.  ``a_codes`` ``[..., K]`` and ``b_codes`` ``[N, K]`` (an ``nn.Linear`` weight) are uint8
    codes of the formats ``a_fmt`` / ``b_fmt`` (``MX_FORMATS``; they may differ) with blocks along K, ``a_scales`` ``[..., ceil(K /
    32)]`` and ``b_scales`` ``[N, ceil(K / 32)]`` their E8M0 bytes, ``bias`` float32 ``[N]``.  Returns ``[..., N]`` in ``out_dtype``
    (float32, bfloat16 or float16):

        y[m, n] = round( sum_k val(a[m, k]) 2^(sa[m, k / 32] - 127) val(b[n, k]) 2^(sb[n, k / 32] - 127) + bias[n] )

    with ``val`` the value of a code as ``mx_dequantize`` decodes it.  A scale byte 0xFF (a block that held NaN / Inf) makes every
    output that reads it NaN.  GPU tensors take the HIP kernel (float32 accumulation; there is no fallback: without the library
    the call raises), CPU tensors evaluate the expression above in float64 and round once."""
    _check_operand("a", a_codes, a_scales, a_fmt)
    _check_operand("b", b_codes, b_scales, b_fmt)
    if b_codes.dim() != 2:
        raise ValueError(f"b_codes must be [N, K], got shape {tuple(b_codes.shape)}")
    K, N = a_codes.shape[-1], b_codes.shape[0]
    if b_codes.shape[1] != K:
        raise ValueError(f"a_codes {tuple(a_codes.shape)} and b_codes {tuple(b_codes.shape)} disagree on K (their last dimensions)")
    if K < 1:
        raise ValueError("mx_matmul needs K >= 1")
    if b_codes.device != a_codes.device:
        raise ValueError(f"a_codes is on {a_codes.device} but b_codes on {b_codes.device}")
    if out_dtype not in _OUT_DTYPES:
        raise TypeError(f"out_dtype must be one of {_OUT_DTYPES}, got {out_dtype}")
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
            raise TypeError("bias must be a float32 tensor")
        if tuple(bias.shape) != (N,):
            raise ValueError(f"bias has shape {tuple(bias.shape)}, expected ({N},)")
        if bias.device != a_codes.device:
            raise ValueError(f"a_codes is on {a_codes.device} but bias on {bias.device}")
    lead = tuple(a_codes.shape[:-1])
    a2, sa2 = a_codes.reshape(-1, K), a_scales.reshape(-1, a_scales.shape[-1])
    if a_codes.is_cuda:
        y = _hip.mx_matmul(a2.contiguous(), sa2.contiguous(), a_fmt, b_codes.contiguous(), b_scales.contiguous(), b_fmt,
                           None if bias is None else bias.contiguous(), out_dtype)
    else:
        a = mx_dequantize(a2, sa2, a_fmt, -1, torch.float64)
        b = mx_dequantize(b_codes, b_scales, b_fmt, -1, torch.float64)
        # a 0xFF block is NaN in every product that reads it, also against a zero (NaN * 0 is NaN): matmul's own propagation
        y = a @ b.t()
        if bias is not None:
            y = y + bias.to(torch.float64)
        y = y.to(out_dtype)
    return y.reshape(lead + (N,))


class MXLinear(nn.Module):
    """``nn.Linear`` for inference on MX codes: the weight is held as uint8 codes ``weight_codes [N, K]`` and E8M0 scales
    ``weight_scales [N, ceil(K / 32)]`` of the format ``weight_fmt`` (buffers, with the optional float32 ``bias``); ``forward``
    quantizes its input to ``act_fmt`` along the last dimension with the MX quantizer (``quantize_with_mx``) and multiplies the two
    sets of codes with ``mx_matmul``.  The output is float32 (or ``out_dtype``) and never requires grad; an input that requires
    grad while gradients are enabled is refused -- training runs on the simulated layers this one is built from."""

    def __init__(self, weight_codes: torch.Tensor, weight_scales: torch.Tensor, weight_fmt: str, bias: Optional[torch.Tensor] = None,
                 act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32):
        super().__init__()
        _mx_format(act_fmt)
        _check_operand("b", weight_codes, weight_scales, weight_fmt)
        if weight_codes.dim() != 2:
            raise ValueError(f"weight_codes must be [N, K], got shape {tuple(weight_codes.shape)}")
        if bias is not None and tuple(bias.shape) != (weight_codes.shape[0],):
            raise ValueError(f"bias has shape {tuple(bias.shape)}, expected ({weight_codes.shape[0]},)")
        self.weight_fmt, self.act_fmt, self.out_dtype = weight_fmt, act_fmt, out_dtype
        self.out_features, self.in_features = weight_codes.shape
        self.register_buffer("weight_codes", weight_codes.detach().clone().contiguous())
        self.register_buffer("weight_scales", weight_scales.detach().clone().contiguous())
        self.register_buffer("bias", None if bias is None else bias.detach().to(torch.float32).clone().contiguous())

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"weight_fmt={self.weight_fmt!r}, act_fmt={self.act_fmt!r}")

    @classmethod
    def from_exported(cls, qt, bias: Optional[torch.Tensor] = None, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32):
        """from the ``QuantizedTensor(kind="mx")`` ``export_integer`` returns for a linear layer's weight"""
        if getattr(qt, "kind", None) != "mx":
            raise ValueError(f"MXLinear needs an MX weight (QuantizedTensor.kind == 'mx'), got kind {getattr(qt, 'kind', None)!r}")
        if qt.codes.dim() != 2:
            raise ValueError(f"MXLinear needs a 2-d weight [N, K], got shape {tuple(qt.codes.shape)}")
        if qt.block_dim % qt.codes.dim() != 1:
            raise ValueError(f"the weight's MX blocks run along dim {qt.block_dim}, not along K (dim 1): blocks along N cannot feed the "
                             "matrix instruction -- quantize the layer with MXQuantizer(fmt, block_dim=1)")
        return cls(qt.codes, qt.block_scale, qt.fmt, bias, act_fmt, out_dtype)

    @classmethod
    def from_quantized(cls, layer: nn.Module, act_fmt: str = "mxfp8_e4m3", out_dtype: torch.dtype = torch.float32):
        """from a ``quantize(nn.Linear(...), bits=w, callback=MXQuantizer(fmt, block_dim=1))`` layer that is past its timeout:
        the weight codes are the export's, the bias what the layer's evaluation-mode forward adds"""
        from qsparse_amd.export import export_integer
        q = layer.__dict__.get("_modules", {}).get("quantize")
        if not isinstance(layer, nn.Linear) or q is None or not isinstance(q.callback, MXQuantizer):
            raise ValueError("MXLinear.from_quantized needs an nn.Linear wrapped by quantize(..., callback=MXQuantizer(...))")
        rec = export_integer(nn.Sequential(layer)).get("0")
        if rec is None or rec.weight is None:
            raise ValueError("the layer has not quantized its weight yet (still inside its timeout): nothing to build an MXLinear from")
        was = layer.training
        layer.eval()
        try:
            with torch.no_grad():
                b = layer.bias
                bias = None if b is None else b.detach().to(torch.float32)
        finally:
            layer.train(was)
        return cls.from_exported(rec.weight, bias, act_fmt, out_dtype)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("MXLinear is an inference layer: its input requires grad.  Train with the simulated layer "
                               "(quantize(nn.Linear(...), callback=MXQuantizer(...))) or call it under torch.no_grad()")
        with torch.no_grad():
            _, codes, scales = quantize_with_mx(x, self.act_fmt, -1, return_codes=True)
            return mx_matmul(codes, scales, self.act_fmt, self.weight_codes, self.weight_scales, self.weight_fmt, self.bias, self.out_dtype)


__all__ = ["mx_matmul", "MXLinear", "MX_FORMATS"]
