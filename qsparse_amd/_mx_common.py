"""What the products on MX codes and their training layers say alike, stated once.  The inference modules (``mx_gemm.py``,
``mx_conv.py``, ``mx_conv_transpose.py``, ``mx_bmm.py``, ``mx_grouped.py``, ``mx_glu.py``) take the argument checks of an operand, of
``out_dtype``, of a bias and of the codes-out keywords, and ``MXActivation``; the training modules (``mx_gemm.py``, ``mx_conv_train.py``,
``mx_batched_train.py``, ``mx_grouped_train.py``, ``mx_glu_train.py``) the check of a training entry, the scaffold of their layers
(``_MXTrainMixin``: options, stochastic-rounding seed and counter, autocast) and the two steps their autograd functions share.
Private: the public modules import from here and keep their own shape messages."""
from typing import NamedTuple

import torch

from qsparse_amd.quantize import MX_BLOCK, _mx_check_rounding, _mx_format, mx_dequantize, quantize_with_mx

_OUT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_ACTS = (None, "relu")


class MXActivation(NamedTuple):
    """An activation as MX bytes, as the products hand it out with ``out_fmt`` and as ``MXLinear`` / ``MXConv2d`` take it in place of a
    float tensor: ``codes`` uint8 ``[..., N]``, ``scales`` uint8 E8M0 ``[..., ceil(N / 32)]`` with blocks of 32 along the last axis, the
    format name ``fmt``.  ``channels_last`` marks the activation of a convolution: ``codes`` is ``[B, H, W, C]`` and ``dequantize``
    returns the ``[B, C, H, W]`` view of it, the way ``MXConv2d`` returns a float tensor.  The layers check it: ``MXConv2d`` takes only
    an activation that has it set, ``MXLinear`` only one that has not."""
    codes: torch.Tensor
    scales: torch.Tensor
    fmt: str
    channels_last: bool = False

    def dequantize(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        y = mx_dequantize(self.codes, self.scales, self.fmt, -1, dtype)
        return y.permute(0, 3, 1, 2) if self.channels_last else y


def _check_codes_out(fn: str, out_fmt, act, out_dtype, split_request: int = 1):
    """the `out_fmt` / `act` keywords of the product `fn` against its other options"""
    if act not in _ACTS:
        raise ValueError(f"unknown act {act!r}: one of {_ACTS}")
    if out_fmt is None:
        if act is not None:
            raise ValueError(f"act={act!r} needs out_fmt: the activation is part of the quantizing epilogue, {fn} without out_fmt returns "
                             "the plain product")
        return
    _mx_format(out_fmt)
    if out_dtype is not torch.float32:
        raise ValueError(f"out_dtype={out_dtype} cannot be combined with out_fmt={out_fmt!r}: the result is MX codes, leave out_dtype at "
                         "its default")
    if split_request != 1:
        raise ValueError("split_k cannot be combined with out_fmt: the split product's reduction does not quantize, use split_k=1")


def _act(y: torch.Tensor, act) -> torch.Tensor:
    """`act` on a float tensor by the definition of the codes-out products: NaN stays NaN, everything else not positive becomes +0"""
    return y if act is None else torch.where(y > 0, y, torch.where(y != y, y, torch.zeros_like(y)))


def _codes_out_cpu(y32: torch.Tensor, out_fmt: str, act):
    """(codes, scales) of act(y32) by the CPU quantizer: the definition of the codes-out products on a float32 result"""
    return tuple(quantize_with_mx(_act(y32, act), out_fmt, -1, return_codes=True)[1:])


def _pair(name: str, v, least: int):
    """`v` as a pair of ints, each >= `least`"""
    if isinstance(v, str):
        raise ValueError(f"{name} must be an int or a pair of ints, got the string {v!r} (padding modes such as 'same' are not supported: "
                         "give the padding as numbers)")
    if isinstance(v, bool) or not isinstance(v, (int, tuple, list)):
        raise TypeError(f"{name} must be an int or a pair of ints, got {type(v).__name__}")
    p = (v, v) if isinstance(v, int) else tuple(v)
    if len(p) != 2 or any(isinstance(e, bool) or not isinstance(e, int) for e in p):
        raise ValueError(f"{name} must be an int or a pair of ints, got {v!r}")
    if min(p) < least:
        raise ValueError(f"{name} must be >= {least}, got {v!r}")
    return p


def _split_request(split_k, name: str = "split_k") -> int:
    """the slice count the C ABI takes for `split_k`: an int >= 1 as it is, "auto" as 0 (the library's rule)"""
    if isinstance(split_k, str):
        if split_k != "auto":
            raise ValueError(f'{name} must be an int >= 1 or "auto", got {split_k!r}')
        return 0
    if isinstance(split_k, bool) or not isinstance(split_k, int):
        raise TypeError(f'{name} must be an int >= 1 or "auto", got {type(split_k).__name__}')
    if not 1 <= split_k < 2 ** 31:
        raise ValueError(f'{name} must be an int >= 1 or "auto", got {split_k}')
    return split_k


def _check_operand(name: str, codes: torch.Tensor, scales: torch.Tensor, fmt: str, what: str, least: int = 4, most=4,
                   needs: str = "4 dimensions", source: str = "quantize_with_mx(..., return_codes=True)", axis: str = ""):
    """one MX operand `<name>_codes` / `<name>_scales` in the format `fmt`.  The codes have the layout `what`: `least` to `most` (None:
    any number of) dimensions, `needs` in the message; `source`: who hands such bytes out; `axis`: a note on the last axis.  It
    runs six times per training step, so a message is put together only where it is raised"""
    _mx_format(fmt)
    if not (isinstance(codes, torch.Tensor) and isinstance(scales, torch.Tensor) and codes.dtype == scales.dtype == torch.uint8):
        for kind, t in (("codes", codes), ("scales", scales)):      # which of the two, and why
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name}_{kind} must be a tensor, got {type(t).__name__}")
            if t.dtype != torch.uint8:
                raise TypeError(f"{name}_{kind} must be uint8 (the bytes {source} returns), got {t.dtype}")
    if codes.dim() < least or most is not None and codes.dim() > most:
        raise ValueError(f"{name}_codes needs {needs} {what}, got shape {tuple(codes.shape)}")
    shape = tuple(codes.shape)
    want = shape[:-1] + ((shape[-1] + MX_BLOCK - 1) // MX_BLOCK,)
    if tuple(scales.shape) != want:
        raise ValueError(f"{name}_scales has shape {tuple(scales.shape)}, expected {want}: one E8M0 byte per block of {MX_BLOCK} "
                         f"along the last dimension{axis} of {name}_codes {shape}")
    if scales.device != codes.device:
        raise ValueError(f"{name}_codes is on {codes.device} but {name}_scales on {scales.device}")


def _check_dtype(name: str, dtype):
    if dtype not in _OUT_DTYPES:
        raise TypeError(f"{name} must be one of {_OUT_DTYPES}, got {dtype}")


def _check_bias_shape(bias, n: int):
    if bias is not None and tuple(bias.shape) != (n,):
        raise ValueError(f"bias has shape {tuple(bias.shape)}, expected ({n},)")


def _check_bias(bias, n: int, first: str, device):
    """the float32 bias `[n]` of a product whose first operand `first` (its name in the message) is on `device`"""
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
            raise TypeError("bias must be a float32 tensor")
        _check_bias_shape(bias, n)
        if bias.device != device:
            raise ValueError(f"{first} is on {device} but bias on {bias.device}")


def _check_train_entry(x, weight, bias, fmts, grad_rounding: str, step, wgrad_split_k, names=("x", "weight")):
    """what `mx_linear`, `mx_conv2d_train` and `mx_bmm_train` check before the shapes.  `names`: what the two operands are called in
    the messages; `wgrad_split_k` None: an entry without that option"""
    if wgrad_split_k is not None:
        _split_request(wgrad_split_k, "wgrad_split_k")
    for fmt in fmts:
        _mx_format(fmt)
    for name, t in ((names[0], x), (names[1], weight)) + ((("bias", bias),) if bias is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        _check_dtype(name, t.dtype)
        if t.device != x.device:
            raise ValueError(f"{names[0]} is on {x.device} but {name} on {t.device}")
    _mx_check_rounding(grad_rounding, step, x)


class _MXTrainMixin:
    """the scaffold of every layer that trains through MX products -- ``MXTrainLinear``, ``MXTrainConv2d``, ``MXTrainGroupedLinear``,
    ``MXTrainGLULinear``, ``MXTrainGroupedGLULinear``, ``MXTrainMultiheadAttention`` -- mixed in before the torch class they derive
    from.  ``_adopt`` and ``extra_repr`` are those of the first two, which own ``wgrad_split_k`` and derive from a torch layer"""

    def _check_mx(self, fmts: dict, dtypes: dict):
        """the formats, then the dtype options as the entries check them: ``out_dtype`` may be None (the input's)"""
        for fmt in fmts.values():
            _mx_format(fmt)
        for name, dtype in dtypes.items():
            if dtype is not None or name != "out_dtype":
                _check_dtype(name, dtype)

    def _init_mx(self, fmts: dict, grad_rounding: str, seed, weight=None, **dtypes):
        """check and keep the options every such layer has.  `fmts` and `dtypes` map attribute names to formats and dtype options;
        `weight`: the tensor whose device counts the backwards (default: ``self.weight``).  Under "stochastic" the layer gets
        ``sr_seed`` -- `seed`, or ONE draw from torch's default CPU generator -- and the non-persistent buffer ``sr_step``"""
        weight = self.weight if weight is None else weight
        self._check_mx(fmts, dtypes)
        _mx_check_rounding(grad_rounding, None, weight)
        for name, value in (*fmts.items(), *dtypes.items(), ("grad_rounding", grad_rounding)):
            setattr(self, name, value)
        if grad_rounding == "stochastic":
            self.sr_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if seed is None else int(seed)
            self.register_buffer("sr_step", torch.zeros(1, dtype=torch.int64, device=weight.device), persistent=False)

    def _init_split(self, wgrad_split_k):
        _split_request(wgrad_split_k, "wgrad_split_k")
        self.wgrad_split_k = wgrad_split_k

    def _adopt(self, layer):
        """take `layer`'s parameters (shared, not copied), count on its device and follow its mode; returns self"""
        self.weight, self.bias = layer.weight, layer.bias
        if self.grad_rounding == "stochastic":
            self.sr_step = torch.zeros(1, dtype=torch.int64, device=layer.weight.device)
        self.train(layer.training)
        return self

    def extra_repr(self) -> str:
        sr = f", grad_rounding={self.grad_rounding!r}" if self.grad_rounding != "nearest" else ""
        split = f", wgrad_split_k={self.wgrad_split_k!r}" if self.wgrad_split_k != "auto" else ""
        return f"{super().extra_repr()}, x_fmt={self.x_fmt!r}, w_fmt={self.w_fmt!r}, grad_fmt={self.grad_fmt!r}{sr}{split}"

    def _mx_sr(self):
        """(seed, step) for the functional form"""
        return (self.sr_seed, self.sr_step) if self.grad_rounding == "stochastic" else (0, None)

    def _mx_input(self, x: torch.Tensor):
        """(x in the autocast dtype, seed, step) for the functional form"""
        dev = x.device.type
        if torch.is_autocast_enabled(dev):
            x = x.to(torch.get_autocast_dtype(dev))
        return (x,) + self._mx_sr()


def _save_train_ctx(ctx, fmts, sr, wgrad_split_k, x: torch.Tensor, bias):
    """the autograd functions' fields (`wgrad_split_k` None where the entry has no such option).  `step` of `sr` is advanced in place
    by the backward: an attribute, not a saved tensor"""
    ctx.fmts, ctx.sr, ctx.wgrad_split_k = fmts, sr, wgrad_split_k
    ctx.x_dtype = x.dtype
    ctx.bias_dtype = None if bias is None else bias.dtype


def _quantize_grad(ctx, quantize):
    """the two forms of dy, which alone take `grad_rounding`, from `quantize(rounding, seed, step)`: row form (dx) on stream 0, column
    form (dW) on stream 1.  After a stochastic one the counter moves on, on the stream: the next backward or replay draws new words"""
    rounding, seed, step = ctx.sr
    forms = quantize(rounding, seed, step)
    if rounding == "stochastic" and step is not None:
        step.add_(1)
    return forms
