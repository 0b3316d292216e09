"""``mx_flash_attention(rows="streamed")`` without a GPU: the CPU path is ``_streamed_def``, its error against float64 attention next to
the composition's, and the keywords ``rows`` / ``impl="flash_streamed"``."""
import pytest
import torch

import test_mx_flash as TF
from qsparse_amd import mx_attention
from qsparse_amd.mx_flash import _streamed_def
from qsparse_amd.quantize import mx_dequantize

E4, F62, FP4 = "mxfp8_e4m3", "mxfp6_e2m3", "mxfp4_e2m1"


def rms_ratio(ops, fmt, causal, scale=0.125):
    """rms error of the streamed call over that of the composition, both against float64 attention on the de-quantized operands"""
    q, k, vt = (mx_dequantize(ops[i], ops[i + 1], fmt, -1, torch.float64) for i in (0, 2, 4))
    s = q @ k.transpose(-1, -2) * scale
    if causal:
        s = s.masked_fill(~torch.ones(s.shape[-2:], dtype=torch.bool, device=s.device).tril(), float("-inf"))
    ref = torch.softmax(s, -1) @ vt.transpose(-1, -2)
    kw = dict(scale=scale, is_causal=causal, p_fmt=fmt)
    rms = lambda y: (y.double() - ref).pow(2).mean().sqrt().item()
    streamed, composed = rms(TF.flash(ops, fmt, fmt, rows="streamed", **kw)), rms(TF.composition(ops, fmt, fmt, **kw))
    print(f"{fmt} causal={causal}: streamed rms {streamed:.4e}, composition rms {composed:.4e}, ratio {streamed / composed:.3f}")
    return streamed / composed


@pytest.mark.parametrize("kw", ({}, {"is_causal": True}, {"p_fmt": FP4, "out_dtype": torch.bfloat16}, {"mask": True}))
def test_cpu_path_is_the_definition(kw):
    ops = TF.operands(1, (2, 3), 17, 150, 40, 24, FP4, E4)
    mask = None
    if kw.pop("mask", False):
        mask = torch.rand(3, 17, 150, generator=torch.Generator().manual_seed(2)) > 0.3
        mask[..., :128] &= torch.arange(17)[:, None] % 3 != 0              # some rows admit nothing in chunk 0
    got = TF.flash(ops, FP4, E4, mask, scale=0.3, rows="streamed", **kw)
    flat = tuple(t.reshape((6,) + t.shape[2:]) for t in ops)
    fmask = None if mask is None else torch.zeros(3, 17, 150).masked_fill(~mask, float("-inf")).repeat(2, 1, 1)
    want = _streamed_def(*flat[:2], FP4, *flat[2:], E4, fmask, 0.3, kw.get("is_causal", False), kw.get("p_fmt", E4),
                         kw.get("out_dtype", torch.float32))
    assert got.shape == (2, 3, 17, 24) and got.dtype == want.dtype and torch.equal(got.reshape(6, 17, 24), want)
    assert bool(got.float().isfinite().all())


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("fmt", (E4, F62))
def test_error_at_640_keys_stays_within_a_tenth_of_the_compositions(fmt, causal):
    assert rms_ratio(TF.operands(3, (3,), 40, 640, 64, 64, fmt, fmt), fmt, causal) <= 1.10


def test_rows_keyword():
    ops = TF.operands(4, (1,), 2, 513, 32, 16)
    with pytest.raises(ValueError, match="S <= 512"):
        TF.flash(ops, E4, E4, scale=1.0, rows="resident")
    assert TF.flash(ops, E4, E4, scale=1.0, rows="streamed").shape == (1, 2, 16)
    with pytest.raises(ValueError, match="rows"):
        TF.flash(ops, E4, E4, scale=1.0, rows="online")
    with pytest.raises(ValueError, match="d <= 128"):
        TF.flash(TF.operands(4, (1,), 2, 16, 129, 16), E4, E4, scale=1.0, rows="streamed")


def test_impl_flash_streamed():
    g = torch.Generator().manual_seed(5)
    q, k, v = torch.randn(2, 5, 16, generator=g), torch.randn(2, 150, 16, generator=g), torch.randn(2, 150, 8, generator=g)
    got = mx_attention(q, k, v, softmax="fused", impl="flash_streamed")
    assert got.shape == (2, 5, 8) and bool(got.isfinite().all())
    assert torch.allclose(got, mx_attention(q, k, v, softmax="fused"), atol=0.05)
    with pytest.raises(ValueError, match="fused"):
        mx_attention(q, k, v, impl="flash_streamed")
    with pytest.raises(ValueError, match="impl"):
        mx_attention(q, k, v, softmax="fused", impl="streamed")
