"""``mx_flash_decode`` without a GPU: the CPU path is ``_decode_def``, its identity with the streamed call at one split, the refusals, the
split heuristic, and its error against float64 attention next to the streamed route's."""
import pytest
import torch

import test_mx_flash as TF
from qsparse_amd import mx_flash_decode, quantize_with_mx
from qsparse_amd.mx_flash import _decode_def, _decode_splits
from qsparse_amd.quantize import mx_dequantize

E4, F62, FP4 = "mxfp8_e4m3", "mxfp6_e2m3", "mxfp4_e2m1"


def operands(seed, B, Hkv, r, T, S, d, dv, qk_fmt=E4, v_fmt=E4, device="cpu"):
    """(q_codes, q_scales, k_codes, k_scales, vt_codes, vt_scales) of random q [B, r Hkv, T, d], k [B, Hkv, S, d], v^T [B, Hkv, dv, S]"""
    g = torch.Generator().manual_seed(seed)
    out = ()
    for shape, fmt in (((B, r * Hkv, T, d), qk_fmt), ((B, Hkv, S, d), qk_fmt), ((B, Hkv, dv, S), v_fmt)):
        out += quantize_with_mx(torch.randn(shape, generator=g).to(device), fmt, -1, return_codes=True)[1:]
    return out


def decode(ops, qk_fmt, v_fmt, kv_len=None, **kw):
    return mx_flash_decode(*ops[:2], qk_fmt, *ops[2:], v_fmt, kv_len, **kw)


def repeated(ops, r):
    """the cache as the streamed call needs it: every kv head r times"""
    return ops[:2] + tuple(t.repeat_interleave(r, 1) for t in ops[2:])


def rms_ratio(ops, r, fmt, splits, scale=0.125):
    """rms error of the decode call over that of the streamed call on the repeated cache, both against float64 attention on the
    de-quantized operands"""
    rep = repeated(ops, r)
    q, k, vt = (mx_dequantize(rep[i], rep[i + 1], fmt, -1, torch.float64) for i in (0, 2, 4))
    ref = torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ vt.transpose(-1, -2)
    rms = lambda y: (y.double() - ref).pow(2).mean().sqrt().item()
    dec = rms(decode(ops, fmt, fmt, scale=scale, p_fmt=fmt, kv_splits=splits))
    streamed = rms(TF.flash(rep, fmt, fmt, scale=scale, p_fmt=fmt, rows="streamed"))
    print(f"{fmt} splits={splits}: decode rms {dec:.4e}, streamed rms {streamed:.4e}, ratio {dec / streamed:.3f}")
    return dec / streamed


@pytest.mark.parametrize("kw", ({}, {"is_causal": True}, {"p_fmt": FP4, "out_dtype": torch.bfloat16, "kv_splits": 3}))
def test_cpu_path_is_the_definition(kw):
    ops = operands(1, 2, 2, 3, 2, 300, 40, 24, FP4, E4)
    kv_len = torch.tensor([300, 131], dtype=torch.int32)
    got = decode(ops, FP4, E4, kv_len, scale=0.3, **kw)
    want = _decode_def(*ops[:2], FP4, *ops[2:], E4, kv_len, 0.3, kw.get("is_causal", False), kw.get("p_fmt", E4),
                       kw.get("out_dtype", torch.float32), kw.get("kv_splits", _decode_splits(4, 3)))
    assert got.shape == (2, 6, 2, 24) and got.dtype == want.dtype and torch.equal(got, want) and bool(got.float().isfinite().all())


@pytest.mark.parametrize("fmt,out_dtype", ((E4, torch.float32), (FP4, torch.float16)))
def test_one_split_is_the_streamed_call_on_the_repeated_cache(fmt, out_dtype):
    ops = operands(2, 2, 2, 4, 3, 300, 48, 40, fmt, fmt)
    kw = dict(scale=0.3, p_fmt=fmt, out_dtype=out_dtype)
    assert torch.equal(decode(ops, fmt, fmt, kv_splits=1, **kw), TF.flash(repeated(ops, 4), fmt, fmt, rows="streamed", **kw))
    sq = operands(3, 1, 2, 1, 40, 40, 32, 16)                    # T == S == L: bottom-right causal is the top-left triangle
    assert torch.equal(decode(sq, E4, E4, scale=0.3, is_causal=True, kv_splits=1),
                       TF.flash(sq, E4, E4, scale=0.3, is_causal=True, rows="streamed"))


def test_auto_splits():
    assert _decode_splits(8, 1) == 1 and _decode_splits(8, 5) == 5 and _decode_splits(8, 256) == 128
    assert _decode_splits(4096, 256) == 1 and _decode_splits(1, 10 ** 6) == 1024


def test_refusals():
    ok = operands(4, 2, 2, 2, 1, 40, 32, 16)
    call = lambda ops, kv_len=None, **kw: decode(ops, E4, E4, kv_len, scale=1.0, **kw)
    with pytest.raises(ValueError, match='<= 64.*rows="streamed"'):
        call(operands(4, 1, 1, 13, 5, 8, 32, 16))                # R = 65
    with pytest.raises(ValueError, match="multiple of Hkv"):
        call(ok[:2] + operands(4, 2, 3, 1, 1, 40, 32, 16)[2:])
    with pytest.raises(ValueError, match="exactly 4 dimensions"):
        call(tuple(t[0] for t in ok))
    for bad in (torch.tensor([40, 40]), torch.tensor([40], dtype=torch.int32), torch.tensor([40, 40], dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="kv_len"):
            call(ok, bad)
    with pytest.raises(ValueError, match="kv_splits"):
        call(ok, kv_splits=0)
    with pytest.raises(ValueError, match="d <= 128"):
        call(operands(4, 1, 1, 1, 1, 8, 129, 16))


@pytest.mark.parametrize("splits", (1, 5))
@pytest.mark.parametrize("fmt", (E4, F62))
def test_error_at_640_keys_stays_within_a_tenth_of_the_streamed_routes(fmt, splits):
    """splitting adds one float32 rounding per split to a result whose error is the rounding of each weight to p_fmt.  Measured on the CPU
    through the definition: E4M3 1.000 at one split (the same bytes) and 0.890 at five, E2M3 1.000 and 1.033"""
    assert rms_ratio(operands(5, 2, 2, 4, 1, 640, 64, 64, fmt, fmt), 4, fmt, splits) <= 1.10
