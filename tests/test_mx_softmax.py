"""``mx_softmax_quantize`` on the CPU: the torch expression of the definition against tests/mx_softmax_ref.py (numpy float32, written
independently), the written-out exponential against float64 ``exp``, the exceptional rows, the argument refusals, the distance to
``torch.softmax`` as a condition, and the ``softmax=`` keyword of ``mx_attention`` / ``MXMultiheadAttention``."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mx_softmax_ref as SR
from qsparse_amd import MXMultiheadAttention, mx_attention, mx_bmm, mx_softmax_quantize, quantize_with_mx
from qsparse_amd.mx_softmax import _exp_def, _mx_softmax_p

SCALE = 0.37
VARIANTS = ("none", "float", "bool_ts", "bool_gts", "bool_b1ts", "causal_lt", "causal_eq", "causal_gt")
_cases = {}


def case(dtype, S, variant):
    """(s [..., T, S], keyword arguments of the call, p_ref float32 numpy [G, T, S]) -- computed once and shared (the GPU tests take the
    same cases)"""
    key = (dtype, S, variant)
    if key not in _cases:
        T = {"causal_lt": max(1, min(3, S - 1)), "causal_eq": S, "causal_gt": S + 2}.get(variant, 3)      # (S = 1 has no T < S)
        lead = (2, 2) if variant == "bool_b1ts" else (1,) if T > 64 else (2,)
        seed = 100 * S + VARIANTS.index(variant)
        s = SR.scores(seed, lead + (T, S), dtype)
        kw, add = {}, None
        if variant == "float":
            kw["mask"] = add = SR.float_mask(seed + 1, (T, S))
        elif variant.startswith("bool"):
            shape = {"bool_ts": (T, S), "bool_gts": lead + (T, S), "bool_b1ts": (2, 1, T, S)}[variant]
            kw["mask"] = SR.bool_mask(seed + 1, shape)
            add = SR.additive(kw["mask"])
            if add.dim() > 2:
                add = add.expand(lead + (T, S)).reshape(-1, T, S)
        elif variant.startswith("causal"):
            kw["is_causal"] = True
        p = SR.ref_p(s.reshape(-1, T, S), SCALE, add, causal=variant.startswith("causal"))
        _cases[key] = (s, kw, p)
    return _cases[key]


def same_p(a, b):
    """bit for bit, a NaN equal to a NaN"""
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("S", SR.SIZES)
@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
def test_cpu_path_equals_the_reference(dtype, S):
    for variant in VARIANTS:
        s, kw, p = case(dtype, S, variant)
        T = s.shape[-2]
        if variant != "bool_b1ts":        # the float32 p itself, where the private function takes the call's mask as it is
            add = kw.get("mask")
            add = SR.additive(add) if add is not None and add.dtype == torch.bool else add
            got = _mx_softmax_p(s.reshape(-1, T, S), add, SCALE, variant.startswith("causal")).numpy()
            assert same_p(got, p), (variant, S, dtype)
        for fmt in SR.FMTS:
            codes, scales = mx_softmax_quantize(s, scale=SCALE, fmt=fmt, **kw)
            rc, rs = SR.ref_codes(p, fmt)
            assert codes.shape == s.shape and scales.shape == s.shape[:-1] + ((S + 31) // 32,)
            assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8
            assert torch.equal(codes.reshape(rc.shape), rc) and torch.equal(scales.reshape(rs.shape), rs), (variant, S, dtype, fmt)


def _grid():
    """[-87, 0] at 2^20 points and, around every breakpoint (n + 1/2) ln 2 of the reduction, the 257 nearest float32 values"""
    t = np.linspace(-87.0, 0.0, 2 ** 20).astype(np.float32)
    brk = ((np.arange(-126, 0) + 0.5) * np.log(2.0)).astype(np.float32)
    brk = brk[brk >= -87.0]
    near = (brk.view(np.int32)[:, None] + np.arange(-128, 129, dtype=np.int32)[None, :]).view(np.float32).reshape(-1)
    return np.concatenate([t, near[(near >= -87.0) & (near <= 0.0)]])


# measured on the grid above: the largest relative error of E against float64 exp is 1.002e-7 = 0.840 float32 ulp, at t = -81.44409
E_MEASURED = 1.002e-7


def test_exp_against_float64():
    t = _grid()
    e = _exp_def(torch.from_numpy(t)).numpy()
    assert e.dtype == np.float32 and same_p(e, SR.ref_exp(t))           # the two statements of E agree in every bit
    exact = np.exp(t.astype(np.float64))
    rel = np.abs(e.astype(np.float64) - exact) / exact
    worst = float(rel.max())
    print(f"E: largest relative error {worst:.4e} = {worst * 2 ** 23:.3f} ulp at t = {t[rel.argmax()]!r} over {t.size} points")
    assert 2 * E_MEASURED <= 2.0 ** -21
    assert worst <= 2 * E_MEASURED
    assert worst >= 0.5 * E_MEASURED          # the recorded figure is this grid's, not a stale one
    one, zero = _exp_def(torch.tensor([0.0, -0.0, float("-inf"), -87.5, -1e30])).numpy(), SR.ref_exp(np.float32([0, -np.inf]))
    assert one[0] == 1.0 and one[1] == 1.0 and list(one[2:].view(np.uint32)) == [0, 0, 0]
    assert zero[0] == 1.0 and zero.view(np.uint32)[1] == 0


def _special_rows(dtype):
    """s [1, 9, 40] with one exceptional row between plain ones, the float mask that fully masks row 5, what is expected of each row"""
    s = SR.scores(7, (1, 9, 40), dtype)
    inf = float("inf")
    s[0, 1, 3] = float("nan")
    s[0, 3, 17] = inf
    s[0, 7, :] = -inf
    s[0, 8, 5:30] = -inf
    mask = torch.zeros(9, 40)
    mask[5, :] = -inf
    if dtype == torch.float16:
        s[0, 2, 0], s[0, 2, 1] = 65504.0, -65504.0
    return s, mask, {1: "nan", 3: "nan", 5: "nan", 7: "nan", 8: "zeros"}


@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
@pytest.mark.parametrize("fmt", SR.FMTS)
def test_exceptional_rows(fmt, dtype):
    s, mask, expect = _special_rows(dtype)
    codes, scales = mx_softmax_quantize(s, mask, scale=SCALE, fmt=fmt)
    rc, rs = SR.ref_codes(SR.ref_p(s, SCALE, mask), fmt)
    assert torch.equal(codes, rc) and torch.equal(scales, rs)
    plain = SR.scores(7, (1, 9, 40), dtype)
    if dtype == torch.float16:
        plain[0, 2, 0], plain[0, 2, 1] = 65504.0, -65504.0
    pc, ps = mx_softmax_quantize(plain, scale=SCALE, fmt=fmt)
    for r in range(9):
        if expect.get(r) == "nan":        # NaN as a whole: 0xFF in each of its blocks, zero codes
            assert bool((scales[0, r] == 0xFF).all()) and not bool(codes[0, r].any()), r
        else:
            assert not bool((scales[0, r] == 0xFF).any()), r
            if r != 8:                    # a neighbour of an exceptional row is what it is alone
                assert torch.equal(codes[0, r], pc[0, r]) and torch.equal(scales[0, r], ps[0, r]), r
    assert not bool(codes[0, 8, 5:30].any()) and bool(codes[0, 8, :5].any())        # -inf beside finite values: plain zeros
    if dtype == torch.float16:            # +-65504 * 0.37 stays finite: the row is one-hot
        assert int(codes[0, 2].count_nonzero()) == 1 and int(codes[0, 2, 0]) != 0


@pytest.mark.parametrize("scale", (0.0, -0.37))
def test_zero_and_negative_scale(scale):
    s = SR.scores(11, (2, 3, 70), torch.float32)
    for fmt in ("mxfp8_e4m3", "mxfp4_e2m1"):
        codes, scales = mx_softmax_quantize(s, scale=scale, fmt=fmt)
        rc, rs = SR.ref_codes(SR.ref_p(s, scale), fmt)
        assert torch.equal(codes, rc) and torch.equal(scales, rs)
        if scale == 0.0:                  # the uniform row 1 / 70, the same code everywhere
            assert bool((codes == codes[0, 0, 0]).all()) and int(codes[0, 0, 0]) != 0
    s[1, 1, 4] = float("inf") if scale == 0.0 else float("-inf")             # inf * 0 is a NaN, -inf * -0.37 is +inf: that row alone
    codes, scales = mx_softmax_quantize(s, scale=scale)
    assert bool((scales[1, 1] == 0xFF).all()) and not bool((scales[1, 0] == 0xFF).any()) and not bool((scales[1, 2] == 0xFF).any())


def test_argument_refusals():
    s = SR.scores(3, (2, 4, 33), torch.float32)
    with pytest.raises(TypeError):
        mx_softmax_quantize(s.double())
    with pytest.raises(TypeError):
        mx_softmax_quantize(s.to(torch.int32))
    with pytest.raises(TypeError):
        mx_softmax_quantize(s.numpy())
    with pytest.raises(ValueError):
        mx_softmax_quantize(s[0, 0])                                         # one dimension
    for shape in ((4, 32), (33, 4), (3, 4, 33), (2, 2, 4, 33)):
        with pytest.raises(ValueError):
            mx_softmax_quantize(s, torch.zeros(shape))                       # wrong mask shape
    with pytest.raises(TypeError):
        mx_softmax_quantize(s, torch.zeros(4, 33, dtype=torch.int32))
    with pytest.raises(ValueError):
        mx_softmax_quantize(s, torch.zeros(4, 33, device="meta"))            # wrong mask device
    with pytest.raises(ValueError):
        mx_softmax_quantize(s, torch.zeros(4, 33), is_causal=True)           # both masks
    with pytest.raises(RuntimeError):
        mx_softmax_quantize(s.clone().requires_grad_(True))
    with pytest.raises(RuntimeError):
        mx_softmax_quantize(s, torch.zeros(4, 33, requires_grad=True))
    with torch.no_grad():                                                    # refused only where a gradient could be asked for
        assert not mx_softmax_quantize(s.clone().requires_grad_(True))[0].requires_grad
    with pytest.raises(ValueError):
        mx_softmax_quantize(s, fmt="mxfp7")
    with pytest.raises(TypeError):
        mx_softmax_quantize(s, scale="1")
    codes, scales = mx_softmax_quantize(torch.zeros(2, 0, 33))
    assert codes.shape == (2, 0, 33) and scales.shape == (2, 0, 2)


@pytest.mark.parametrize("fmt", SR.FMTS)
def test_distance_to_torch_softmax(fmt):
    """a condition, not an identity: the share of differing codes stays at or below 1e-3 and no scale byte differs by more than 1"""
    s = SR.scores(2024, (8, 33, 197), torch.float32)
    mask = SR.float_mask(2025, (33, 197))
    for kw, add in (({}, None), ({"mask": mask}, mask)):
        codes, scales = mx_softmax_quantize(s, scale=SCALE, fmt=fmt, **kw)
        u = s * SCALE if add is None else s * SCALE + add
        _, tc, ts = quantize_with_mx(torch.softmax(u, -1), fmt, -1, return_codes=True)
        share = float((codes != tc).float().mean())
        step = int((scales.int() - ts.int()).abs().max())
        print(f"{fmt} mask={add is not None}: share of differing codes {share:.3e}, largest scale-byte difference {step}")
        assert share <= 1e-3 and step <= 1


def _qkv(seed, shape_q, S, dv, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    lead, (T, d) = shape_q[:-2], shape_q[-2:]
    return (torch.randn(*lead, T, d, generator=g).to(dtype), torch.randn(*lead, S, d, generator=g).to(dtype),
            torch.randn(*lead, S, dv, generator=g).to(dtype))


def fused_composition(q, k, v, attn_mask=None, is_causal=False, scale=None, fmt="mxfp8_e4m3", out_dtype=torch.float32):
    """what ``mx_attention(softmax="fused")`` is defined as, from public calls"""
    _, qc, qs_ = quantize_with_mx(q, fmt, -1, return_codes=True)
    _, kc, ks = quantize_with_mx(k, fmt, -1, return_codes=True)
    s = mx_bmm(qc, qs_, fmt, kc, ks, fmt)
    pc, ps = mx_softmax_quantize(s, attn_mask, scale=q.shape[-1] ** -0.5 if scale is None else scale, is_causal=is_causal, fmt=fmt)
    _, vc, vs = quantize_with_mx(v.transpose(-1, -2).contiguous(), fmt, -1, return_codes=True)
    return mx_bmm(pc, ps, fmt, vc, vs, fmt, None, out_dtype)


def torch_composition(q, k, v, mask=None, scale=None, fmt="mxfp8_e4m3", out_dtype=torch.float32):
    """steps 1 - 8 of ``mx_attention``'s docstring, as they were before the keyword"""
    _, qc, qs_ = quantize_with_mx(q, fmt, -1, return_codes=True)
    _, kc, ks = quantize_with_mx(k, fmt, -1, return_codes=True)
    s = mx_bmm(qc, qs_, fmt, kc, ks, fmt) * (q.shape[-1] ** -0.5 if scale is None else scale)
    if mask is not None:
        s = s + mask
    _, pc, ps = quantize_with_mx(torch.softmax(s, -1), fmt, -1, return_codes=True)
    _, vc, vs = quantize_with_mx(v.transpose(-1, -2).contiguous(), fmt, -1, return_codes=True)
    return mx_bmm(pc, ps, fmt, vc, vs, fmt, None, out_dtype)


def test_attention_softmax_keyword():
    q, k, v = _qkv(5, (2, 3, 37, 16), 37, 16)
    causal = torch.zeros(37, 37).masked_fill(~torch.ones(37, 37, dtype=torch.bool).tril(), float("-inf"))
    assert torch.equal(mx_attention(q, k, v, is_causal=True, softmax="fused"), fused_composition(q, k, v, is_causal=True))
    assert torch.equal(mx_attention(q, k, v, is_causal=True, softmax="torch"), torch_composition(q, k, v, causal))
    assert torch.equal(mx_attention(q, k, v, is_causal=True), torch_composition(q, k, v, causal))           # the default is "torch"
    q, k, v = _qkv(6, (2, 2, 33, 40), 45, 24, torch.bfloat16)
    mask = SR.float_mask(9, (33, 45))
    got = mx_attention(q, k, v, mask, scale=0.2, p_fmt="mxfp4_e2m1", softmax="fused", out_dtype=torch.bfloat16)
    _, qc, qs_ = quantize_with_mx(q, "mxfp8_e4m3", -1, return_codes=True)
    _, kc, ks = quantize_with_mx(k, "mxfp8_e4m3", -1, return_codes=True)
    pc, ps = mx_softmax_quantize(mx_bmm(qc, qs_, "mxfp8_e4m3", kc, ks, "mxfp8_e4m3"), mask, scale=0.2, fmt="mxfp4_e2m1")
    _, vc, vs = quantize_with_mx(v.transpose(-1, -2).contiguous(), "mxfp8_e4m3", -1, return_codes=True)
    assert torch.equal(got, mx_bmm(pc, ps, "mxfp4_e2m1", vc, vs, "mxfp8_e4m3", None, torch.bfloat16))
    assert torch.equal(mx_attention(q, k, v, mask, scale=0.2, softmax="torch"), torch_composition(q, k, v, mask, 0.2))
    for bad in ("flash", None, "Fused"):
        with pytest.raises(ValueError):
            mx_attention(q, k, v, softmax=bad)
    with pytest.raises(ValueError):
        mx_attention(q, k, v, mask, is_causal=True, softmax="fused")
    with pytest.raises(TypeError):
        mx_attention(q, k, v, None, False, None, "fused")                    # keyword-only, and last


def test_multihead_attention_forwards_the_keyword():
    torch.manual_seed(0)
    mha = nn.MultiheadAttention(32, 4, batch_first=True)
    x = torch.randn(2, 9, 32)
    layers = {sm: MXMultiheadAttention.from_float(mha, softmax=sm) for sm in ("torch", "fused")}
    assert MXMultiheadAttention.from_float(mha).softmax == "torch" and layers["fused"].softmax == "fused"
    for sm, layer in layers.items():
        h, E = 4, 32
        qkv = layer.in_proj(x)
        q, k, v = (t.reshape(2, 9, h, E // h).transpose(1, 2) for t in qkv.chunk(3, -1))
        o = mx_attention(q, k, v, is_causal=True, softmax=sm)
        want = layer.out_proj(o.transpose(1, 2).reshape(2, 9, E))
        assert torch.equal(layer(x, is_causal=True)[0], want), sm
    direct = MXMultiheadAttention(layers["torch"].in_proj, layers["torch"].out_proj, 4, True, softmax="fused")
    assert torch.equal(direct(x)[0], layers["fused"](x)[0])
    with pytest.raises(ValueError):
        MXMultiheadAttention.from_float(mha, softmax="flash")
