"""The MX rotary embedding on the CPU: ``mx_rope_table``, ``mx_rope``, ``mx_rope_quantize`` and the ``rope=`` keyword of
``mx_attention`` / ``mx_attention_train``.  The definition (include/qsparse_hip.h, "MX rotary embedding") is a fixed sequence of float32
operations, so everything here is an identity: against tests/mx_rope_ref.py (a numpy loop over the pairs), against the compositions the
docstrings write down, and against autograd through the torch expression.  The one tolerance -- the distance from the float64 rotation
-- is derived where it is used."""
import math

import pytest
import torch

import mx_rope_ref as RR
from qsparse_amd import (MXMultiheadAttention, MXTrainMultiheadAttention, mx_attention, mx_attention_train, mx_bmm, mx_bmm_train,
                         mx_quantize_2way_batched, mx_rope, mx_rope_quantize, mx_rope_table, mx_softmax_backward_quantize,
                         mx_softmax_quantize, quantize_with_mx)
from qsparse_amd.mx_rope import _rope_def

DS = (2, 6, 32, 64, 96, 128)
TS = (1, 33)
QK, PF, VF, GF = "mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2"


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("dtype", RR.DTS, ids=str)
def test_definition_matches_the_numpy_loop(dtype, interleaved):
    for d in DS:
        for T in TS:
            x = RR.inputs(d * 100 + T, (2, 3, T, d), dtype)
            cos, sin = RR.tables(T, d, d + T)
            for inverse in (False, True):
                ref = RR.rope_ref(x, cos, sin, interleaved, inverse)
                y32 = mx_rope(x, cos, sin, interleaved=interleaved, inverse=inverse, out_dtype=torch.float32)
                assert y32.dtype == torch.float32 and y32.shape == x.shape
                assert RR.same_bits(y32, ref), (d, T, inverse)
                y = mx_rope(x, cos, sin, interleaved=interleaved, inverse=inverse)           # one rounding to x's dtype
                assert y.dtype == dtype and RR.same_bits(y, ref.to(dtype)), (d, T, inverse)
                assert RR.same_bits(mx_rope(x, cos, sin, interleaved=interleaved, inverse=inverse, out_dtype=torch.float16),
                                    ref.to(torch.float16))


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
def test_inverse_is_the_call_on_minus_sin_and_undoes_the_rotation(interleaved):
    for dtype in RR.DTS:
        x = RR.inputs(5, (3, 33, 64), dtype)
        cos, sin = RR.tables(33, 64, 2)
        a = mx_rope(x, cos, sin, interleaved=interleaved, inverse=True, out_dtype=torch.float32)
        b = mx_rope(x, cos, sin.neg(), interleaved=interleaved, out_dtype=torch.float32)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # and with a true table (c^2 + s^2 = 1 up to rounding) it is the inverse rotation, up to a few float32 roundings
    x = RR.inputs(6, (2, 33, 64), torch.float32)
    cos, sin = mx_rope_table(33, 64)
    back = mx_rope(mx_rope(x, cos, sin, interleaved=interleaved), cos, sin, interleaved=interleaved, inverse=True)
    assert (back - x).abs().max() <= 1e-5 * x.abs().max()


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
def test_within_three_roundings_of_the_float64_rotation(interleaved):
    """y_a = fl(fl(a c) - fl(b s)).  With u = 2^-24: fl(a c) = a c (1 + e1), fl(b s) = b s (1 + e2), the difference another (1 + e3),
    |e| <= u, so |y_a - (a c - b s)| <= (|a c| + |b s|) (2 u + u^2) <= (|a| + |b|) (2 u + u^2), because |c|, |s| <= 1 (a float32
    cosine never rounds above 1).  y_b likewise.  A subnormal product or sum adds at most 2^-150 per operation."""
    T, d = 33, 96
    x = RR.inputs(7, (4, T, d), torch.float32)
    cos, sin = RR.tables(T, d, 3)
    y = mx_rope(x, cos, sin, interleaved=interleaved).double()
    xd, c, s = x.double(), cos.double(), sin.double()
    a, b = (xd[..., 0::2], xd[..., 1::2]) if interleaved else (xd[..., :d // 2], xd[..., d // 2:])
    ya, yb = (y[..., 0::2], y[..., 1::2]) if interleaved else (y[..., :d // 2], y[..., d // 2:])
    u = 2.0 ** -24
    bound = (a.abs() + b.abs()) * (2 * u + u * u) + 3 * 2.0 ** -150
    assert ((ya - (a * c - b * s)).abs() <= bound).all()
    assert ((yb - (b * c + a * s)).abs() <= bound).all()


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("dtype", RR.DTS, ids=str)
def test_rope_quantize_is_the_two_way_quantizer_on_the_float32_rotation(dtype, interleaved):
    for T, d in ((1, 2), (33, 6), (33, 32), (33, 96), (1, 128)):
        x = RR.inputs(T + d, (2, 2, T, d), dtype)
        cos, sin = RR.tables(T, d, 4)
        for inverse in (False, True):
            y32 = RR.rope_ref(x, cos, sin, interleaved, inverse)
            for rf, cf in (("mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp4_e2m1", None), (None, "mxfp6_e2m3")):
                got = mx_rope_quantize(x, cos, sin, row_fmt=rf, col_fmt=cf, interleaved=interleaved, inverse=inverse)
                ref = mx_quantize_2way_batched(y32, rf, cf)
                assert len(got) == 4
                for g, r in zip(got, ref):
                    assert (g is None) == (r is None)
                    if g is not None:
                        assert g.dtype == torch.uint8 and g.is_contiguous() and torch.equal(g, r), (T, d, rf, cf)


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("inverse", (False, True), ids=("forward", "inverse"))
def test_backward_is_autograd_through_the_torch_expression(interleaved, inverse):
    T, d = 33, 32
    cos, sin = RR.tables(T, d, 5)
    x = RR.inputs(8, (2, 3, T, d), torch.float32)
    dy = RR.inputs(9, (2, 3, T, d), torch.float32)
    x1 = x.clone().requires_grad_(True)
    y1 = mx_rope(x1, cos, sin, interleaved=interleaved, inverse=inverse)
    assert y1.requires_grad
    y1.backward(dy)
    x2 = x.clone().requires_grad_(True)
    y2 = _rope_def(x2, cos, sin, interleaved, inverse)
    y2.backward(dy)
    assert torch.equal(y1.detach().view(torch.int32), y2.detach().view(torch.int32))
    assert torch.equal(x1.grad.view(torch.int32), x2.grad.view(torch.int32))
    # the backward is the inverse call, in the input's dtype whatever the output's
    xb = x.bfloat16().requires_grad_(True)
    mx_rope(xb, cos, sin, interleaved=interleaved, inverse=inverse, out_dtype=torch.float32).backward(dy)
    assert xb.grad.dtype == torch.bfloat16
    assert torch.equal(xb.grad, mx_rope(dy, cos, sin, interleaved=interleaved, inverse=not inverse, out_dtype=torch.bfloat16))
    assert not mx_rope(x, cos, sin).requires_grad
    with torch.no_grad():
        assert not mx_rope(x1, cos, sin).requires_grad


def test_table_is_the_float64_cosine_rounded_once():
    T, d, base = 37, 64, 10000.0
    cos, sin = mx_rope_table(T, d)
    assert cos.dtype == sin.dtype == torch.float32 and cos.shape == sin.shape == (T, d // 2) and cos.is_contiguous()
    for t in (0, 1, 17, 36):
        for j in (0, 1, 13, 31):
            ang = t * base ** (-2.0 * j / d)
            # the angle itself is formed in float64 by torch (pow, one product): allow its last-place differences to reach the result
            assert abs(float(cos[t, j]) - math.cos(ang)) <= 2.0 ** -24 + 1e-12 * max(1.0, ang)
            assert abs(float(sin[t, j]) - math.sin(ang)) <= 2.0 ** -24 + 1e-12 * max(1.0, ang)
    assert torch.equal(cos[0], torch.ones(d // 2)) and torch.equal(sin[0], torch.zeros(d // 2))
    pos = torch.tensor([5, 0, 36, 7])
    c2, s2 = mx_rope_table(4, d, positions=pos)
    assert torch.equal(c2, cos[pos]) and torch.equal(s2, sin[pos])
    c3, _ = mx_rope_table(T, d, base=500000.0)
    assert not torch.equal(c3, cos)
    ang = torch.arange(T, dtype=torch.float64)[:, None] * (torch.tensor(base, dtype=torch.float64) **
                                                           (torch.arange(d // 2, dtype=torch.float64) * (-2.0 / d)))[None]
    assert torch.equal(cos, ang.cos().float()) and torch.equal(sin, ang.sin().float())
    for bad in (dict(T=4, d=3), dict(T=4, d=0), dict(T=-1, d=4), dict(T=4, d=4, base=0.0), dict(T=4, d=4, positions=torch.arange(5))):
        with pytest.raises(ValueError):
            mx_rope_table(**bad)


def test_refusals():
    x = RR.inputs(1, (2, 5, 8), torch.float32)
    cos, sin = RR.tables(5, 8)
    for fn in (lambda *a, **k: mx_rope(*a, **k), lambda *a, **k: mx_rope_quantize(*a, row_fmt=QK, **k)):
        with pytest.raises(ValueError, match="even d"):
            fn(x[..., :7], cos, sin)
        with pytest.raises(ValueError, match="expected"):
            fn(x, cos[:4], sin)
        with pytest.raises(ValueError, match="expected"):
            fn(x, cos, sin[:, :3])
        with pytest.raises(TypeError, match="float32"):
            fn(x, cos.double(), sin)
        with pytest.raises(ValueError, match="contiguous"):
            fn(x, cos, sin.t().contiguous().t())
        with pytest.raises(ValueError, match="is on"):
            fn(x, cos.to("meta"), sin)
        with pytest.raises(RuntimeError, match="requires grad"):
            fn(x, cos.clone().requires_grad_(True), sin)
        with pytest.raises(TypeError):
            fn(x.long(), cos, sin)
        with pytest.raises(TypeError):
            fn(x, None, sin)
    with pytest.raises(ValueError, match="row_fmt, col_fmt or both"):
        mx_rope_quantize(x, cos, sin)
    with pytest.raises(ValueError, match="leading dimension"):
        mx_rope_quantize(x[0], cos, sin, row_fmt=QK)
    with pytest.raises(ValueError):
        mx_rope_quantize(x, cos, sin, row_fmt="mxfp9")
    with pytest.raises(TypeError):
        mx_rope(x, cos, sin, out_dtype=torch.float64)
    assert mx_rope(x[0], cos, sin).shape == (5, 8)            # the dense call takes a single slice
    # the attention keyword
    q, k, v = (RR.inputs(i, (2, 5, 8), torch.float32) for i in (2, 3, 4))
    k7, v7 = RR.inputs(5, (2, 7, 8), torch.float32), RR.inputs(6, (2, 7, 8), torch.float32)
    c7, s7 = RR.tables(7, 8, 1)
    for att in (mx_attention, mx_attention_train):
        for sm in ("torch", "fused"):
            with pytest.raises(ValueError, match="T == S"):
                att(q, k7, v7, rope=(cos, sin), softmax=sm)
            with pytest.raises(TypeError, match="2-tuple"):
                att(q, k, v, rope=(cos, sin, cos), softmax=sm)
            with pytest.raises(ValueError, match="expected"):
                att(q, k7, v7, rope=(cos, sin, cos, sin), softmax=sm)
            with pytest.raises(RuntimeError, match="requires grad"):
                att(q, k, v, rope=(cos, sin.clone().requires_grad_(True)), softmax=sm)
            with pytest.raises(ValueError, match="even d"):
                att(q[..., :7], k[..., :7], v, rope=(cos, sin), softmax=sm)
            att(q, k7, v7, rope=(cos, sin, c7, s7), softmax=sm)


# ---- attention: the written compositions ------------------------------------------------------------------------------------------

SHAPE = (2, 2, 33, 32)


def attention_operands(dtype, device="cpu", S=None):
    B, H, T, d = SHAPE
    q = RR.inputs(11, SHAPE, dtype).to(device)
    k = RR.inputs(12, (B, H, S or T, d), dtype).to(device)
    v = RR.inputs(13, (B, H, S or T, d), dtype).to(device)
    do = RR.inputs(14, SHAPE, dtype).to(device)
    cq, sq = (t.to(device) for t in mx_rope_table(T, d))
    ck, sk = (t.to(device) for t in mx_rope_table(S or T, d, positions=torch.arange(S or T) + 3))
    return q, k, v, do, (cq, sq, ck, sk)


def fused_composition(q, k, v, do, rope, interleaved, causal=True):
    """`mx_attention_train(softmax="fused", rope=)` as its docstring writes it: (o, dq, dk, dv)"""
    cq, sq, ck, sk = rope
    scale = q.shape[-1] ** -0.5
    q_row, q_rs, q_col, q_cs = mx_rope_quantize(q, cq, sq, row_fmt=QK, col_fmt=QK, interleaved=interleaved)
    k_row, k_rs, k_col, k_cs = mx_rope_quantize(k, ck, sk, row_fmt=QK, col_fmt=QK, interleaved=interleaved)
    s = mx_bmm(q_row, q_rs, QK, k_row, k_rs, QK)
    p_row, p_rs, p_col, p_cs, m, Z = mx_softmax_quantize(s, None, scale=scale, is_causal=causal, fmt=PF, col_fmt=PF, return_stats=True)
    v_n, v_ns, v_k, v_ks = mx_quantize_2way_batched(v, VF, VF)
    o = mx_bmm(p_row, p_rs, PF, v_k, v_ks, VF, None, q.dtype)
    g_row, g_rs, g_col, g_cs = mx_quantize_2way_batched(do, GF, GF)
    dv = mx_bmm(p_col, p_cs, PF, g_col, g_cs, GF, None, v.dtype)
    dp = mx_bmm(g_row, g_rs, GF, v_n, v_ns, VF)
    ds_row, ds_rs, ds_col, ds_cs = mx_softmax_backward_quantize(dp, s, m, Z, None, scale=scale, is_causal=causal, row_fmt=GF, col_fmt=GF)
    dq_rot = mx_bmm(ds_row, ds_rs, GF, k_col, k_cs, QK)
    dk_rot = mx_bmm(ds_col, ds_cs, GF, q_col, q_cs, QK)
    assert dq_rot.dtype == torch.float32
    dq = mx_rope(dq_rot, cq, sq, interleaved=interleaved, inverse=True, out_dtype=q.dtype)
    dk = mx_rope(dk_rot, ck, sk, interleaved=interleaved, inverse=True, out_dtype=k.dtype)
    return o, dq, dk, dv


def train_call(q, k, v, do, rope, interleaved, softmax, causal=True):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = mx_attention_train(q, k, v, is_causal=causal, softmax=softmax, rope=rope, rope_interleaved=interleaved,
                           qk_fmt=QK, p_fmt=PF, v_fmt=VF, grad_fmt=GF)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("softmax", ("torch", "fused"))
def test_attention_is_its_composition(softmax, interleaved):
    q, k, v, _, rope = attention_operands(torch.bfloat16)
    cq, sq, ck, sk = rope
    d = q.shape[-1]
    got = mx_attention(q, k, v, is_causal=True, softmax=softmax, rope=(cq, sq, ck, sk), rope_interleaved=interleaved, out_dtype=torch.bfloat16)
    qc, qs = mx_rope_quantize(q, cq, sq, row_fmt=QK, interleaved=interleaved)[:2]
    kc, ks = mx_rope_quantize(k, ck, sk, row_fmt=QK, interleaved=interleaved)[:2]
    s = mx_bmm(qc, qs, QK, kc, ks, QK)
    if softmax == "fused":
        pc, ps = mx_softmax_quantize(s, None, scale=d ** -0.5, is_causal=True, fmt=PF)
    else:
        s = s * d ** -0.5 + torch.zeros(33, 33).masked_fill(~torch.ones(33, 33, dtype=torch.bool).tril(), float("-inf"))
        _, pc, ps = quantize_with_mx(torch.softmax(s, -1), PF, -1, return_codes=True)
    _, vc, vs = quantize_with_mx(v.transpose(-1, -2).contiguous(), VF, -1, return_codes=True)
    ref = mx_bmm(pc, ps, PF, vc, vs, VF, None, torch.bfloat16)
    assert got.dtype == torch.bfloat16 and torch.equal(got, ref)
    # which is the attention without the keyword on the float32 rotations
    q32 = mx_rope(q, cq, sq, interleaved=interleaved, out_dtype=torch.float32)
    k32 = mx_rope(k, ck, sk, interleaved=interleaved, out_dtype=torch.float32)
    assert torch.equal(got, mx_attention(q32, k32, v, is_causal=True, softmax=softmax, out_dtype=torch.bfloat16))
    # a 2-tuple is the 4-tuple with the same tables twice; no rope is what it always was
    assert torch.equal(mx_attention(q, k, v, softmax=softmax, rope=(cq, sq), rope_interleaved=interleaved),
                       mx_attention(q, k, v, softmax=softmax, rope=(cq, sq, cq, sq), rope_interleaved=interleaved))
    assert not torch.equal(mx_attention(q, k, v, softmax=softmax), mx_attention(q, k, v, softmax=softmax, rope=(cq, sq)))


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=str)
def test_attention_train_torch_is_its_composition(dtype, interleaved):
    q, k, v, do, rope = attention_operands(dtype)
    o, dq, dk, dv = train_call(q, k, v, do, rope, interleaved, "torch")
    q2, k2, v2 = (t.clone().requires_grad_(True) for t in (q, k, v))
    qr = mx_rope(q2, rope[0], rope[1], interleaved=interleaved, out_dtype=torch.float32)
    kr = mx_rope(k2, rope[2], rope[3], interleaved=interleaved, out_dtype=torch.float32)
    sr = dict(grad_fmt=GF, grad_rounding="nearest", step=None)
    s = mx_bmm_train(qr, kr, a_fmt=QK, b_fmt=QK, out_dtype=torch.float32, seed=1, **sr)
    s = s * q.shape[-1] ** -0.5 + torch.zeros(33, 33).masked_fill(~torch.ones(33, 33, dtype=torch.bool).tril(), float("-inf"))
    ref = mx_bmm_train(torch.softmax(s, -1), v2, b_layout="kn", a_fmt=PF, b_fmt=VF, out_dtype=dtype, seed=0, **sr)
    ref.backward(do)
    assert o.dtype == dtype and torch.equal(o, ref.detach())
    for got, want in ((dq, q2.grad), (dk, k2.grad), (dv, v2.grad)):
        assert got.dtype == dtype and torch.equal(got, want)
    # the forward value is mx_attention's
    assert torch.equal(o, mx_attention(q, k, v, is_causal=True, rope=rope, rope_interleaved=interleaved, out_dtype=dtype))


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=str)
def test_attention_train_fused_is_its_composition(dtype, interleaved):
    q, k, v, do, rope = attention_operands(dtype)
    got = train_call(q, k, v, do, rope, interleaved, "fused")
    ref = fused_composition(q, k, v, do, rope, interleaved)
    for name, g, r in zip(("o", "dq", "dk", "dv"), got, ref):
        assert g.dtype == dtype and torch.equal(g, r), name
    assert torch.equal(got[0], mx_attention(q, k, v, is_causal=True, softmax="fused", rope=rope, rope_interleaved=interleaved,
                                            out_dtype=dtype))
    # only some gradients asked for: the same bits for those
    q1 = q.clone().requires_grad_(True)
    mx_attention_train(q1, k, v, is_causal=True, softmax="fused", rope=rope, rope_interleaved=interleaved).backward(do)
    assert torch.equal(q1.grad, ref[1])


def test_layers_pass_the_keyword_on():
    import torch.nn as nn
    torch.manual_seed(0)
    E, H, T, B = 64, 2, 9, 2
    mha = nn.MultiheadAttention(E, H, batch_first=True)
    x = torch.randn(B, T, E)
    cos, sin = mx_rope_table(T, E // H)
    inf = MXMultiheadAttention.from_float(mha)
    with torch.no_grad():
        y0, y1 = inf(x)[0], inf(x, rope=(cos, sin), rope_interleaved=True)[0]
        q, k, v = (t.reshape(B, T, H, E // H).transpose(1, 2) for t in inf.in_proj(x).chunk(3, -1))
        o = mx_attention(q, k, v, rope=(cos, sin), rope_interleaved=True)
        assert torch.equal(y1, inf.out_proj(o.transpose(1, 2).reshape(B, T, E))) and not torch.equal(y0, y1)
    for sm in ("torch", "fused"):
        tr = MXTrainMultiheadAttention.from_float(mha, softmax=sm)
        xa = x.clone().requires_grad_(True)
        ya = tr(xa, rope=(cos, sin))[0]
        ya.sum().backward()
        assert xa.grad is not None and not torch.equal(ya.detach(), tr(x)[0].detach())
        with torch.no_grad():
            assert torch.equal(tr.to_inference()(x, rope=(cos, sin))[0], ya.detach())


def test_argument_checks_of_the_entry_points():
    """the C ABI's own checks, in qs_mx_quant2_batched_v's order: refused or routed before anything is enqueued, so pointers that are
    never dereferenced do on a host without a GPU"""
    import ctypes

    from qsparse_amd import _hip
    lib = _hip.load()
    X, TAB, OUT = 0x10000, 0x20000, 0x30000
    VEC, PLAIN, ARG, DTYPE, ALIGN = _hip.MX_ROPE_ROUTE_VEC, _hip.MX_ROPE_ROUTE_PLAIN, -2, -1, -3

    def route(**kw):
        a = _hip.MxRopeQuant2Args()
        a.struct_size = ctypes.sizeof(a)
        a.x, a.cos, a.sin, a.row_codes, a.row_scales = X, TAB, TAB, OUT, OUT + 128
        a.G0, a.G1, a.R, a.C, a.x_stride_r, a.x_stride_g1 = 1, 2, 2, 8, 8, 16
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.qs_mx_rope_quant2_route(ctypes.byref(a)), lib.qs_mx_rope_quant2_v(ctypes.byref(a))

    assert lib.qs_mx_rope_quant2_route(None) == ARG and lib.qs_mx_rope_route(None) == ARG
    for kw, status in ((dict(C=7, x_stride_r=7), ARG),                  # odd d
                       (dict(cos=None), ARG), (dict(sin=None), ARG), (dict(x=None), ARG),
                       (dict(row_scales=None), ARG),                    # half a pair
                       (dict(row_codes=None, row_scales=None), ARG),    # no pair at all
                       (dict(row_format=9), ARG), (dict(R=-1), ARG), (dict(G1=-1), ARG),
                       (dict(xdt=5), DTYPE),
                       (dict(x=X + 2), ALIGN), (dict(cos=TAB + 2), ALIGN), (dict(sin=TAB + 1), ALIGN),
                       (dict(x_stride_r=6), ARG),                       # rows would overlap
                       (dict(x_stride_g1=-16), ARG),
                       (dict(R=0), 0), (dict(G0=0), 0), (dict(C=0, x_stride_r=0), 0)):
        assert route(**kw) == (status, status), kw
    for kw, want in ((dict(), VEC), (dict(interleaved=1), VEC), (dict(inverse=1), VEC),
                     (dict(cos=TAB + 4), PLAIN), (dict(x=X + 4), PLAIN), (dict(x_stride_r=9), PLAIN),
                     (dict(C=4), PLAIN),                                # float32: h = 2 is off the vector of 4 ...
                     (dict(C=4, interleaved=1), VEC),                   # ... which the interleaved layout does not need
                     (dict(xdt=1), PLAIN), (dict(xdt=1, interleaved=1), VEC),     # bf16: h = 4 is off the vector of 8
                     (dict(col_codes=OUT + 256, col_scales=OUT + 512), PLAIN),    # R % 16 != 0
                     (dict(R=16, x_stride_g1=128, col_codes=OUT + 256, col_scales=OUT + 512), VEC),
                     (dict(R=16, x_stride_g1=128, col_codes=OUT + 257, col_scales=OUT + 512), PLAIN)):
        a = _hip.MxRopeQuant2Args()
        a.struct_size = ctypes.sizeof(a)
        a.x, a.cos, a.sin, a.row_codes, a.row_scales = X, TAB, TAB, OUT, OUT + 128
        a.G0, a.G1, a.R, a.C, a.x_stride_r, a.x_stride_g1 = 1, 2, 2, 8, 8, 16
        for k, v in kw.items():
            setattr(a, k, v)
        assert lib.qs_mx_rope_quant2_route(ctypes.byref(a)) == want, kw
    b = _hip.MxRopeArgs()
    b.struct_size = ctypes.sizeof(b)
    b.x, b.cos, b.sin = X, TAB, TAB
    b.G0, b.G1, b.R, b.C, b.x_stride_r, b.x_stride_g1 = 1, 2, 2, 8, 8, 16
    assert lib.qs_mx_rope_route(ctypes.byref(b)) == ARG and lib.qs_mx_rope_v(ctypes.byref(b)) == ARG      # no y
    b.y = OUT
    assert lib.qs_mx_rope_route(ctypes.byref(b)) == VEC
    b.y = OUT + 4
    assert lib.qs_mx_rope_route(ctypes.byref(b)) == PLAIN
    b.ydt = 7
    assert lib.qs_mx_rope_route(ctypes.byref(b)) == DTYPE
    b.ydt, b.y = 1, OUT + 1
    assert lib.qs_mx_rope_route(ctypes.byref(b)) == ALIGN
    b.y, b.C = OUT, 6
    assert lib.qs_mx_rope_route(ctypes.byref(b)) == PLAIN
    b.C = 5
    assert lib.qs_mx_rope_route(ctypes.byref(b)) == ARG and lib.qs_mx_rope_v(ctypes.byref(b)) == ARG
    b.C, b.R = 6, 0
    assert lib.qs_mx_rope_route(ctypes.byref(b)) == 0 and lib.qs_mx_rope_v(ctypes.byref(b)) == 0
