"""Batched matrix products on MX codes on the CPU: ``mx_bmm`` against the stacked per-slice ``mx_matmul`` (bit for bit, codes out
included), its argument errors and empty products; ``mx_attention`` and ``MXMultiheadAttention`` against their composition written
out with the public calls; the refusals."""
import math
import re

import pytest
import torch
import torch.nn as nn

import qsparse_amd as qs
from qsparse_amd import MXMultiheadAttention, mx_attention, mx_bmm, mx_matmul, quantize_with_mx
from qsparse_amd.mx_gemm import MXLinear

FMTS = ["mxfp8_e4m3", "mxfp8_e5m2", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp4_e2m1"]
E4, FP4 = "mxfp8_e4m3", "mxfp4_e2m1"


def codes_of(x, fmt):
    return tuple(quantize_with_mx(x, fmt, -1, return_codes=True)[1:])


def operands(g, lead, M, N, K, fa, fb):
    return (codes_of(torch.randn(*lead, M, K, generator=g) * 3, fa) + codes_of(torch.randn(*lead, N, K, generator=g), fb))


def stacked(ac, asc, fa, bc, bsc, fb, bias=None, dt=torch.float32, **kw):
    """mx_matmul slice by slice over the flattened leading dimensions; a tuple of stacks with out_fmt"""
    M, K, N = ac.shape[-2], ac.shape[-1], bc.shape[-2]
    lead = tuple(ac.shape[:-2])
    a3, s3, b3, t3 = (t.reshape((-1,) + tuple(t.shape[-2:])) for t in (ac, asc, bc, bsc))
    bias2 = None if bias is None else bias.reshape(-1, N)
    outs = []
    for i in range(a3.shape[0]):
        b = None if bias is None else (bias if bias.dim() == 1 else bias2[i])
        outs.append(mx_matmul(a3[i], s3[i], fa, b3[i], t3[i], fb, b, dt, **kw))
    if kw.get("out_fmt") is None:
        return torch.stack(outs).reshape(lead + (M, N))
    return tuple(torch.stack([o[j] for o in outs]).reshape(lead + tuple(outs[0][j].shape)) for j in range(2))


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("fa,fb", [(E4, E4), (FP4, "mxfp6_e2m3"), ("mxfp8_e5m2", FP4), ("mxfp6_e3m2", E4)])
def test_cpu_path_is_the_stacked_matmul(fa, fb):
    g = torch.Generator().manual_seed(FMTS.index(fa) * 5 + FMTS.index(fb))
    for lead, (M, N, K) in (((3,), (5, 7, 40)), ((2, 3), (4, 33, 64)), ((1,), (1, 1, 1))):
        ops = operands(g, lead, M, N, K, fa, fb)
        args = (*ops[:2], fa, *ops[2:], fb)
        for bias in (None, torch.randn(N, generator=g), torch.randn(*lead, N, generator=g)):
            for dt in (torch.float32, torch.bfloat16, torch.float16):
                y = mx_bmm(*args, bias, dt)
                assert y.shape == lead + (M, N) and bits(y, stacked(*args, bias, dt))
            for out_fmt in (E4, FP4):
                for act in (None, "relu"):
                    got, want = mx_bmm(*args, bias, out_fmt=out_fmt, act=act), stacked(*args, bias, out_fmt=out_fmt, act=act)
                    assert got[0].shape == lead + (M, N) and got[1].shape == lead + (M, -(-N // 32))
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_ff_scale_byte_stays_in_its_slice():
    g = torch.Generator().manual_seed(1)
    ac, asc, bc, bsc = operands(g, (3,), 4, 5, 64, E4, E4)
    asc[1, 2, 0] = 255
    y = mx_bmm(ac, asc, E4, bc, bsc, E4)
    nan = torch.zeros(3, 4, 5, dtype=torch.bool)
    nan[1, 2] = True
    assert torch.equal(y.isnan(), nan)


def test_empty_products():
    for lead, M, N in (((0,), 3, 4), ((2,), 0, 4), ((2,), 3, 0), ((2, 0), 3, 4)):
        ac, asc = torch.zeros(*lead, M, 40, dtype=torch.uint8), torch.full((*lead, M, 2), 127, dtype=torch.uint8)
        bc, bsc = torch.zeros(*lead, N, 40, dtype=torch.uint8), torch.full((*lead, N, 2), 127, dtype=torch.uint8)
        y = mx_bmm(ac, asc, E4, bc, bsc, FP4, None, torch.bfloat16)
        assert y.shape == lead + (M, N) and y.dtype == torch.bfloat16
        c, s = mx_bmm(ac, asc, E4, bc, bsc, FP4, out_fmt=E4)
        assert c.shape == lead + (M, N) and s.shape == lead + (M, -(-N // 32)) and c.dtype == s.dtype == torch.uint8


def test_argument_errors():
    g = torch.Generator().manual_seed(3)
    ac, asc, bc, bsc = operands(g, (2,), 3, 4, 40, E4, E4)
    ok = (ac, asc, E4, bc, bsc, E4)

    def raises(exc, msg, *a, **kw):
        with pytest.raises(exc, match=re.escape(msg)):
            mx_bmm(*a, **kw)

    raises(ValueError, "one weight [N, K] shared by every row of a is mx_matmul", ac, asc, E4, bc[0], bsc[0], E4)
    raises(ValueError, "a_codes needs at least 3 dimensions [..., M, K], got shape (3, 40)", ac[0], asc[0], E4, bc, bsc, E4)
    raises(ValueError, "b_codes needs at least 3 dimensions [..., N, K], got shape (40,)", ac, asc, E4, bc[0, 0], bsc[0, 0], E4)
    raises(ValueError, "disagree on their leading dimensions (nothing is broadcast)", ac, asc, E4, bc[:1], bsc[:1], E4)
    raises(ValueError, "disagree on their leading dimensions", ac, asc, E4, bc[None], bsc[None], E4)
    raises(ValueError, "disagree on K (their last dimensions)", ac, asc, E4, bc[..., :32], bsc[..., :1], E4)
    raises(ValueError, "a_scales has shape (2, 3, 1), expected (2, 3, 2)", ac, asc[..., :1], E4, bc, bsc, E4)
    raises(TypeError, "b_codes must be uint8", ac, asc, E4, bc.float(), bsc, E4)
    raises(TypeError, "a_codes must be a tensor, got NoneType", None, asc, E4, bc, bsc, E4)
    raises(ValueError, "mx_bmm needs K >= 1", ac[..., :0], asc[..., :0], E4, bc[..., :0], bsc[..., :0], E4)
    raises(TypeError, "out_dtype must be one of", *ok, None, torch.float64)
    raises(TypeError, "bias must be a float32 tensor", *ok, torch.zeros(4, dtype=torch.float64))
    raises(ValueError, "bias has shape (3,), expected (4,) or (2, 4)", *ok, torch.zeros(3))
    raises(ValueError, "bias has shape (1, 4), expected (4,) or (2, 4)", *ok, torch.zeros(1, 4))
    raises(ValueError, "act='relu' needs out_fmt", *ok, act="relu")
    raises(ValueError, "unknown act 'gelu'", *ok, out_fmt=E4, act="gelu")
    raises(ValueError, "cannot be combined with out_fmt", *ok, None, torch.bfloat16, out_fmt=E4)
    with pytest.raises(ValueError):
        mx_bmm(ac, asc, "mxfp9", bc, bsc, E4)
    with pytest.raises(ValueError):
        mx_bmm(*ok, out_fmt="mxfp9")
    with pytest.raises(TypeError):
        mx_bmm(*ok, split_k=2)          # there is no split-K form


# ---- attention -------------------------------------------------------------------------------------------------------------------
def attention_composition(q, k, v, mask=None, scale=None, qk=E4, pf=E4, vf=E4, dt=torch.float32, bmm=mx_bmm):
    """the definition of mx_attention, written out with the public calls (`bmm`: mx_bmm, or the stacked mx_matmul)"""
    qc, qs_ = codes_of(q, qk)
    kc, ks = codes_of(k, qk)
    s = bmm(qc, qs_, qk, kc, ks, qk) * (q.shape[-1] ** -0.5 if scale is None else scale)
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = torch.zeros(mask.shape, dtype=torch.float32, device=mask.device).masked_fill(~mask, float("-inf"))
        s = s + mask
    pc, ps = codes_of(torch.softmax(s, -1), pf)
    vc, vs = codes_of(v.transpose(-1, -2).contiguous(), vf)
    return bmm(pc, ps, pf, vc, vs, vf, None, dt)


def qkv(g, B, h, T, S, d, dv=None):
    return (torch.randn(B, h, T, d, generator=g), torch.randn(B, h, S, d, generator=g), torch.randn(B, h, S, dv or d, generator=g))


@pytest.mark.parametrize("d", [40, 64])
@pytest.mark.parametrize("S", [11, 16])
def test_attention_is_its_composition(d, S):
    g = torch.Generator().manual_seed(d + S)
    T = 11
    q, k, v = qkv(g, 2, 3, T, S, d, 24)
    add = torch.randn(T, S, generator=g)
    boolean = torch.rand(2, 1, T, S, generator=g) > 0.3
    boolean[..., 0] = True                                     # every row keeps a key
    causal = torch.ones(T, S, dtype=torch.bool).tril()
    for kw, mask in (({}, None), ({"attn_mask": add}, add), ({"attn_mask": boolean}, boolean), ({"is_causal": True}, causal)):
        y = mx_attention(q, k, v, **kw)
        assert y.shape == (2, 3, T, 24) and not y.isnan().any()
        assert bits(y, attention_composition(q, k, v, mask))
        assert bits(y, attention_composition(q, k, v, mask, bmm=stacked))
    y = mx_attention(q, k, v, scale=0.25, qk_fmt="mxfp6_e2m3", p_fmt=FP4, v_fmt="mxfp8_e5m2", out_dtype=torch.bfloat16)
    assert bits(y, attention_composition(q, k, v, None, 0.25, "mxfp6_e2m3", FP4, "mxfp8_e5m2", torch.bfloat16))
    # close to float attention: a sanity check of the composition itself, not a bound on the formats
    ref = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1) @ v
    assert (mx_attention(q, k, v) - ref).abs().max() < 0.25 * ref.abs().max()


def test_attention_refusals():
    g = torch.Generator().manual_seed(5)
    q, k, v = qkv(g, 1, 2, 5, 6, 32)
    with pytest.raises(ValueError, match="attn_mask or is_causal, not both"):
        mx_attention(q, k, v, torch.zeros(5, 6), True)
    with pytest.raises(RuntimeError, match="training side of attention on MX codes is not offered"):
        mx_attention(q, k.clone().requires_grad_(True), v)
    with torch.no_grad():
        assert mx_attention(q, k.clone().requires_grad_(True), v).shape == (1, 2, 5, 32)
    with pytest.raises(ValueError, match="q needs at least 3 dimensions"):
        mx_attention(q[0, 0], k[0, 0], v[0, 0])
    with pytest.raises(ValueError, match="disagree on their leading dimensions"):
        mx_attention(q, k[:, :1], v[:, :1])
    with pytest.raises(ValueError, match="disagree on d"):
        mx_attention(q, k[..., :16], v)
    with pytest.raises(ValueError, match="disagree on S"):
        mx_attention(q, k, v[..., :5, :])
    with pytest.raises(ValueError, match=re.escape("attn_mask has shape (6, 5), expected [..., 5, 6]")):
        mx_attention(q, k, v, torch.zeros(6, 5))
    with pytest.raises(TypeError, match="boolean or a floating-point"):
        mx_attention(q, k, v, torch.zeros(5, 6, dtype=torch.int64))
    with pytest.raises(TypeError, match="q must be one of"):
        mx_attention(q.double(), k, v)


# ---- the layer -------------------------------------------------------------------------------------------------------------------
def layer_composition(mha, x, mask=None, act_fmt=E4, w_fmt=E4, attention=attention_composition):
    E, h = mha.embed_dim, mha.num_heads
    lin = []
    for w, b in ((mha.in_proj_weight, mha.in_proj_bias), (mha.out_proj.weight, mha.out_proj.bias)):
        _, c, s = quantize_with_mx(w.detach(), w_fmt, 1, return_codes=True)
        lin.append(MXLinear(c, s, w_fmt, None if b is None else b.detach(), act_fmt).to(x.device))
    xb = x if mha.batch_first else x.transpose(0, 1)
    B, T = xb.shape[:2]
    q, k, v = (t.reshape(B, T, h, E // h).transpose(1, 2) for t in lin[0](xb).chunk(3, -1))
    y = lin[1](attention(q, k, v, mask).transpose(1, 2).reshape(B, T, E))
    return y if mha.batch_first else y.transpose(0, 1)


@pytest.mark.parametrize("batch_first,bias", [(True, True), (False, True), (True, False)])
def test_layer_is_its_composition(batch_first, bias):
    torch.manual_seed(7)
    mha = nn.MultiheadAttention(120, 3, bias=bias, batch_first=batch_first)          # d = 40
    layer = MXMultiheadAttention.from_float(mha)
    B, T = 2, 9
    x = torch.randn(B, T, 120) if batch_first else torch.randn(T, B, 120)
    y, w = layer(x)
    assert w is None and y.shape == x.shape and not y.requires_grad and bits(y, layer_composition(mha, x))
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    assert bits(layer(x, is_causal=True)[0], layer_composition(mha, x, causal))
    add = torch.randn(B, 3, T, T)
    assert bits(layer(x, attn_mask=add)[0], layer_composition(mha, x, add))
    ref = mha(x, x, x, need_weights=False)[0]
    assert (y - ref).abs().max() < 0.25 * ref.abs().max()
    assert "num_heads=3" in repr(layer)


def test_layer_state_dict_round_trip():
    torch.manual_seed(8)
    a, b = (MXMultiheadAttention.from_float(nn.MultiheadAttention(64, 1, batch_first=True), w_fmt=FP4) for _ in range(2))   # d = 64
    x = torch.randn(2, 5, 64)
    assert not torch.equal(a(x)[0], b(x)[0])
    sd = a.state_dict()
    assert sorted(sd) == ["in_proj.bias", "in_proj.weight_codes", "in_proj.weight_scales", "out_proj.bias", "out_proj.weight_codes",
                          "out_proj.weight_scales"]
    b.load_state_dict(sd)
    assert bits(a(x)[0], b(x)[0])


def test_layer_refusals():
    x = torch.randn(2, 5, 64)
    layer = MXMultiheadAttention.from_float(nn.MultiheadAttention(64, 2, batch_first=True))
    with pytest.raises(ValueError, match="need_weights=True is not offered"):
        layer(x, need_weights=True)
    with pytest.raises(ValueError, match="key_padding_mask is not offered"):
        layer(x, key_padding_mask=torch.zeros(2, 5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="requires grad"):
        layer(x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="x must be"):
        layer(x[0])
    with pytest.raises(ValueError, match="kdim / vdim"):
        MXMultiheadAttention.from_float(nn.MultiheadAttention(64, 2, kdim=32, vdim=32))
    with pytest.raises(ValueError, match="add_bias_kv=True is not supported"):
        MXMultiheadAttention.from_float(nn.MultiheadAttention(64, 2, add_bias_kv=True))
    with pytest.raises(ValueError, match="add_zero_attn=True is not supported"):
        MXMultiheadAttention.from_float(nn.MultiheadAttention(64, 2, add_zero_attn=True))
    with pytest.raises(TypeError, match="needs an nn.MultiheadAttention"):
        MXMultiheadAttention.from_float(nn.Linear(4, 4))
    with pytest.raises(ValueError, match="num_heads must be"):
        MXMultiheadAttention(layer.in_proj, layer.out_proj, 5)
    assert qs.MXMultiheadAttention is MXMultiheadAttention and qs.mx_bmm is mx_bmm and qs.mx_attention is mx_attention


# ---- the C ABI without a GPU: layout of the descriptors, and the checks that come before anything is enqueued --------------------
def test_descriptors_have_the_headers_layout(tmp_path):
    import ctypes
    import os
    import subprocess
    from qsparse_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = {"qs_mx_bmm_args": _hip.MxBmmArgs, "qs_mx_bmm_q_args": _hip.MxBmmQArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(root, "include", "qsparse_hip.h")}"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append(f'printf("{cname} %zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {fname}));' for fname, _ in ct._fields_]
        lines.append('printf("\\n");')
    (tmp_path / "layout.c").write_text("\n".join(lines + ['return 0; }']))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    for line, (cname, ct) in zip(out, pairs.items()):
        name, size, *offsets = line.split()
        assert name == cname and int(size) == ctypes.sizeof(ct)
        assert [int(o) for o in offsets] == [getattr(ct, f).offset for f, _ in ct._fields_], cname


def test_entry_points_validate_in_matmuls_order_without_a_gpu():
    import ctypes
    from qsparse_amd import _hip
    lib = _hip.load()
    ARG, DTYPE, ALIGN = -2, -1, -3
    for fn in (lib.qs_mx_bmm_v, lib.qs_mx_bmm_route, lib.qs_mx_bmm_q_v, lib.qs_mx_bmm_q_route):
        assert fn(None) == ARG

    def desc(cls, **kw):
        a = cls()
        a.struct_size = ctypes.sizeof(a)
        a.a_codes, a.a_scales, a.b_codes, a.b_scales = 1024, 2048, 4096, 8192
        a.G, a.M, a.N, a.K = 3, 5, 8, 64
        if cls is _hip.MxBmmArgs:
            a.y = 1 << 20
        else:
            a.out_codes, a.out_scales = 1 << 20, 1 << 21
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    for cls, route in ((_hip.MxBmmArgs, lib.qs_mx_bmm_route), (_hip.MxBmmQArgs, lib.qs_mx_bmm_q_route)):
        assert route(desc(cls)) == _hip.MX_GEMM_ROUTE_VEC
        assert route(desc(cls, K=40)) == _hip.MX_GEMM_ROUTE_PLAIN                       # K % 16 != 0
        assert route(desc(cls, b_codes=4097)) == _hip.MX_GEMM_ROUTE_PLAIN               # a base off the 16-byte grid
        assert route(desc(cls, bias=64, bias_batch_stride=8)) == _hip.MX_GEMM_ROUTE_VEC
        assert route(desc(cls, bias=64, bias_batch_stride=4)) == ARG                    # neither 0 nor N
        assert route(desc(cls, a_scales=None)) == ARG and route(desc(cls, b_format=5)) == ARG and route(desc(cls, G=-1)) == ARG
        assert route(desc(cls, bias=66)) == ALIGN
        for empty in ("G", "M", "N"):
            assert route(desc(cls, **{empty: 0})) == 0
        assert route(desc(cls, K=0)) == ARG and route(desc(cls, K=0, G=0)) == 0
        assert route(desc(cls, G=1 << 40, M=1 << 12, K=1 << 12)) == ARG                 # G M K beyond INT64_MAX
        assert route(desc(cls, G=1 << 31, M=1, N=1, K=1)) == ARG                        # more work-groups than a grid holds
    assert lib.qs_mx_bmm_route(desc(_hip.MxBmmArgs, y=None)) == ARG
    assert lib.qs_mx_bmm_route(desc(_hip.MxBmmArgs, ydt=7, y=(1 << 20) + 1, G=-1)) == ARG        # the arguments come before the dtype
    assert lib.qs_mx_bmm_route(desc(_hip.MxBmmArgs, ydt=7, y=(1 << 20) + 1)) == DTYPE            # ... the dtype before the alignment
    assert lib.qs_mx_bmm_route(desc(_hip.MxBmmArgs, y=(1 << 20) + 2)) == ALIGN
    assert lib.qs_mx_bmm_route(desc(_hip.MxBmmArgs, ydt=_hip._DT[torch.bfloat16], y=(1 << 20) + 2)) == _hip.MX_GEMM_ROUTE_VEC
    q = _hip.MxBmmQArgs
    assert lib.qs_mx_bmm_q_route(desc(q, out_scales=None)) == ARG and lib.qs_mx_bmm_q_route(desc(q, out_format=9)) == ARG
    assert lib.qs_mx_bmm_q_route(desc(q, act=2)) == ARG
    # out_codes [3, 5, 8] = 120 bytes may not share a byte with a_codes [3, 5, 64] = 960 bytes at 1024 or b_codes [3, 8, 64] at 4096
    assert lib.qs_mx_bmm_q_route(desc(q, out_codes=1024 + 959)) == ARG and lib.qs_mx_bmm_q_route(desc(q, out_codes=1024 + 960)) > 0
    assert lib.qs_mx_bmm_q_route(desc(q, out_codes=4096 - 120)) > 0 and lib.qs_mx_bmm_q_route(desc(q, out_codes=4096 - 119)) == ARG
    assert lib.qs_mx_bmm_q_route(desc(q, out_codes=4096 + 3 * 8 * 64 - 1)) == ARG       # the LAST slice of b_codes counts
