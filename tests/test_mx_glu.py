"""The gated (SwiGLU / GeGLU / ReGLU) products on MX codes without a GPU: the interleave, the CPU paths against the composition of public
calls they are defined as, the refusals, the layers, ``state_dict``, and the new C entry points' argument checks (which return before
anything is enqueued)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import qsparse_amd as qs
from qsparse_amd import (MXActivation, MXGatedMoEFeedForward, MXGLULinear, MXGroupedGLULinear, MXGroupedLinear, MXMoEFeedForward, _hip,
                         mx_bmm, mx_conv2d, mx_glu_deinterleave, mx_glu_interleave, mx_glu_matmul, mx_grouped_glu_matmul,
                         mx_grouped_matmul, mx_matmul, quantize_with_mx)
from qsparse_amd._mx_common import _act

ACTS = ("silu", "gelu", "relu")
FA, FB = "mxfp8_e4m3", "mxfp6_e2m3"


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def codes_of(x, fmt):
    return tuple(quantize_with_mx(x, fmt, -1, return_codes=True)[1:])


def act_ref(g, act):
    if act == "gelu":           # the header's expression op by op (ATen's vectorized CPU gelu is not within its bound: tests/mx_glu_ref.py)
        return (g * 0.5) * (1.0 + torch.erf(g * math.sqrt(0.5)))
    return F.silu(g) if act == "silu" else _act(g, "relu")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_interleave_layout_and_round_trip():
    g = torch.Generator().manual_seed(0)
    for shape in ((64, 5), (3, 96, 7), (2, 3, 32, 1)):
        gate, up = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
        both = mx_glu_interleave(gate, up)
        H = shape[-2]
        assert both.shape == shape[:-2] + (2 * H, shape[-1])
        for q in range(H // 32):
            assert torch.equal(both[..., 64 * q:64 * q + 32, :], gate[..., 32 * q:32 * q + 32, :])
            assert torch.equal(both[..., 64 * q + 32:64 * q + 64, :], up[..., 32 * q:32 * q + 32, :])
        back = mx_glu_deinterleave(both)
        assert torch.equal(back[0], gate) and torch.equal(back[1], up)
    # biases: [H], and stacked [E, H] with dim=-1; uint8 codes as well as floats
    bg, bu = torch.randn(64, generator=g), torch.randn(64, generator=g)
    b = mx_glu_interleave(bg, bu)
    assert b.shape == (128,) and torch.equal(b[:32], bg[:32]) and torch.equal(b[32:64], bu[:32]) and torch.equal(b[64:96], bg[32:])
    assert all(torch.equal(x, y) for x, y in zip(mx_glu_deinterleave(b), (bg, bu)))
    sg, su = torch.randn(4, 96, generator=g), torch.randn(4, 96, generator=g)
    sb = mx_glu_interleave(sg, su, dim=-1)
    assert sb.shape == (4, 192) and all(torch.equal(sb[e], mx_glu_interleave(sg[e], su[e])) for e in range(4))
    assert all(torch.equal(x, y) for x, y in zip(mx_glu_deinterleave(sb, dim=-1), (sg, su)))
    cg, cu = torch.randint(0, 256, (32, 9), dtype=torch.uint8, generator=g), torch.randint(0, 256, (32, 9), dtype=torch.uint8, generator=g)
    assert torch.equal(mx_glu_interleave(cg, cu), torch.cat((cg, cu)))
    # quantizing the interleaved weight is interleaving the codes: the blocks run along K
    w = codes_of(mx_glu_interleave(gate[0, 0].expand(32, 40).contiguous(), up[0, 0].expand(32, 40).contiguous()), FB)
    assert torch.equal(w[0], mx_glu_interleave(codes_of(gate[0, 0].expand(32, 40).contiguous(), FB)[0],
                                               codes_of(up[0, 0].expand(32, 40).contiguous(), FB)[0]))


def test_interleave_refuses_what_is_not_whole_corners():
    with pytest.raises(ValueError, match="one wave's corner"):
        mx_glu_interleave(torch.zeros(48, 8), torch.zeros(48, 8))
    with pytest.raises(ValueError, match="one wave's corner"):
        mx_glu_interleave(torch.zeros(4, 33), torch.zeros(4, 33), dim=-1)
    with pytest.raises(ValueError, match="one wave's corner"):
        mx_glu_deinterleave(torch.zeros(96, 8))
    with pytest.raises(ValueError, match="agree"):
        mx_glu_interleave(torch.zeros(32, 8), torch.zeros(32, 9))
    with pytest.raises(ValueError, match="out of range"):
        mx_glu_interleave(torch.zeros(32, 8), torch.zeros(32, 8), dim=2)
    with pytest.raises(TypeError):
        mx_glu_deinterleave([1, 2])


def dense_case(seed=1, M=37, H=64, K=72):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 2
    w = mx_glu_interleave(torch.randn(H, K, generator=g) / K ** 0.5, torch.randn(H, K, generator=g) / K ** 0.5)
    bias = mx_glu_interleave(torch.randn(H, generator=g), torch.randn(H, generator=g))
    return codes_of(x, FA) + codes_of(w, FB) + (bias,)


@pytest.mark.parametrize("act", ACTS)
def test_dense_cpu_path_is_the_composition(act):
    ops = dense_case()
    for bias in (ops[4], None):
        v = mx_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, bias)
        g, u = mx_glu_deinterleave(v, dim=-1)
        z = act_ref(g, act) * u
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            assert same(mx_glu_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, bias, dt, act=act), z.to(dt))
        for f in ("mxfp8_e4m3", "mxfp4_e2m1"):
            got = mx_glu_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, bias, act=act, out_fmt=f)
            assert all(torch.equal(a, b) for a, b in zip(got, codes_of(z, f))) and got[1].shape == (37, 2)
    # leading dimensions pass through
    y = mx_glu_matmul(ops[0][:36].reshape(4, 9, -1), ops[1][:36].reshape(4, 9, -1), FA, ops[2], ops[3], FB, ops[4], act=act)
    assert y.shape == (4, 9, 64) and same(y.reshape(36, 64), mx_glu_matmul(ops[0][:36], ops[1][:36], FA, ops[2], ops[3], FB, ops[4], act=act))


def grouped_case(seed=2, T=50, E=3, H=32, K=40):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, K, generator=g) * 2
    w = mx_glu_interleave(torch.randn(E, H, K, generator=g) / K ** 0.5, torch.randn(E, H, K, generator=g) / K ** 0.5)
    bias = mx_glu_interleave(torch.randn(E, H, generator=g), torch.randn(E, H, generator=g), dim=-1)
    return codes_of(x, FA) + codes_of(w, FB) + (bias,)


@pytest.mark.parametrize("act", ACTS)
def test_grouped_cpu_path_is_the_composition(act):
    ops = grouped_case()
    offs = torch.tensor([20, 20, 41])          # an empty group, 9 tail rows
    for bias in (ops[4], ops[4][1].contiguous(), None):
        v = mx_grouped_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, offs, bias)
        g, u = mx_glu_deinterleave(v, dim=-1)
        z = act_ref(g, act) * u
        assert same(mx_grouped_glu_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, offs, bias, act=act), z)
        assert same(mx_grouped_glu_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, offs, bias, torch.bfloat16, act=act), z.bfloat16())
        assert z[41:].eq(0).all() and not torch.signbit(z[41:]).any()
        codes, scales = mx_grouped_glu_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, offs, bias, act=act, out_fmt="mxfp6_e3m2")
        want = codes_of(z, "mxfp6_e3m2")
        assert torch.equal(codes, want[0]) and torch.equal(scales, want[1])
        assert not codes[41:].any() and not scales[41:].any()
        # a group is the dense product with its weight
        be = None if bias is None else bias if bias.dim() == 1 else bias[2]
        assert same(z[20:41], mx_glu_matmul(ops[0][20:41], ops[1][20:41], FA, ops[2][2], ops[3][2], FB, be, act=act))


def test_refusals():
    ops = dense_case()
    call = lambda *a, **kw: mx_glu_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, *a, **kw)
    for act in (None, "tanh", "swish", 1):
        with pytest.raises(ValueError, match="unknown act"):
            call(act=act)
    with pytest.raises(ValueError, match="one wave's corner"):          # N / 32 odd
        mx_glu_matmul(ops[0], ops[1], FA, ops[2][:96], ops[3][:96], FB)
    with pytest.raises(ValueError, match="cannot be combined"):
        call(None, torch.bfloat16, out_fmt="mxfp8_e4m3")
    with pytest.raises(ValueError, match="unknown MX format|mxfp"):
        call(out_fmt="fp8")
    with pytest.raises(TypeError):
        call(None, torch.float64)
    with pytest.raises(ValueError, match="disagree on K"):
        mx_glu_matmul(ops[0][:, :40], ops[1][:, :2], FA, ops[2], ops[3], FB)
    with pytest.raises(ValueError, match="bias has shape"):
        call(ops[4][:64])
    with pytest.raises(ValueError, match="a_scales has shape"):
        mx_glu_matmul(ops[0], ops[1][:, :1], FA, ops[2], ops[3], FB)
    with pytest.raises(ValueError, match="is on"):
        mx_glu_matmul(ops[0], ops[1], FA, ops[2].to("meta"), ops[3].to("meta"), FB)
    with pytest.raises(TypeError):
        mx_glu_matmul(ops[0].float(), ops[1], FA, ops[2], ops[3], FB)


def test_grouped_refusals_are_those_of_mx_grouped_matmul():
    ops = grouped_case()
    for offs, exc in ((torch.tensor([20, 10, 41]), ValueError), (torch.tensor([20, 30, 51]), ValueError), (torch.tensor([-1, 30, 41]), ValueError),
                      (torch.tensor([20, 41]), ValueError), (torch.tensor([20.0, 30.0, 41.0]), TypeError), ([20, 30, 41], TypeError),
                      (torch.tensor([20, 30, 41], device="meta"), ValueError)):
        with pytest.raises(exc) as glu:
            mx_grouped_glu_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, offs)
        with pytest.raises(exc) as plain:
            mx_grouped_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, offs)
        assert str(glu.value) == str(plain.value)
    with pytest.raises(ValueError, match="unknown act"):
        mx_grouped_glu_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, torch.tensor([20, 30, 41]), act=None)
    with pytest.raises(ValueError, match="one weight per group"):
        mx_grouped_glu_matmul(ops[0], ops[1], FA, ops[2][0], ops[3][0], FB, torch.tensor([20]))
    with pytest.raises(ValueError, match="bias has shape"):
        mx_grouped_glu_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, torch.tensor([20, 30, 41]), ops[4][:2])


def test_existing_products_still_refuse_gelu():
    ops = dense_case()
    c = torch.zeros(1, 4, 4, 32, dtype=torch.uint8), torch.zeros(1, 4, 4, 1, dtype=torch.uint8)
    w = torch.zeros(8, 1, 1, 32, dtype=torch.uint8), torch.zeros(8, 1, 1, 1, dtype=torch.uint8)
    for act in ("gelu", "silu"):
        with pytest.raises(ValueError, match="unknown act"):
            mx_matmul(ops[0], ops[1], FA, ops[2], ops[3], FB, out_fmt="mxfp8_e4m3", act=act)
        with pytest.raises(ValueError, match="unknown act"):
            mx_bmm(ops[0][None], ops[1][None], FA, ops[2][None], ops[3][None], FB, out_fmt="mxfp8_e4m3", act=act)
        with pytest.raises(ValueError, match="unknown act"):
            mx_conv2d(c[0], c[1], FA, w[0], w[1], FA, out_fmt="mxfp8_e4m3", act=act)
        with pytest.raises(ValueError, match="unknown act"):
            mx_grouped_matmul(ops[0], ops[1], FA, ops[2][None], ops[3][None], FB, torch.tensor([37]), out_fmt="mxfp8_e4m3", act=act)


def test_layers_equal_the_functional_calls_and_round_trip_their_state():
    g = torch.Generator().manual_seed(3)
    H, K, E = 64, 72, 3
    rnd = lambda *s: torch.randn(*s, generator=g)
    wg, wu, bg, bu = rnd(H, K) / 8, rnd(H, K) / 8, rnd(H), rnd(H)
    x = rnd(2, 9, K) * 2
    xc = codes_of(x, "mxfp8_e5m2")
    wc = codes_of(mx_glu_interleave(wg, wu), FB)
    for act in ACTS:
        lin = MXGLULinear.from_float(wg, wu, bg, bu, FB, "mxfp8_e5m2", act=act, out_dtype=torch.bfloat16)
        assert torch.equal(lin.weight_codes, wc[0]) and torch.equal(lin.bias, mx_glu_interleave(bg, bu))
        assert (lin.in_features, lin.out_features) == (K, H) and f"act={act!r}" in repr(lin)
        want = mx_glu_matmul(xc[0], xc[1], "mxfp8_e5m2", wc[0], wc[1], FB, mx_glu_interleave(bg, bu), torch.bfloat16, act=act)
        assert same(lin(x), want) and same(lin(MXActivation(xc[0], xc[1], "mxfp8_e5m2")), want)
    lin = MXGLULinear.from_float(wg, wu, w_fmt=FB, out_fmt="mxfp4_e2m1")
    out = lin(x)
    want = mx_glu_matmul(*codes_of(x, "mxfp8_e4m3"), "mxfp8_e4m3", wc[0], wc[1], FB, out_fmt="mxfp4_e2m1")
    assert isinstance(out, MXActivation) and out.fmt == "mxfp4_e2m1" and torch.equal(out.codes, want[0]) and torch.equal(out.scales, want[1])
    other = MXGLULinear.from_float(torch.zeros(H, K), torch.zeros(H, K), w_fmt=FB, out_fmt="mxfp4_e2m1")
    other.load_state_dict(lin.state_dict())
    assert sorted(lin.state_dict()) == ["weight_codes", "weight_scales"] and torch.equal(other(x).codes, out.codes)
    with pytest.raises(RuntimeError, match="inference layer"):
        lin(x.clone().requires_grad_())
    with pytest.raises(ValueError, match="both"):
        MXGLULinear.from_float(wg, wu, bg, None)
    with pytest.raises(ValueError, match="one wave's corner"):
        MXGLULinear.from_float(wg[:48], wu[:48])
    # grouped
    gw, gu, gbg, gbu = rnd(E, H, K) / 8, rnd(E, H, K) / 8, rnd(E, H), rnd(E, H)
    glin = MXGroupedGLULinear.from_float(gw, gu, gbg, gbu, FB, act="gelu", out_fmt="mxfp8_e4m3")
    rows, offs = rnd(30, K), torch.tensor([7, 7, 25])
    gc = codes_of(mx_glu_interleave(gw, gu), FB)
    want = mx_grouped_glu_matmul(*codes_of(rows, "mxfp8_e4m3"), "mxfp8_e4m3", gc[0], gc[1], FB, offs, mx_glu_interleave(gbg, gbu, dim=-1),
                                 act="gelu", out_fmt="mxfp8_e4m3")
    out = glin(rows, offs)
    assert torch.equal(out.codes, want[0]) and torch.equal(out.scales, want[1])
    assert (glin.num_groups, glin.in_features, glin.out_features) == (E, K, H)
    other = MXGroupedGLULinear.from_float(torch.zeros_like(gw), torch.zeros_like(gu), gbg, gbu, FB, act="gelu", out_fmt="mxfp8_e4m3")
    other.load_state_dict(glin.state_dict())
    assert torch.equal(other(rows, offs).codes, out.codes)
    for e in range(E):          # the same per group
        one = MXGLULinear.from_float(gw[e], gu[e], gbg[e], gbu[e], FB, act="gelu", out_fmt="mxfp8_e4m3")
        assert torch.equal(one.weight_codes, glin.weight_codes[e]) and torch.equal(one.bias, glin.bias[e])


def test_from_exported_takes_the_interleaved_weight():
    g = torch.Generator().manual_seed(4)
    w = mx_glu_interleave(torch.randn(32, 40, generator=g), torch.randn(32, 40, generator=g))
    _, codes, scales = quantize_with_mx(w, FB, -1, return_codes=True)

    class QT:
        kind, fmt, block_dim = "mx", FB, 1

    QT.codes, QT.block_scale = codes, scales
    lin = MXGLULinear.from_exported(QT, act="relu")
    x = torch.randn(5, 40, generator=g)
    assert same(lin(x), mx_glu_matmul(*codes_of(x, "mxfp8_e4m3"), "mxfp8_e4m3", codes, scales, FB, act="relu"))
    QT.block_dim = 0
    with pytest.raises(ValueError, match="along K"):
        MXGLULinear.from_exported(QT)
    QT.kind = "int"
    with pytest.raises(ValueError, match="MX weight"):
        MXGroupedGLULinear.from_exported(QT)


@pytest.mark.parametrize("act", ACTS)
def test_gated_moe_block_is_its_composition(act):
    g = torch.Generator().manual_seed(8)
    T, D, H, E, k = 40, 48, 64, 4, 2
    rnd = lambda *s: torch.randn(*s, generator=g)
    router, wg, bg, wu, bu, wd, bd = rnd(E, D), rnd(E, H, D) / 7, rnd(E, H), rnd(E, H, D) / 7, rnd(E, H), rnd(E, D, H) / 8, rnd(E, D)
    moe = MXGatedMoEFeedForward.from_float(router, wg, bg, wu, bu, wd, bd, k, "mxfp8_e4m3", "mxfp8_e4m3", "mxfp6_e2m3", act=act)
    assert isinstance(moe, MXMoEFeedForward) and isinstance(moe.up, MXGroupedGLULinear) and moe.hidden_dim == H
    x = rnd(T, D)
    top, ids = torch.topk(x @ router.t(), k, -1)
    order = torch.argsort(ids.reshape(-1), stable=True)
    offs = (ids.reshape(-1).unsqueeze(1) == torch.arange(E)).sum(0).cumsum(0).to(torch.int32)
    rows = codes_of(x[torch.div(order, k, rounding_mode="floor")], "mxfp8_e4m3")
    wc = codes_of(mx_glu_interleave(wg, wu), "mxfp8_e4m3")
    hidden = mx_grouped_glu_matmul(rows[0], rows[1], "mxfp8_e4m3", wc[0], wc[1], "mxfp8_e4m3", offs, mx_glu_interleave(bg, bu, dim=-1),
                                   act=act, out_fmt="mxfp6_e2m3")
    dc = codes_of(wd, "mxfp8_e4m3")
    y = mx_grouped_matmul(hidden[0], hidden[1], "mxfp6_e2m3", dc[0], dc[1], "mxfp8_e4m3", offs, bd)
    want = (y[torch.argsort(order)].reshape(-1, k, D) * torch.softmax(top, -1).unsqueeze(-1)).sum(1)
    assert same(moe(x), want)
    assert same(moe(MXActivation(*codes_of(x, "mxfp8_e4m3"), "mxfp8_e4m3")), moe(MXActivation(*codes_of(x, "mxfp8_e4m3"), "mxfp8_e4m3")))
    keys = ["down.bias", "down.weight_codes", "down.weight_scales", "router", "up.bias", "up.weight_codes", "up.weight_scales"]
    assert sorted(moe.state_dict()) == keys and torch.equal(moe.state_dict()["up.weight_codes"], wc[0])
    z = torch.zeros
    other = MXGatedMoEFeedForward.from_float(z(E, D), z(E, H, D), z(E, H), z(E, H, D), z(E, H), z(E, D, H), z(E, D), k, hidden_fmt="mxfp6_e2m3",
                                             act=act)
    other.load_state_dict(moe.state_dict())
    assert same(other(x), want)
    # the types: each block takes its own kind of `up`
    down = MXGroupedLinear.from_float(wd, bd, "mxfp8_e4m3", "mxfp6_e2m3")
    with pytest.raises(TypeError, match="MXGroupedGLULinear"):
        MXGatedMoEFeedForward(router, MXGroupedLinear.from_float(wg, bg, out_fmt="mxfp6_e2m3", act="relu"), down, k)
    with pytest.raises(TypeError, match="up and down must be MXGroupedLinear layers"):
        MXMoEFeedForward(router, moe.up, down, k)
    with pytest.raises(ValueError, match="hand out MX codes"):
        MXGatedMoEFeedForward(router, MXGroupedGLULinear.from_float(wg, wu), down, k)


# ---- the C entry points: bad descriptors return QS_ERR_* with nothing enqueued (no GPU is touched) -------------------------------------
OK, ERR_DTYPE, ERR_ARG, ERR_ALIGN = 0, -1, -2, -3


def dense_args(**kw):
    a = _hip.MxGluMatmulArgs()
    a.struct_size = ctypes.sizeof(a)
    a.a_codes, a.a_scales, a.b_codes, a.b_scales = 0x10000, 0x20000, 0x30000, 0x40000
    a.out_format, a.act, a.y, a.ydt = -1, 1, 0x50000, 0
    a.M, a.H, a.K = 4, 32, 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def grouped_args(**kw):
    a = _hip.MxGroupedGluMatmulArgs()
    a.struct_size = ctypes.sizeof(a)
    a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.offs = 0x10000, 0x20000, 0x30000, 0x40000, 0x60000
    a.out_format, a.act, a.y, a.ydt = -1, 1, 0x50000, 0
    a.T, a.E, a.H, a.K = 4, 2, 32, 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD = [(dict(H=48), ERR_ARG), (dict(H=-32), ERR_ARG), (dict(act=3), ERR_ARG), (dict(act=-1), ERR_ARG), (dict(out_format=5), ERR_ARG),
       (dict(out_format=-2), ERR_ARG), (dict(y=0), ERR_ARG), (dict(out_format=0), ERR_ARG),          # codes asked for, no out_codes
       (dict(out_format=0, out_codes=0x50000), ERR_ARG), (dict(a_codes=0), ERR_ARG), (dict(b_scales=0), ERR_ARG), (dict(a_format=5), ERR_ARG),
       (dict(K=-1), ERR_ARG), (dict(ydt=7), ERR_DTYPE), (dict(ydt=7, H=48), ERR_ARG),                 # ARG comes before DTYPE
       (dict(y=0x50002), ERR_ALIGN), (dict(bias=0x70001), ERR_ALIGN), (dict(ydt=7, bias=0x70001), ERR_DTYPE),      # DTYPE before ALIGN
       (dict(K=0), ERR_ARG), (dict(y=0x10000), ERR_ARG), (dict(y=0x30000 + 64 * 64 - 4), ERR_ARG),   # y on a_codes, on the last bytes of b_codes
       (dict(out_format=2, out_codes=0x50000, out_scales=0x10000 + 255), ERR_ARG)]                  # the scales on a_codes' last byte


def test_c_entry_points_refuse_bad_descriptors_without_a_gpu():
    lib = _hip.load()
    for v, route, make in ((lib.qs_mx_glu_matmul_v, lib.qs_mx_glu_matmul_route, dense_args),
                           (lib.qs_mx_grouped_glu_matmul_v, lib.qs_mx_grouped_glu_matmul_route, grouped_args)):
        assert v(None) == ERR_ARG and route(None) == ERR_ARG
        short = make()
        short.struct_size = 2
        assert v(ctypes.byref(short)) == ERR_ARG
        for kw, status in BAD:
            a = make(**kw)
            assert v(ctypes.byref(a)) == status and route(ctypes.byref(a)) == status, kw
        # an empty product: nothing enqueued, 0 -- but only after the checks
        for kw in (dict(H=0), {"M" if make is dense_args else "T": 0}):
            a = make(**kw)
            assert v(ctypes.byref(a)) == OK and route(ctypes.byref(a)) == OK
        assert v(ctypes.byref(make(H=0, act=9))) == ERR_ARG
        # the routes of the ungated product, by the same conditions on the inputs
        assert route(ctypes.byref(make())) == _hip.MX_GEMM_ROUTE_VEC
        assert route(ctypes.byref(make(K=72))) == _hip.MX_GEMM_ROUTE_PLAIN
        assert route(ctypes.byref(make(a_codes=0x10001))) == _hip.MX_GEMM_ROUTE_PLAIN
        assert route(ctypes.byref(make(out_format=4, out_codes=0x50001, out_scales=0x58001))) == _hip.MX_GEMM_ROUTE_VEC
    lib = _hip.load()
    g = grouped_args
    for kw, status in ((dict(offs=0), ERR_ARG), (dict(offs=0x60002), ERR_ALIGN), (dict(E=4097), ERR_ARG), (dict(bias=0x70000, bias_batch_stride=32), ERR_ARG),
                       (dict(bias=0x70000, bias_batch_stride=64), 1), (dict(E=0, b_codes=0, b_scales=0, offs=0), 1)):
        assert lib.qs_mx_grouped_glu_matmul_route(ctypes.byref(g(**kw))) == status, kw


def test_descriptor_structs_have_the_headers_layout(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = {"qs_mx_glu_matmul_args": _hip.MxGluMatmulArgs, "qs_mx_grouped_glu_matmul_args": _hip.MxGroupedGluMatmulArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(root, "include", "qsparse_hip.h")}"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append(f'printf("%zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {f}));' for f, _ in ct._fields_]
        lines.append('printf("\\n");')
    (tmp_path / "layout.c").write_text("\n".join(lines + ['return 0; }']))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    for line, ct in zip(out, pairs.values()):
        size, *offsets = (int(t) for t in line.split())
        assert size == ctypes.sizeof(ct) and offsets == [getattr(ct, f).offset for f, _ in ct._fields_]
