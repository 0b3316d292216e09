"""Training through the gated MX products without a GPU: argument refusals, the interleaved layers, the CPU paths against the
composition written out from public calls, the C ABI of the new entry points, and the definition of ``dv`` against float64."""
import ctypes
import math

import pytest
import torch

import qsparse_amd as qs
from qsparse_amd import (MXGatedMoEFeedForward, MXGLULinear, MXGroupedGLULinear, MXTrainGatedMoEFeedForward, MXTrainGLULinear,
                         MXTrainGroupedGLULinear, MXTrainMoEFeedForward, _hip, mx_glu_backward_quantize, mx_glu_deinterleave,
                         mx_glu_interleave, mx_glu_linear, mx_glu_matmul, mx_grouped_glu_linear, mx_grouped_glu_matmul, mx_grouped_matmul,
                         mx_grouped_weight_grad, mx_matmul, mx_quantize_2way, quantize_with_mx)
from qsparse_amd.mx_batched_train import mx_quantize_2way_batched
from qsparse_amd.mx_glu_train import _glu_dv
from qsparse_amd.mx_grouped_train import _group_membership

ACTS = ("silu", "gelu", "relu")
ERR_DTYPE, ERR_ARG, ERR_ALIGN = -1, -2, -3


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def codes_of(x, fmt):
    return tuple(quantize_with_mx(x, fmt, -1, return_codes=True)[1:])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_backward_quantize_refusals():
    dh, v = rnd(1, 4, 32), rnd(2, 4, 64)
    ok = dict(act="silu", row_fmt="mxfp8_e5m2")
    with pytest.raises(ValueError, match="multiple of 32"):
        mx_glu_backward_quantize(rnd(1, 4, 16), rnd(2, 4, 32), **ok)
    with pytest.raises(ValueError, match=r"\[T, 2 H\]"):
        mx_glu_backward_quantize(dh, rnd(2, 4, 32), **ok)
    with pytest.raises(ValueError, match=r"\[T, 2 H\]"):
        mx_glu_backward_quantize(dh, rnd(2, 5, 64), **ok)
    with pytest.raises(TypeError):
        mx_glu_backward_quantize(dh.double(), v, **ok)
    with pytest.raises(TypeError):
        mx_glu_backward_quantize(dh, v.to(torch.int32), **ok)
    with pytest.raises(ValueError, match="unknown act"):
        mx_glu_backward_quantize(dh, v, act="tanh", row_fmt="mxfp8_e5m2")
    with pytest.raises(ValueError, match="row_fmt, col_fmt or both"):
        mx_glu_backward_quantize(dh, v, act="silu")
    with pytest.raises(ValueError):
        mx_glu_backward_quantize(dh, v, act="silu", row_fmt="fp8")
    with pytest.raises(ValueError, match="but v on"):
        mx_glu_backward_quantize(dh, v.to("meta"), **ok)


def test_function_and_layer_refusals():
    x = rnd(3, 4, 40)
    with pytest.raises(ValueError, match="interleave"):
        mx_glu_linear(x, rnd(4, 96, 40))                  # 96 rows: H = 48 is no multiple of 32
    with pytest.raises(ValueError, match="interleave"):
        mx_grouped_glu_linear(x, rnd(4, 2, 32, 40), torch.tensor([2, 4]))
    with pytest.raises(ValueError, match="disagree on K"):
        mx_glu_linear(x, rnd(4, 64, 48))
    with pytest.raises(TypeError):
        mx_glu_linear(x.double(), rnd(4, 64, 40))
    with pytest.raises(TypeError, match="preact_dtype"):
        mx_glu_linear(x, rnd(4, 64, 40), preact_dtype=torch.float64)
    with pytest.raises(ValueError, match="unknown act"):
        mx_glu_linear(x, rnd(4, 64, 40), act="swish")
    with pytest.raises(ValueError, match="bias has shape"):
        mx_glu_linear(x, rnd(4, 64, 40), rnd(5, 32))
    with pytest.raises(ValueError, match="but weight on"):
        mx_glu_linear(x, rnd(4, 64, 40).to("meta"))
    with pytest.raises(ValueError, match="offs has shape"):
        mx_grouped_glu_linear(x, rnd(4, 2, 64, 40), torch.tensor([2, 3, 4]))
    with pytest.raises(ValueError, match="multiple of 32"):
        MXTrainGLULinear.from_float(rnd(1, 48, 40), rnd(2, 48, 40))
    with pytest.raises(ValueError, match="both be given"):
        MXTrainGLULinear.from_float(rnd(1, 32, 40), rnd(2, 32, 40), rnd(3, 32), None)
    with pytest.raises(TypeError, match="MXTrainGroupedGLULinear"):
        MXTrainGatedMoEFeedForward(rnd(1, 2, 40), qs.MXTrainGroupedLinear(2, 40, 32), qs.MXTrainGroupedLinear(2, 32, 40), 1)
    a = codes_of(rnd(6, 4, 64), "mxfp8_e4m3")
    b = codes_of(rnd(7, 64, 64), "mxfp8_e4m3")
    with pytest.raises(TypeError, match="preact_dtype"):
        mx_glu_matmul(a[0], a[1], "mxfp8_e4m3", b[0], b[1], "mxfp8_e4m3", preact_dtype=torch.float64)
    be = codes_of(rnd(7, 2, 64, 64), "mxfp8_e4m3")
    with pytest.raises(TypeError, match="preact_dtype"):
        mx_grouped_glu_matmul(a[0], a[1], "mxfp8_e4m3", be[0], be[1], "mxfp8_e4m3", torch.tensor([2, 4]), preact_dtype=torch.int8)


# ---- the products' preact_dtype on the CPU ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdt", [torch.float32, torch.bfloat16])
def test_cpu_products_with_preact_dtype(vdt):
    fa, fb = "mxfp8_e4m3", "mxfp6_e2m3"
    a, b = codes_of(rnd(8, 6, 72), fa), codes_of(mx_glu_interleave(rnd(9, 32, 72), rnd(10, 32, 72)), fb)
    bias = rnd(11, 64)
    args = (a[0], a[1], fa, b[0], b[1], fb, bias)
    out, v = mx_glu_matmul(*args, act="gelu", preact_dtype=vdt)
    assert torch.equal(out, mx_glu_matmul(*args, act="gelu")) and torch.equal(v, mx_matmul(*args, vdt))
    (c, s), v = mx_glu_matmul(*args, act="silu", out_fmt="mxfp8_e4m3", preact_dtype=vdt)
    want = mx_glu_matmul(*args, act="silu", out_fmt="mxfp8_e4m3")
    assert torch.equal(c, want[0]) and torch.equal(s, want[1]) and v.dtype == vdt and v.shape == (6, 64)
    be = codes_of(mx_glu_interleave(rnd(9, 2, 32, 72), rnd(10, 2, 32, 72)), fb)
    offs = torch.tensor([2, 5])
    gargs = (a[0], a[1], fa, be[0], be[1], fb, offs, None)
    out, v = mx_grouped_glu_matmul(*gargs, act="relu", preact_dtype=vdt)
    assert torch.equal(out, mx_grouped_glu_matmul(*gargs, act="relu")) and torch.equal(v, mx_grouped_matmul(*gargs, vdt))
    assert not v[5:].any()


# ---- layers ---------------------------------------------------------------------------------------------------------------------------
def test_from_float_round_trip_state_dict_and_inference_bytes():
    wg, wu, bg, bu = rnd(1, 64, 40), rnd(2, 64, 40), rnd(3, 64), rnd(4, 64)
    layer = MXTrainGLULinear.from_float(wg, wu, bg, bu, act="gelu", w_fmt="mxfp6_e3m2")
    assert list(layer.state_dict()) == ["weight", "bias"] and layer.weight.shape == (128, 40) and layer.bias.shape == (128,)
    assert torch.equal(layer.weight, mx_glu_interleave(wg, wu)) and isinstance(layer.weight, torch.nn.Parameter)
    got = layer.gate_up()
    assert all(torch.equal(a, b) for a, b in zip(got, (wg, wu, bg, bu)))
    assert (layer.in_features, layer.out_features) == (40, 64)
    inf = layer.to_inference()
    assert isinstance(inf, MXGLULinear) and inf.act == "gelu" and inf.weight_fmt == "mxfp6_e3m2"
    ref = MXGLULinear.from_float(wg, wu, bg, bu, "mxfp6_e3m2", act="gelu")
    assert torch.equal(inf.weight_codes, ref.weight_codes) and torch.equal(inf.weight_scales, ref.weight_scales)
    assert torch.equal(inf.bias, ref.bias)
    nob = MXTrainGLULinear.from_float(wg, wu)
    assert list(nob.state_dict()) == ["weight"] and nob.gate_up()[2:] == (None, None)
    sr = MXTrainGLULinear.from_float(wg, wu, grad_rounding="stochastic", seed=3)
    assert list(sr.state_dict()) == ["weight"] and sr.sr_seed == 3 and int(sr.sr_step) == 0

    E = 3
    wg, wu, bg, bu = rnd(1, E, 32, 40), rnd(2, E, 32, 40), rnd(3, E, 32), rnd(4, E, 32)
    grouped = MXTrainGroupedGLULinear.from_float(wg, wu, bg, bu)
    assert list(grouped.state_dict()) == ["weight", "bias"] and grouped.weight.shape == (E, 64, 40) and grouped.bias.shape == (E, 64)
    assert all(torch.equal(a, b) for a, b in zip(grouped.gate_up(), (wg, wu, bg, bu)))
    assert (grouped.num_groups, grouped.in_features, grouped.out_features) == (E, 40, 32)
    inf = grouped.to_inference(out_fmt="mxfp8_e4m3")
    ref = MXGroupedGLULinear.from_float(wg, wu, bg, bu, out_fmt="mxfp8_e4m3")
    assert isinstance(inf, MXGroupedGLULinear) and inf.out_fmt == "mxfp8_e4m3"
    assert torch.equal(inf.weight_codes, ref.weight_codes) and torch.equal(inf.weight_scales, ref.weight_scales)
    assert torch.equal(inf.bias, ref.bias)


def test_gated_moe_layer_on_the_cpu():
    E, D, H, k, T = 3, 40, 32, 2, 9
    args = (rnd(1, E, D), rnd(2, E, H, D), rnd(3, E, H), rnd(4, E, H, D), rnd(5, E, H), rnd(6, E, D, H), rnd(7, E, D), k)
    moe = MXTrainGatedMoEFeedForward.from_float(*args, act="silu")
    assert isinstance(moe, MXTrainMoEFeedForward) and MXTrainGatedMoEFeedForward.forward is MXTrainMoEFeedForward.forward
    assert list(moe.state_dict()) == ["router", "up.weight", "up.bias", "down.weight", "down.bias"]
    x = rnd(8, T, D).requires_grad_(True)
    y = moe(x)
    inf = moe.to_inference()
    assert isinstance(inf, MXGatedMoEFeedForward) and torch.equal(y.detach(), inf(x.detach()))
    ref = MXGatedMoEFeedForward.from_float(*args, act="silu")
    assert torch.equal(inf(x.detach()), ref(x.detach()))
    y.sum().backward()
    assert x.grad.shape == x.shape and moe.up.weight.grad.shape == (E, 2 * H, D) and moe.router.grad is not None
    # the ungated block is what it was
    plain = MXTrainMoEFeedForward.from_float(args[0], args[1], args[2], args[5], args[6], k)
    assert plain._hidden_act == "relu" and torch.equal(plain(x.detach()), plain.to_inference()(x.detach()))


# ---- the CPU paths against the written-out composition -------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
def test_cpu_mx_glu_linear_is_the_composition(act):
    T, H, K = 37, 32, 72
    fx, fw, fg = "mxfp8_e4m3", "mxfp6_e3m2", "mxfp8_e5m2"
    w = mx_glu_interleave(rnd(1, H, K) / 8, rnd(2, H, K) / 8).requires_grad_(True)
    b = rnd(3, 2 * H).requires_grad_(True)
    x, dh = rnd(4, T, K).requires_grad_(True), rnd(5, T, H)
    h = mx_glu_linear(x, w, b, act=act, x_fmt=fx, w_fmt=fw, grad_fmt=fg)
    h.backward(dh)
    x_row, x_rs, x_col, x_cs = mx_quantize_2way(x.detach(), fx, fx)
    w_row, w_rs, w_col, w_cs = mx_quantize_2way(w.detach(), fw, fw)
    assert torch.equal(h.detach(), mx_glu_matmul(x_row, x_rs, fx, w_row, w_rs, fw, b.detach(), act=act))
    v = mx_matmul(x_row, x_rs, fx, w_row, w_rs, fw, b.detach())
    dv = _glu_dv(dh, v, act)
    g_row, g_rs, g_col, g_cs = mx_quantize_2way(dv, fg, fg)
    got = mx_glu_backward_quantize(dh, v, act=act, row_fmt=fg, col_fmt=fg)
    assert all(torch.equal(a, c) for a, c in zip(got, (g_row, g_rs, g_col, g_cs)))
    assert torch.equal(x.grad, mx_matmul(g_row, g_rs, fg, w_col, w_cs, fw))
    assert torch.equal(w.grad, mx_matmul(g_col, g_cs, fg, x_col, x_cs, fx))
    assert torch.equal(b.grad, dv.sum(0, dtype=torch.float32))
    # gradients nobody asks for are None; without grad nothing is kept
    y = mx_glu_linear(x.detach(), w, None, act=act, x_fmt=fx, w_fmt=fw, grad_fmt=fg)
    assert torch.autograd.grad(y, w, dh)[0].shape == w.shape
    with torch.no_grad():
        assert not mx_glu_linear(x, w, b, act=act).requires_grad


def test_cpu_mx_grouped_glu_linear_is_the_composition():
    T, H, K, E = 37, 32, 72, 3
    fx, fw, fg = "mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2"
    w = mx_glu_interleave(rnd(1, E, H, K) / 8, rnd(2, E, H, K) / 8).requires_grad_(True)
    b = rnd(3, E, 2 * H).requires_grad_(True)
    x, dh, offs = rnd(4, T, K).requires_grad_(True), rnd(5, T, H), torch.tensor([10, 10, 30])
    h = mx_grouped_glu_linear(x, w, offs, b, act="silu", x_fmt=fx, w_fmt=fw, grad_fmt=fg)
    h.backward(dh)
    x_row, x_rs, x_col, x_cs = mx_quantize_2way(x.detach(), fx, fx)
    w_row, w_rs, w_col, w_cs = mx_quantize_2way_batched(w.detach(), fw, fw)
    v = mx_grouped_matmul(x_row, x_rs, fx, w_row, w_rs, fw, offs, b.detach())
    dv = _glu_dv(dh, v, "silu")
    g_row, g_rs, g_col, g_cs = mx_quantize_2way(dv, fg, fg)
    assert not h[30:].any()
    assert torch.equal(x.grad, mx_grouped_matmul(g_row, g_rs, fg, w_col, w_cs, fw, offs))
    assert torch.equal(w.grad, mx_grouped_weight_grad(g_col, g_cs, fg, x_col, x_cs, fx, offs))
    assert torch.equal(b.grad, _group_membership(offs, T) @ dv) and not b.grad[1].any()


@pytest.mark.parametrize("grouped", [False, True])
def test_cpu_stochastic_rounding_repeats_and_moves_on(grouped):
    E = 3
    lead = (E,) if grouped else ()
    w = mx_glu_interleave(rnd(1, *lead, 32, 64) / 8, rnd(2, *lead, 32, 64) / 8).requires_grad_(True)
    x, dh, offs = rnd(4, 16, 64), rnd(5, 16, 32), torch.tensor([5, 5, 14])

    def run(step):
        xl = x.clone().requires_grad_(True)
        w.grad = None
        kw = dict(grad_fmt="mxfp4_e2m1", grad_rounding="stochastic", seed=7, step=step)
        (mx_grouped_glu_linear(xl, w, offs, None, **kw) if grouped else mx_glu_linear(xl, w, None, **kw)).backward(dh)
        return xl.grad, w.grad

    step = torch.zeros(1, dtype=torch.int64)
    a, b, c = run(step), run(torch.zeros(1, dtype=torch.int64)), run(step)
    assert int(step) == 2
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("qs_mx_glu_matmul_pre_v", "qs_mx_glu_matmul_pre_route", "qs_mx_grouped_glu_matmul_pre_v",
               "qs_mx_grouped_glu_matmul_pre_route", "qs_mx_glu_bwd_quant2_v", "qs_mx_glu_bwd_quant2_route")


def bwd_args(**kw):
    a = _hip.MxGluBwdQuant2Args()
    a.struct_size = ctypes.sizeof(a)
    a.row_format, a.col_format, a.act = 1, 1, 1
    a.dh, a.v, a.dhdt, a.vdt = 0x10000, 0x20000, 1, 0
    a.row_codes, a.row_scales, a.col_codes, a.col_scales = 0x30000, 0x40000, 0x50000, 0x60000
    a.T, a.H = 144, 96
    for k, val in kw.items():
        setattr(a, k, val)
    return a


def test_abi_symbols_version_and_routes_without_a_gpu():
    lib = _hip.load()
    assert lib.qs_version() == 28
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS) and all(s in _hip.SIGNATURES for s in NEW_SYMBOLS)
    v, route = lib.qs_mx_glu_bwd_quant2_v, lib.qs_mx_glu_bwd_quant2_route
    assert v(None) == ERR_ARG and route(None) == ERR_ARG
    assert v(ctypes.byref(bwd_args(struct_size=2))) == ERR_ARG
    VEC, PLAIN = _hip.MX_Q2_ROUTE_TILE_VEC, _hip.MX_Q2_ROUTE_TILE_PLAIN
    for kw, want in (({}, VEC), (dict(T=130), PLAIN), (dict(T=130, col_format=-1), VEC), (dict(dh=0x10002), PLAIN),
                     (dict(v=0x20004), PLAIN), (dict(col_codes=0x50001), PLAIN), (dict(row_codes=0x30001), VEC),
                     (dict(row_format=-1, row_codes=0, row_scales=0), VEC),
                     (dict(T=0), 0), (dict(H=0), 0),
                     (dict(H=48), ERR_ARG), (dict(H=-32), ERR_ARG), (dict(T=-1), ERR_ARG), (dict(act=3), ERR_ARG), (dict(act=-1), ERR_ARG),
                     (dict(row_format=-1, col_format=-1), ERR_ARG), (dict(row_format=5), ERR_ARG), (dict(col_format=-2), ERR_ARG),
                     (dict(dh=0), ERR_ARG), (dict(v=0), ERR_ARG), (dict(row_scales=0), ERR_ARG), (dict(col_codes=0), ERR_ARG),
                     (dict(rounding=2), ERR_ARG), (dict(index_base=2), ERR_ARG), (dict(step=4), ERR_ARG),
                     (dict(dhdt=7), ERR_DTYPE), (dict(vdt=-1), ERR_DTYPE), (dict(H=48, vdt=9), ERR_ARG),
                     (dict(dh=0x10001), ERR_ALIGN), (dict(v=0x20002), ERR_ALIGN), (dict(vdt=1, v=0x20002), PLAIN)):
        assert route(ctypes.byref(bwd_args(**kw))) == want, kw
        if want <= 0:                                   # (nothing is enqueued: safe without a GPU)
            assert v(ctypes.byref(bwd_args(**kw))) == want, kw


def pre_args(ct, **kw):
    a = ct()
    a.struct_size = ctypes.sizeof(a)
    a.a_codes, a.a_scales, a.b_codes, a.b_scales = 0x10000, 0x20000, 0x30000, 0x40000
    a.out_format, a.act, a.y, a.ydt = -1, 1, 0x50000, 0
    a.v, a.vdt = 0x70000, 1
    a.H, a.K = 32, 64
    if ct is _hip.MxGluMatmulArgs:
        a.M = 4
    else:
        a.T, a.E, a.offs = 4, 2, 0x60000
    for k, val in kw.items():
        setattr(a, k, val)
    return a


@pytest.mark.parametrize("name,ct", [("qs_mx_glu_matmul", _hip.MxGluMatmulArgs), ("qs_mx_grouped_glu_matmul", _hip.MxGroupedGluMatmulArgs)])
def test_abi_pre_entry_points_check_v_like_y(name, ct):
    lib = _hip.load()
    v, route, old = getattr(lib, name + "_pre_v"), getattr(lib, name + "_pre_route"), getattr(lib, name + "_route")
    rows = "M" if ct is _hip.MxGluMatmulArgs else "T"
    assert v(None) == ERR_ARG and route(None) == ERR_ARG
    good = route(ctypes.byref(pre_args(ct)))
    assert good > 0 and good == old(ctypes.byref(pre_args(ct)))
    for kw, want in (({rows: 0}, 0), (dict(H=0), 0), (dict(v=0), ERR_ARG), (dict(vdt=5), ERR_DTYPE), (dict(ydt=5, vdt=5), ERR_DTYPE),
                     (dict(v=0x70001), ERR_ALIGN), (dict(vdt=0, v=0x70002), ERR_ALIGN), (dict(H=48, v=0), ERR_ARG),
                     (dict(v=0x10000), ERR_ARG), (dict(v=0x30100), ERR_ARG), (dict(v=0x50000 - 8), ERR_ARG),
                     (dict(out_format=0, out_codes=0x70000 + 8, out_scales=0x80000), ERR_ARG)):
        assert route(ctypes.byref(pre_args(ct, **kw))) == want, kw
        if want <= 0:
            assert v(ctypes.byref(pre_args(ct, **kw))) == want, kw
    # the entry points without it never look at v
    assert old(ctypes.byref(pre_args(ct, v=0, vdt=99))) == good and old(ctypes.byref(pre_args(ct, v=0x10000))) == good
    short = pre_args(ct)
    short.struct_size = ct.v.offset                     # a caller compiled before the field existed
    assert old(ctypes.byref(short)) == good and route(ctypes.byref(short)) == ERR_ARG


def test_descriptor_layouts_match_the_header(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = {"qs_mx_glu_matmul_args": _hip.MxGluMatmulArgs, "qs_mx_grouped_glu_matmul_args": _hip.MxGroupedGluMatmulArgs,
             "qs_mx_glu_bwd_quant2_args": _hip.MxGluBwdQuant2Args}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(root, "include", "qsparse_hip.h")}"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append(f'printf("%zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {f}));' for f, _ in ct._fields_]
        lines.append('printf("\\n");')
    (tmp_path / "layout.c").write_text("\n".join(lines + ['return 0; }']))
    subprocess.run(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    for line, ct in zip(out, pairs.values()):
        size, *offsets = (int(t) for t in line.split())
        assert size == ctypes.sizeof(ct) and offsets == [getattr(ct, f).offset for f, _ in ct._fields_]
    assert _hip.MxGluBwdQuant2Args._fields_[0][0] == "struct_size"


# ---- dv against float64 -----------------------------------------------------------------------------------------------------------------
# unit roundoff of float32
U = 2.0 ** -24
# absolute error bounds of act'(g) and act(g) in float32 for |g| <= 8, derived below: (E_da, E_a)
ACT_ERR = {"relu": (0.0, 0.0), "silu": (102 * U, 32 * U), "gelu": (10 * U, 30 * U)}


@pytest.mark.parametrize("act", ACTS)
def test_dv_float32_against_float64(act):
    """``_glu_dv`` (the CPU path's float32 evaluation of the definition) against the same expressions in float64 on the same widened
    inputs, for g in [-8, 8].  The tolerance is derived, not tuned.  u = 2^-24 is float32's unit roundoff: every float32 operation
    returns its exact result times (1 + delta), |delta| <= u.  ``expf`` and ``erff`` are taken at their documented bounds, 1 ulp
    (relative 2 u) for expf and 2 ulp (relative 4 u) for erff, which hold for the CPU's libm / SLEEF as for the device library.

    silu.  e = expf(-g) has relative error 2 u; 1 + e adds u; so s = 1 / (1 + e) and a = g / (1 + e) carry 4 u relative: E_a = 4 u |a| <=
    32 u.  In a' = s (1 + g (1 - s)): s has absolute error 4 u (s <= 1); 1 - s cancels, absolute 4 u + u = 5 u; times g (|g| <= 8, |g (1 -
    s)| <= 8): 40 u + 8 u = 48 u; plus one: the sum is at most 9 in size, 48 u + 9 u = 57 u; times s: 57 u + 9 * 4 u + 9 u = 102 u = E_da.
    gelu.  The argument g * alpha carries u from the product and u from alpha's own rounding; erf' (x) x <= 0.43, so that moves erf by
    at most u; erff adds 4 u: 5 u absolute.  1 + erf (at most 2): 7 u.  Times g * 0.5 (exact, at most 4): 28 u, plus the product's u
    |a| <= 2 u after cancellation: E_a = 30 u.  In a' = g * pdf + cdf: cdf = 0.5 (1 + erf) carries 3.5 u; pdf = expf(-0.5 g g) * beta has
    the argument's rounding u g^2 / 2, expf's 2 u, beta's and the product's 2 u: g * pdf moves by 0.399 g e^(-g^2/2) (g^2 / 2 + 4) u <= 2 u;
    the sum (at most 1.13 in size, rounded once or twice) adds 2.3 u: 3.5 + 2 + 2.3 < 10 u = E_da.
    relu.  Both factors are exact.

    dg = (d * u_) * a': the two products add 2 u relative (a' is at most 1.13 in size: 3 u |d u_| covers them) to |d u_| E_da.
    du = d * a: one product, u |d a| <= 8 u |d|, plus |d| E_a.  No operand is small enough for a float32 underflow."""
    T, H = 64, 64
    g = (torch.rand(T, H, generator=torch.Generator().manual_seed(1)) * 16 - 8)
    g[0, :8] = torch.tensor([-8.0, 8.0, 0.0, -0.0, 1.0, -1.0, 0.5, -0.5])
    up, d = rnd(2, T, H) * 2, rnd(3, T, H)
    v = mx_glu_interleave(g, up, dim=-1)
    got = _glu_dv(d, v, act)
    assert got.dtype == torch.float32
    g64, u64, d64 = g.double(), up.double(), d.double()
    if act == "relu":
        a, da = g64.clamp_min(0), (g64 > 0).double()
    elif act == "silu":
        s = 1 / (1 + torch.exp(-g64))
        a, da = g64 * s, s * (1 + g64 * (1 - s))
    else:
        cdf = 0.5 * (1 + torch.erf(g64 * math.sqrt(0.5)))
        a, da = g64 * cdf, cdf + g64 * torch.exp(-0.5 * g64 * g64) / math.sqrt(2 * math.pi)
    want = mx_glu_interleave(d64 * u64 * da, d64 * a, dim=-1)
    e_da, e_a = ACT_ERR[act]
    tol = mx_glu_interleave((d64 * u64).abs() * (e_da + 3 * U), d64.abs() * (e_a + 8 * U), dim=-1)
    err = (got.double() - want).abs()
    print(f"{act}: max error / bound = {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= tol).all())
