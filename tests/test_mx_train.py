"""Training through MX matrix products, CPU side: the two-way quantizer's entry point (declaration, binding, validation: no GPU
needed), ``mx_quantize_2way`` against tests/mx_ref.py, ``mx_linear`` against a composition of the two float64 references written
here, ``MXTrainLinear``, and a training run measured against the same network in float32.

The bound on the three products, per output element, is the one tests/test_mx_gemm_gpu.py derives for float32 accumulation: 2 L 2^-23
S + ulp_dtype(y64) (+ 2^-23 |bias| for y), L the contraction length (K, N, M for y, dx, dW), S = sum |a b|.  The CPU path rounds a
float64 sum once, far inside it."""
import copy
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn as nn

import mx_gemm_ref as G
import mx_ref as R
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_gemm import MXLinear, MXTrainLinear, mx_linear, mx_quantize_2way

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = list(R.FORMATS)
VEC, PLAIN = _hip.MX_Q2_ROUTE_TILE_VEC, _hip.MX_Q2_ROUTE_TILE_PLAIN


def test_entry_point_is_declared_bound_and_validates_without_a_gpu(tmp_path):
    lib = _hip.load()
    assert lib.qs_version() == _hip.ABI_VERSION == 28                          # the version this binding needs
    assert "qs_mx_quant2_v" in _hip.SIGNATURES and "qs_mx_quant2_route" in _hip.SIGNATURES
    assert lib.qs_mx_quant2_v(None) == -2 and lib.qs_mx_quant2_route(None) == -2
    short = _hip.MxQuant2Args()
    short.struct_size = 2
    assert lib.qs_mx_quant2_v(ctypes.byref(short)) == -2                       # a descriptor too short to carry its own size
    a = _hip.MxQuant2Args()
    a.struct_size = ctypes.sizeof(a)
    call = lambda: (lib.qs_mx_quant2_v(ctypes.byref(a)), lib.qs_mx_quant2_route(ctypes.byref(a)))
    a.x, a.R, a.C = 4096, 64, 64
    assert call() == (-2, -2)                                                  # both pairs null
    a.row_codes = 8192
    assert call() == (-2, -2)                                                  # codes without scales
    a.row_codes, a.row_scales = None, 8192
    assert call() == (-2, -2)                                                  # scales without codes
    a.row_codes, a.col_scales = 16384, 32768
    assert call() == (-2, -2)                                                  # half a col pair next to a whole row pair
    a.col_codes = 65536
    a.row_format = 5
    assert call() == (-2, -2)                                                  # unknown format
    a.row_format, a.col_format = 4, -1
    assert call() == (-2, -2)
    a.col_format, a.xdt = 1, 7
    assert call() == (-1, -1)                                                  # unknown dtype
    a.xdt, a.x = 0, 4098
    assert call() == (-3, -3)                                                  # x not aligned to a float32
    a.xdt = 1
    assert lib.qs_mx_quant2_route(ctypes.byref(a)) == PLAIN                    # ... but to a bf16: a route, the element-access one
    a.x, a.R = 4096, -1
    assert call() == (-2, -2)
    a.R, a.x = 64, None
    assert call() == (-2, -2)
    a.x = 4096
    for R_, C in ((0, 64), (64, 0), (0, 0)):
        a.R, a.C = R_, C
        assert call() == (0, 0)                                                # empty: accepted, nothing enqueued
    # the route the launch would take, decided by the launching code itself
    route = lambda: lib.qs_mx_quant2_route(ctypes.byref(a))
    a.R, a.C, a.xdt = 64, 64, 1
    assert route() == VEC
    a.C = 68
    assert route() == PLAIN                                                    # two-byte x: C % 8
    a.xdt = 0
    assert route() == VEC                                                      # float32: C % 4
    a.C = 66
    assert route() == PLAIN
    a.C, a.xdt, a.R = 64, 2, 72
    assert route() == PLAIN                                                    # col pair written: R % 16
    a.col_codes = a.col_scales = None
    assert route() == VEC                                                      # ... row pair only: any R
    a.col_codes, a.col_scales, a.R = 65536, 32768, 80
    assert route() == VEC
    a.col_codes = 65540
    assert route() == PLAIN                                                    # col_codes base
    a.col_codes, a.x = 65536, 4098
    assert route() == PLAIN                                                    # x one element past a 16-byte boundary
    a.x, a.row_codes, a.row_scales, a.col_scales = 4096, 16385, 8193, 32769
    assert route() == VEC                                                      # row codes and scale bytes: any address
    a.row_codes = a.row_scales = None
    a.row_format = 99
    assert route() == VEC                                                      # the format of a pair that is not given is ignored
    # the ctypes mirror against the header's own layout
    fields = [f for f, _ in _hip.MxQuant2Args._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu", sizeof(qs_mx_quant2_args));\n%s\nreturn 0; }\n'
                   % (os.path.join(ROOT, "include", "qsparse_hip.h"), "\n".join(f'printf(" %zu", offsetof(qs_mx_quant2_args, {f}));' for f in fields)))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(src)], check=True)
    size, *offs = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(_hip.MxQuant2Args) and [int(o) for o in offs] == [getattr(_hip.MxQuant2Args, f).offset for f in fields]
    assert fields == ["struct_size", "row_format", "col_format", "x", "xdt", "row_codes", "row_scales", "col_codes", "col_scales", "R", "C", "stream",
                      "rounding", "reserved0", "seed", "step", "index_base"]


def randn(shape, dtype, seed=0, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.exp(torch.randn(shape[0], 1, generator=g) * spread)).to(dtype)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_two_way_on_cpu_equals_the_reference_both_ways(fmt, dtype):
    other = FMTS[(FMTS.index(fmt) + 2) % 5]
    for i, shape in enumerate(((1, 1), (33, 31), (64, 96), (5, 200), (70, 40))):
        x = randn(shape, dtype, seed=i)
        if shape == (64, 96):
            x[3, 40], x[50, 7] = float("nan"), float("inf")                   # a NaN and an Inf block in each direction
        rc, rs, cc, cs = mx_quantize_2way(x, fmt, other)
        _, c, s = R.reference(x, fmt, -1)
        assert R.same(rc, c) and R.same(rs, s), (shape, "row")
        _, c, s = R.reference(x.t().contiguous(), other, -1)
        assert R.same(cc, c) and R.same(cs, s), (shape, "col")
        if shape == (64, 96):
            assert rs[3, 1] == 255 and rs[50, 0] == 255 and int((rs == 255).sum()) == 2 and not rc[3, 32:64].any()
            assert cs[40, 0] == 255 and cs[7, 1] == 255 and int((cs == 255).sum()) == 2 and not cc[7, 32:64].any()
        assert rc.dtype == cc.dtype == torch.uint8 and not rc.requires_grad
    x = randn((40, 50), dtype).requires_grad_(True)
    rc, rs, cc, cs = mx_quantize_2way(x, fmt)                                  # row pair only; outputs never differentiable
    assert cc is None and cs is None and not rc.requires_grad and R.same(rc, R.reference(x, fmt)[1])
    rc, rs, cc, cs = mx_quantize_2way(x, None, fmt)
    assert rc is None and rs is None and R.same(cs, R.reference(x.detach().t().contiguous(), fmt)[2])
    assert R.same(mx_quantize_2way(x.t(), fmt)[0], R.reference(x.detach().t().contiguous(), fmt)[1])       # a non-contiguous input
    with pytest.raises(ValueError, match="row_fmt, col_fmt or both"):
        mx_quantize_2way(x)
    with pytest.raises(ValueError, match="2-d"):
        mx_quantize_2way(torch.zeros(2, 3, 4), fmt)
    with pytest.raises(ValueError, match="unknown MX format"):
        mx_quantize_2way(x, "mxfp5")
    with pytest.raises(TypeError, match="must be one of"):
        mx_quantize_2way(x.double(), fmt)
    assert qs.mx_quantize_2way is mx_quantize_2way and qs.mx_linear is mx_linear and qs.MXTrainLinear is MXTrainLinear


def composition(x2, w, b, dy2, fmts):
    """{name: (y64, S, L)}: the three products composed here from the quantizer's and the product's float64 references"""
    fx, fw, fg = fmts
    q = lambda t, f: R.reference(t, f, -1)[1:]
    M, K = x2.shape
    N = w.shape[0]
    ops = {"y": (q(x2, fx), fx, q(w, fw), fw, b, K), "dx": (q(dy2, fg), fg, q(w.t().contiguous(), fw), fw, None, N),
           "dw": (q(dy2.t().contiguous(), fg), fg, q(x2.t().contiguous(), fx), fx, None, M)}
    out = {}
    for name, (a, fa, bb, fb, bias, L) in ops.items():
        _, y64, S = G.reference(*a, fa, *bb, fb, bias)
        out[name] = (y64, S, L)
    return out


def check_linear(x, w, b, dy, fmts, x_grad=True, w_grad=True):
    K, N = x.shape[-1], w.shape[0]
    xg, wg = x.clone().requires_grad_(x_grad), w.clone().requires_grad_(w_grad)
    bg = None if b is None else b.clone().requires_grad_(True)
    y = mx_linear(xg, wg, bg, *fmts)
    assert y.shape == x.shape[:-1] + (N,) and y.dtype == x.dtype
    if not (x_grad or w_grad or b is not None):
        assert not y.requires_grad
        return
    y.backward(dy)
    ref = composition(x.reshape(-1, K), w, b, dy.reshape(-1, N), fmts)
    got = {"y": (y.detach().reshape(-1, N), x.dtype)}
    if x_grad:
        assert xg.grad.shape == x.shape and xg.grad.dtype == x.dtype
        got["dx"] = (xg.grad.reshape(-1, K), x.dtype)
    else:
        assert xg.grad is None
    if w_grad:
        assert wg.grad.shape == w.shape and wg.grad.dtype == w.dtype
        got["dw"] = (wg.grad, w.dtype)
    else:
        assert wg.grad is None
    for name, (t, odt) in got.items():
        y64, S, L = ref[name]
        bound = 2 * L * 2.0 ** -23 * S + G.ulp(y64, odt) + (2.0 ** -23 * b.abs().double() if name == "y" and b is not None else 0)
        ok, ratio = G.within(t, y64, bound)
        print(name, tuple(x.shape), x.dtype, w.dtype, fmts, "largest |err| / bound", ratio)
        assert ok, (name, ratio)
        assert G.same(t, y64.to(odt)), name                                     # the CPU path: float64, one rounding
    if b is not None:
        db64 = dy.reshape(-1, N).double().sum(0)
        assert bg.grad.dtype == b.dtype
        assert bool(((bg.grad.double() - db64).abs() <= dy.shape[:-1].numel() * 2.0 ** -23 * dy.reshape(-1, N).double().abs().sum(0) + G.ulp(db64, b.dtype)).all())


@pytest.mark.parametrize("fmts", [("mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp4_e2m1", "mxfp6_e2m3", "mxfp6_e3m2"), ("mxfp6_e3m2", "mxfp4_e2m1", "mxfp8_e4m3")])
def test_mx_linear_on_cpu_against_the_composed_references(fmts):
    g = torch.Generator().manual_seed(7)
    K, N = 70, 40
    w, b = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    x3, dy3 = torch.randn(2, 5, K, generator=g) * 2, torch.randn(2, 5, N, generator=g) / N
    check_linear(x3, w, b, dy3, fmts)                                           # leading dimensions [2, 5, K]
    check_linear(x3, w, None, dy3, fmts)                                        # no bias
    check_linear(x3, w, b, dy3, fmts, w_grad=False)                             # a weight that needs no grad
    check_linear(x3, w, b, dy3, fmts, x_grad=False)                             # an x that needs no grad
    check_linear(x3, w, None, dy3, fmts, x_grad=False, w_grad=False)            # nothing needs grad
    x2, dy2 = torch.randn(37, K, generator=g), torch.randn(37, N, generator=g)
    check_linear(x2.bfloat16(), w, b, dy2.bfloat16(), fmts)                     # bf16 x, float32 parameters: bf16 dx, float32 dW, db
    check_linear(x2.half(), w.half(), b.half(), dy2.half(), fmts)
    check_linear(x2[0], w, b, dy2[0], fmts)                                     # x [K]


def test_mx_linear_refusals_and_saved_tensors():
    x, w = torch.randn(4, 64), torch.randn(8, 64, requires_grad=True)
    with pytest.raises(ValueError, match="unknown MX format"):
        mx_linear(x, w, grad_fmt="e5m2")
    with pytest.raises(ValueError, match="disagree on K"):
        mx_linear(torch.randn(4, 32), w)
    with pytest.raises(ValueError, match=r"\[N, K\]"):
        mx_linear(x, w[0])
    with pytest.raises(ValueError, match="bias has shape"):
        mx_linear(x, w, torch.zeros(4))
    with pytest.raises(TypeError, match="must be one of"):
        mx_linear(x.double(), w)
    # the backward keeps x as transposed codes (1 + 1/32 bytes per element), the weight as the tensor itself
    y = mx_linear(x.requires_grad_(True), w)
    saved = y.grad_fn.saved_tensors
    assert saved[0] is w or saved[0].data_ptr() == w.data_ptr()
    assert [tuple(t.shape) for t in saved[1:]] == [(64, 4), (64, 1)] and all(t.dtype == torch.uint8 for t in saved[1:])
    # a weight modified in place between forward and backward: autograd's own version error
    with torch.no_grad():
        w.mul_(2)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()


def test_col_pair_of_x_only_where_a_weight_gradient_can_be_asked_for(monkeypatch):
    """the forward's call on x asks for the transposed codes only with grad enabled and a weight that requires grad"""
    import qsparse_amd.mx_gemm as M
    calls = []
    real = M.mx_quantize_2way
    monkeypatch.setattr(M, "mx_quantize_2way", lambda x, row_fmt=None, col_fmt=None, *sr: calls.append((tuple(x.shape), row_fmt, col_fmt)) or real(x, row_fmt, col_fmt, *sr))
    layer, x = MXTrainLinear(64, 32), torch.randn(6, 64)
    X, W, F = (6, 64), (32, 64), "mxfp8_e4m3"

    def forward_calls(fn):
        calls.clear()
        y = fn()
        return y, list(calls)

    y, got = forward_calls(lambda: layer(x))
    assert got == [(X, F, F), (W, F, None)] and y.requires_grad
    for mode in (torch.no_grad, torch.inference_mode):
        with mode():
            y0, got = forward_calls(lambda: layer(x))
        assert got == [(X, F, None), (W, F, None)] and not y0.requires_grad and torch.equal(y0, y.detach())
        with mode():
            _, got = forward_calls(lambda: layer(x.clone().requires_grad_(True)) if mode is torch.no_grad else layer(x))
        assert got == [(X, F, None), (W, F, None)]
    layer.weight.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    y1, got = forward_calls(lambda: layer(xg))                                   # a frozen weight: x still gets its gradient
    assert got == [(X, F, None), (W, F, None)] and y1.requires_grad
    calls.clear()
    y1.sum().backward()
    assert calls == [((6, 32), "mxfp8_e5m2", None), (W, None, F)] and xg.grad is not None and layer.weight.grad is None
    # the backward is once-differentiable: a double backward is refused instead of differentiating through nothing
    layer.weight.requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    gy = torch.randn(6, 32, requires_grad=True)
    gx, = torch.autograd.grad(layer(xg), xg, grad_outputs=gy, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


def test_mxtrainlinear_is_a_drop_in_linear():
    torch.manual_seed(0)
    lin = nn.Linear(70, 12)
    layer = MXTrainLinear.from_linear(lin, w_fmt="mxfp6_e2m3")
    assert isinstance(layer, nn.Linear) and list(layer.state_dict()) == list(lin.state_dict()) == ["weight", "bias"]
    assert layer.weight is lin.weight and layer.bias is lin.bias and layer.weight.data_ptr() == lin.weight.data_ptr()
    assert (layer.x_fmt, layer.w_fmt, layer.grad_fmt) == ("mxfp8_e4m3", "mxfp6_e2m3", "mxfp8_e5m2") and "w_fmt='mxfp6_e2m3'" in repr(layer)
    own = MXTrainLinear(70, 12, bias=False, x_fmt="mxfp4_e2m1")
    assert own.bias is None and list(own.state_dict()) == ["weight"] and own.weight.shape == (12, 70) and own.weight.requires_grad
    own.load_state_dict({"weight": lin.weight.detach().clone()})
    with pytest.raises(ValueError, match="unknown MX format"):
        MXTrainLinear(4, 4, grad_fmt="fp8")
    with pytest.raises(TypeError, match="nn.Linear"):
        MXTrainLinear.from_linear(nn.Conv2d(3, 3, 1))
    x = torch.randn(3, 5, 70)
    assert torch.equal(layer(x), mx_linear(x, lin.weight, lin.bias, w_fmt="mxfp6_e2m3"))
    # under autocast: the input is cast to the autocast dtype, the output has it; the parameters stay float32
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y = layer(x)
    assert y.dtype == torch.bfloat16 and torch.equal(y, mx_linear(x.bfloat16(), lin.weight, lin.bias, w_fmt="mxfp6_e2m3"))
    y.float().sum().backward()
    assert lin.weight.grad.dtype == torch.float32 and lin.weight.grad.shape == (12, 70) and lin.bias.grad.shape == (12,)
    # to_inference: the MXLinear on the current weight; its bytes are the row pair the training forward multiplies with
    inf = layer.to_inference()
    rc, rs, _, _ = mx_quantize_2way(lin.weight, "mxfp6_e2m3")
    assert isinstance(inf, MXLinear) and torch.equal(inf.weight_codes, rc) and torch.equal(inf.weight_scales, rs)
    assert inf.weight_fmt == "mxfp6_e2m3" and inf.act_fmt == "mxfp8_e4m3" and torch.equal(inf.bias, lin.bias.detach())
    _, c, s = R.reference(lin.weight, "mxfp6_e2m3", -1)
    assert torch.equal(inf.weight_codes, c) and torch.equal(inf.weight_scales, s)
    with torch.no_grad():
        assert torch.equal(inf(x), layer(x))                                   # float32 in, float32 out: the same product on the same bytes
    assert layer.to_inference("mxfp4_e2m1").act_fmt == "mxfp4_e2m1"
    # MXLinear itself is untouched: an inference layer
    with pytest.raises(RuntimeError, match="requires grad"):
        inf(x.clone().requires_grad_(True))


def _regression(dev, steps=300):
    """a two-layer MLP on a fixed synthetic regression, from the same init with the same optimizer: (initial loss, final loss)"""
    g = torch.Generator().manual_seed(0)
    X = torch.randn(256, 64, generator=g)
    teacher = nn.Sequential(nn.Linear(64, 96), nn.Tanh(), nn.Linear(96, 32))
    with torch.no_grad():
        for p in teacher.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        Y = teacher(X)
    X, Y = X.to(dev), Y.to(dev)
    torch.manual_seed(1)
    ref = nn.Sequential(nn.Linear(64, 96), nn.Tanh(), nn.Linear(96, 32))
    out = {}
    for name in ("float32", "mx"):
        net = copy.deepcopy(ref)
        if name == "mx":
            net[0], net[2] = MXTrainLinear.from_linear(net[0]), MXTrainLinear.from_linear(net[2])
        net = net.to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=3e-3)
        losses = []
        for _ in range(steps):
            opt.zero_grad()
            loss = nn.functional.mse_loss(net(X), Y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        with torch.no_grad():
            losses.append(float(nn.functional.mse_loss(net(X), Y)))
        out[name] = (losses[0], losses[-1])
    return out


def test_training_sanity_against_the_float32_net():
    out = _regression("cpu")
    (i32, f32), (imx, fmx) = out["float32"], out["mx"]
    print("float32 net: initial", i32, "final", f32, "| MX net: initial", imx, "final", fmx)
    assert f32 * 10 <= i32, "the yardstick itself must learn: the float32 net lowers its loss at least 10-fold"
    assert fmx <= (i32 * f32) ** 0.5, "the MX net's final loss is at most the geometric mean of the initial and the float32 final loss"
