"""Training through MX matrix products on the GPU: ``mx_linear`` / ``MXTrainLinear``.

The three products are the SAME GEMM kernel (qs_mx_matmul_v) on bytes that must equal what ``quantize_with_mx(...,
return_codes=True)`` writes for x, W, dy, W^T, dy^T and x^T -- so y, dx and dW are compared bit for bit with that composition; any
difference is a bug of the new path.  Against the float64 reference the bound is the one tests/test_mx_gemm_gpu.py derives, per
output element: 2 L 2^-23 S + ulp_dtype(y64) (+ 2^-23 |bias| for y), L the contraction length of the product (K, N, M).

That derivation assumes every alignment keeps 24 significant bits.  The instruction keeps fewer INSIDE a group of eight products --
they survive only down to 2^-13 of the group's larger one (probe section 4b) -- which the L-proportional bound covers once
2 L 2^-23 >= 2^-13, i.e. L >= 512; tests/test_mx_gemm_gpu.py applies it from K = 768 up.  Both shapes below therefore keep all three
contraction lengths where the bound is applied to float32 outputs at or above that, the ragged one included.  (Measured with (M, N,
K) = (100, 70, 90), float32: largest |err| / bound 0.86 for y at L = 90 and 1.14 for dx at L = 70, while y, dx and dW were bit-identical
to `mx_matmul` on the one-way quantizer's bytes -- the product kernel's own accumulation, not the new path; (256, 192, 320) gave 0.12 /
0.23 / 0.15.)  Below L = 512 the products are held to the bound that follows the instruction's measured accumulation,
``mx_gemm_ref.model_bound``, in tests/test_mx_short_k_gpu.py -- (100, 70, 90) and (45, 33, 40) of ``mx_linear`` among its cases."""
import copy

import pytest
import torch
import torch.nn as nn

import mx_gemm_ref as G
import mx_ref as R
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_gemm import MXTrainLinear, mx_linear, mx_matmul
from qsparse_amd.quantize import quantize_with_mx
from test_mx_train import _regression          # the CPU file's task and criterion, run here on the device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FX, FW, FG = "mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2"
ALIGNED, RAGGED = (512, 576, 640), (530, 522, 542)        # M, N, K: every contraction length >= 512; RAGGED: none a multiple of 4


def codes_of(t, fmt):
    with torch.no_grad():
        _, c, s = quantize_with_mx(t.contiguous(), fmt, -1, return_codes=True)
    return c, s


def case(shape, dtype, seed=0):
    M, N, K = shape
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 2).to(dtype)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    dy = (torch.randn(M, N, generator=g) / N).to(dtype)
    return x, w, b, dy


def run(x, w, b, dy, dev, fmts=(FX, FW, FG), routes=None):
    xd, wd, dyd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), dy.to(dev)
    bd = None if b is None else b.to(dev).requires_grad_(True)
    y = mx_linear(xd, wd, bd, *fmts)
    if routes is not None:
        routes.append(("fwd", _hip.mx_quant2_last_route, _hip.mx_gemm_last_route))
    y.backward(dyd)
    return y.detach(), xd.grad, wd.grad, None if bd is None else bd.grad


def references(x, w, b, dy, fmts=(FX, FW, FG)):
    """{name: (y64, S, L)} of the three products from the float64 references, written out here from the definition"""
    fx, fw, fg = fmts
    q = lambda t, f: R.reference(t, f, -1)[1:]
    xr, wr, gr = q(x, fx), q(w, fw), q(dy, fg)
    wt, gt, xt = q(w.t().contiguous(), fw), q(dy.t().contiguous(), fg), q(x.t().contiguous(), fx)
    M, K = x.shape
    N = w.shape[0]
    out = {}
    for name, a, fa, bb, fb, bias, L in (("y", xr, fx, wr, fw, b, K), ("dx", gr, fg, wt, fw, None, N), ("dw", gt, fg, xt, fx, None, M)):
        _, y64, S = G.reference(*a, fa, *bb, fb, bias)
        out[name] = (y64, S, L)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [ALIGNED, RAGGED])
def test_bit_identical_to_mx_matmul_on_the_one_way_quantizers_bytes_and_within_the_bound(dtype, shape):
    M, N, K = shape
    x, w, b, dy = case(shape, dtype)
    routes = []
    y, dx, dw, db = run(x, w, b, dy, DEV, routes=routes)
    assert y.dtype == dtype and dx.dtype == dtype and dw.dtype == torch.float32 and db.dtype == torch.float32
    # (1) the same kernel on the one-way quantizer's bytes
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    y0 = mx_matmul(*codes_of(xd, FX), FX, *codes_of(wd, FW), FW, b.to(DEV), dtype)
    dx0 = mx_matmul(*codes_of(dyd, FG), FG, *codes_of(wd.t(), FW), FW, None, dtype)
    dw0 = mx_matmul(*codes_of(dyd.t(), FG), FG, *codes_of(xd.t(), FX), FX, None, torch.float32)
    assert torch.equal(y, y0) and torch.equal(dx, dx0) and torch.equal(dw, dw0)
    assert torch.equal(db, dyd.sum(0, dtype=torch.float32))
    # (2) the float64 reference, and the package's CPU path, within the derived bound
    yc, dxc, dwc, dbc = run(x, w, b, dy, "cpu")
    for name, got, cpu, odt in (("y", y, yc, dtype), ("dx", dx, dxc, dtype), ("dw", dw, dwc, torch.float32)):
        y64, S, L = references(x, w, b, dy)[name]
        bound = 2 * L * 2.0 ** -23 * S + G.ulp(y64, odt) + (2.0 ** -23 * b.abs().double() if name == "y" else 0)
        ok, ratio = G.within(got, y64, bound)
        okc, ratioc = G.within(cpu, y64, bound)
        print(name, shape, dtype, "largest |err| / bound: gpu", ratio, "cpu", ratioc)
        assert ok and okc, (name, ratio, ratioc)
        assert bool(((got.cpu().double() - cpu.double()).abs() <= 2 * bound).all())
    # (3) routes: the forward's last two-way call is the weight's (row pair only), the GEMM the forward product
    vec = shape == ALIGNED
    q2 = _hip.MX_Q2_ROUTE_TILE_VEC if vec else _hip.MX_Q2_ROUTE_TILE_PLAIN
    gemm = _hip.MX_GEMM_ROUTE_VEC if vec else _hip.MX_GEMM_ROUTE_PLAIN
    assert routes == [("fwd", q2, gemm)]


def test_routes_of_every_launch_of_a_step():
    """the event log names every launch of this library with its route: 2 + 2 two-way calls and 3 GEMMs, nothing else"""
    for shape, q2, gemm in ((ALIGNED, _hip.MX_Q2_ROUTE_TILE_VEC, _hip.MX_GEMM_ROUTE_VEC), (RAGGED, _hip.MX_Q2_ROUTE_TILE_PLAIN, _hip.MX_GEMM_ROUTE_PLAIN)):
        x, w, b, dy = case(shape, torch.bfloat16)
        xd, wd, bd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        _hip.start_event_log()
        y = mx_linear(xd, wd, bd)
        fwd = _hip.stop_event_log()
        assert {k: len(v) for k, v in fwd.items()} == {f"mx_quant2[{q2}]": 2, f"mx_matmul[{gemm}]": 1}
        _hip.start_event_log()
        y.backward(dy.to(DEV))
        bwd = _hip.stop_event_log()
        assert {k: len(v) for k, v in bwd.items()} == {f"mx_quant2[{q2}]": 2, f"mx_matmul[{gemm}]": 2}
        # a first layer: no input gradient -> no dgrad GEMM, no weight transposition, one two-way call (col pair of dy only)
        wd.grad = None
        y = mx_linear(x.to(DEV), wd, bd)
        _hip.start_event_log()
        y.backward(dy.to(DEV))
        bwd = _hip.stop_event_log()
        assert {k: len(v) for k, v in bwd.items()} == {f"mx_quant2[{q2}]": 1, f"mx_matmul[{gemm}]": 1}
        # grad disabled: the forward's call on x writes the row pair only -- as many bytes as the weight-free call below, and nothing
        # is kept of x; the bytes the event log accounts per launch tell the two apart
        for mode in (torch.no_grad, torch.inference_mode):
            with mode():
                _hip.start_event_log()
                y2 = mx_linear(xd, wd, bd)
                nograd = _hip.stop_event_log(with_bytes=True)
            assert torch.equal(y2, y) and not y2.requires_grad
            assert {k: len(v) for k, v in nograd.items()} == {f"mx_quant2[{q2}]": 2, f"mx_matmul[{gemm}]": 1}
            M, N, K = shape
            moved = sorted(int(b_) for _, b_ in nograd[f"mx_quant2[{q2}]"])
            nb = lambda n: -(-n // 32)
            assert moved == sorted([M * K * 2 + M * K + M * nb(K), N * K * 4 + N * K + N * nb(K)]), moved


def test_mixed_dtypes_leading_dims_and_formats():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 96, generator=g).bfloat16().to(DEV).requires_grad_(True)
    layer = MXTrainLinear(96, 48, x_fmt="mxfp6_e2m3", w_fmt="mxfp4_e2m1", grad_fmt="mxfp8_e4m3").to(DEV)
    y = layer(x)
    assert y.shape == (2, 5, 48) and y.dtype == torch.bfloat16
    dy = torch.randn(2, 5, 48, generator=g).bfloat16().to(DEV)
    y.backward(dy)
    assert x.grad.dtype == torch.bfloat16 and x.grad.shape == x.shape and layer.weight.grad.dtype == torch.float32
    # the same product kernel on the one-way quantizer's bytes: bit for bit, at any contraction length
    fx, fw, fg = "mxfp6_e2m3", "mxfp4_e2m1", "mxfp8_e4m3"
    x2, w, dy2 = x.detach().reshape(10, 96), layer.weight.detach(), dy.reshape(10, 48)
    assert torch.equal(y.detach().reshape(10, 48), mx_matmul(*codes_of(x2, fx), fx, *codes_of(w, fw), fw, layer.bias.detach(), torch.bfloat16))
    assert torch.equal(x.grad.reshape(10, 96), mx_matmul(*codes_of(dy2, fg), fg, *codes_of(w.t(), fw), fw, None, torch.bfloat16))
    assert torch.equal(layer.weight.grad, mx_matmul(*codes_of(dy2.t(), fg), fg, *codes_of(x2.t(), fx), fx, None, torch.float32))
    assert torch.equal(layer.bias.grad, dy2.sum(0, dtype=torch.float32))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert layer(torch.randn(4, 96, device=DEV)).dtype == torch.bfloat16
    inf = layer.to_inference()
    with torch.no_grad():
        assert inf(x.detach()).shape == y.shape
    rc, rs, _, _ = qs.mx_quantize_2way(layer.weight, "mxfp4_e2m1")
    assert torch.equal(inf.weight_codes, rc) and torch.equal(inf.weight_scales, rs)


def test_captured_step_replays_bit_for_bit():
    """forward, backward and an SGD update of one MXTrainLinear under torch.cuda.graph: a single layer, no parallel branches"""
    g = torch.Generator().manual_seed(11)
    M, K, N, lr = 256, 192, 128, 0.05
    xs = [torch.randn(M, K, generator=g).bfloat16().to(DEV) for _ in range(3)]
    ts = [torch.randn(M, N, generator=g).bfloat16().to(DEV) for _ in range(3)]
    torch.manual_seed(0)
    init = MXTrainLinear(K, N).to(DEV)

    def step(layer, x, t):
        y = layer(x)
        gy = ((y - t) / y.numel()).detach()                 # the gradient of a mean-squared error, formed outside autograd
        for p in layer.parameters():
            p.grad = None
        y.backward(gy)
        with torch.no_grad():
            for p in layer.parameters():
                p.add_(p.grad, alpha=-lr)
        return y.detach()

    eager = copy.deepcopy(init)
    want = []
    for x, t in zip(xs, ts):
        y = step(eager, x, t).clone()
        want.append((y, eager.weight.detach().clone(), eager.bias.detach().clone()))

    layer = copy.deepcopy(init)
    static_x, static_t = xs[0].clone(), ts[0].clone()
    keep = copy.deepcopy(layer.state_dict())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(layer, static_x, static_t)
    torch.cuda.current_stream().wait_stream(side)
    layer.load_state_dict(keep)                             # undo the warm-up's update
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = step(layer, static_x, static_t)
    layer.load_state_dict(keep)                             # (capture enqueues nothing, but keep the start explicit)
    for (x, t), (y, w, b) in zip(zip(xs, ts), want):
        static_x.copy_(x)
        static_t.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_y, y) and torch.equal(layer.weight.detach(), w) and torch.equal(layer.bias.detach(), b)


def test_training_sanity_against_the_float32_net():
    out = _regression(DEV)
    (i32, f32), (imx, fmx) = out["float32"], out["mx"]
    print("float32 net: initial", i32, "final", f32, "| MX net: initial", imx, "final", fmx)
    assert f32 * 10 <= i32, "the yardstick itself must learn: the float32 net lowers its loss at least 10-fold"
    assert fmx <= (i32 * f32) ** 0.5, "the MX net's final loss is at most the geometric mean of the initial and the float32 final loss"
