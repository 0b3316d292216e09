"""MX block-scaled quantizers on the GPU: the HIP kernels (qs_mx_quant_fwd_v) against the float64 CPU reference of tests/mx_ref.py,
bit for bit -- values, code bytes and scale bytes -- on every route the entry point has, asserted by route."""
import copy

import pytest
import torch
import torch.nn as nn

import mx_ref as R
import qsparse_amd as qs
from qsparse_amd import _hip, graphs
from qsparse_amd.quantize import MXQuantizer, quantize_with_mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMTS = list(R.FORMATS)
VEC, PLAIN, STRIDED = _hip.MX_ROUTE_INNER_VEC, _hip.MX_ROUTE_INNER_PLAIN, _hip.MX_ROUTE_STRIDED


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def check(x_cpu, fmt, dim=-1, route=None, what="", x_dev=None):
    """GPU (y, codes, scales) == CPU reference; `route`: the kernel the launch must have taken"""
    ry, rc, rs = R.reference(x_cpu, fmt, dim)
    xd = x_cpu.to(DEV) if x_dev is None else x_dev
    y, c, s = quantize_with_mx(xd, fmt, dim, return_codes=True)
    if route is not None:
        assert _hip.mx_last_route == route, (what, _hip.mx_last_route, route)
    assert y.is_cuda and c.is_cuda and s.is_cuda and y.stride() == xd.stride()
    assert R.same(y, ry), (fmt, dim, what, "y")
    assert R.same(c, rc), (fmt, dim, what, "codes")
    assert R.same(s, rs), (fmt, dim, what, "scales")
    y2 = quantize_with_mx(xd, fmt, dim)
    if route is not None:
        assert _hip.mx_last_route == route
    assert R.same(y2, ry), (fmt, dim, what, "y without codes")
    return y, c, s


def randn(shape, dtype, seed=0, spread=4.0):
    g = torch.Generator().manual_seed(seed)
    lead = (shape[0],) + (1,) * (len(shape) - 1)
    return (torch.randn(shape, generator=g) * torch.exp(torch.randn(lead, generator=g) * spread)).to(dtype)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_every_route_equals_reference(fmt, dtype):
    check(randn((8, 197, 3072), dtype), fmt, -1, VEC, "token-major")
    x = randn((16, 256, 14, 14), dtype, seed=1)
    check(x, fmt, 1, STRIDED, "NCHW along C")
    cl = x.contiguous(memory_format=torch.channels_last)
    y, _, s = check(cl, fmt, 1, VEC, "channels_last along C")
    assert y.is_contiguous(memory_format=torch.channels_last) and s.shape == (16, 8, 14, 14)
    check(randn((64, 3, 7, 7), dtype, seed=2), fmt, 1, STRIDED, "conv stem weight")
    check(randn((512, 512, 3, 3), dtype, seed=3), fmt, 1, STRIDED, "conv weight")
    check(randn((8, 64, 5), dtype, seed=4), fmt, 0, STRIDED, "leading dim")
    flat = randn((64 * 64 + 1,), dtype, seed=5)
    fd = flat.to(DEV)
    view = fd[1:].view(64, 64)                                              # storage offset of one element: not 16-byte aligned
    assert view.data_ptr() % 16 != 0
    check(flat[1:].view(64, 64), fmt, -1, PLAIN, "unaligned view", x_dev=view)
    for n in (31, 33, 56, 100):
        check(randn((37, n), dtype, seed=n), fmt, -1, PLAIN, f"line length {n}")
        check(randn((3, n, 6), dtype, seed=n), fmt, 1, STRIDED, f"strided length {n}")
    t = randn((6, 96, 10), dtype, seed=7).transpose(1, 2)                   # neither contiguous nor channels_last: one copy
    check(t, fmt, 2, None, "transposed", x_dev=randn((6, 96, 10), dtype, seed=7).to(DEV).transpose(1, 2))


@pytest.mark.parametrize("fmt", FMTS)
def test_large_two_d(fmt):
    check(randn((4096, 4096), torch.bfloat16, seed=11, spread=6.0), fmt, -1, VEC, "2-d")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_exhaustive_two_byte_patterns(fmt, dtype):
    for x in (R.all_patterns(dtype), R.permuted_finite_patterns(dtype)):
        check(x.reshape(-1, 32), fmt, -1, VEC, "exhaustive, aligned")
        check(x.reshape(-1, 32).t().contiguous(), fmt, 0, STRIDED, "exhaustive, strided")
        xd = torch.cat([x[:1], x]).to(DEV)[1:].view(-1, 32)
        check(x.reshape(-1, 32), fmt, -1, PLAIN, "exhaustive, unaligned", x_dev=xd)


@pytest.mark.parametrize("fmt", FMTS)
def test_ties_clamp_zeros_nonfinite_and_exponent_clamps(fmt):
    eb, mb, bias, emax, top = R.FORMATS[fmt]
    m = R.midpoints(fmt)
    for k in (-126, -60, -3, 0, 7, 100, 118):
        blk = torch.zeros(len(m), 32)
        blk[:, 0], blk[:, 1], blk[:, 2] = top, m, -m
        check(blk * 2.0 ** k, fmt, -1, VEC, f"ties at 2^{k}")
        check((blk * 2.0 ** k)[:, :31].contiguous(), fmt, -1, PLAIN, f"ties at 2^{k}")
        check((blk * 2.0 ** k).t().contiguous(), fmt, 0, STRIDED, f"ties at 2^{k}")
    tops = torch.linspace(1.0, 2.0, 32)[:-1].repeat(4, 1) * 2.0 ** emax * torch.tensor([[1.0], [-1.0], [2.0 ** -20], [2.0 ** 30]])
    tops = torch.cat([tops, torch.full((4, 1), 1.9 * 2.0 ** emax)], 1)
    check(tops, fmt, -1, VEC, "clamp")
    z = torch.zeros(2, 64)
    z[0, ::2] = -0.0
    z[1, 40:] = -0.0
    y, c, s = check(z, fmt, -1, VEC, "zeros")
    assert torch.equal(torch.signbit(y.cpu()), torch.signbit(z))
    for bad in (float("nan"), float("inf"), -float("inf")):
        x = randn((3, 96), torch.float32)
        x[1, 40] = bad
        for route, xx, dim in ((VEC, x, -1), (PLAIN, x[:, :95].contiguous(), -1), (STRIDED, x.t().contiguous(), 0)):
            check(xx, fmt, dim, route, f"one {bad}")
    sub = torch.arange(1, 65).float().reshape(2, 32) * 2.0 ** -149
    subs = torch.cat([sub, -sub * 2 ** 10, sub * 2 ** 24])
    big = torch.cat([torch.full((1, 32), 3.0e38), -torch.arange(1, 33).float().reshape(1, 32) * 1.0e37, randn((1, 32), torch.float32) * 2.0 ** 126])
    for x in (subs, big):
        check(x, fmt, -1, VEC, "exponent clamps")
        check(x.t().contiguous(), fmt, 0, STRIDED, "exponent clamps")
        check(torch.cat([x, x[:, :1]], 1), fmt, -1, PLAIN, "exponent clamps")


def test_preserve_dtype_and_float64():
    x = randn((16, 256), torch.bfloat16)
    qs.set_qsparse_options(preserve_dtype=True)
    try:
        for fmt in FMTS:
            for xx, dim, route in ((x, -1, VEC), (x[:, :100].contiguous(), -1, PLAIN), (x, 0, STRIDED)):
                y = quantize_with_mx(xx.to(DEV), fmt, dim)
                assert _hip.mx_last_route == route and y.dtype == torch.bfloat16
                assert R.same(y, R.reference(xx, fmt, dim, torch.bfloat16)[0])
            h = (x.float() * 1e3).to(torch.float16)
            assert R.same(quantize_with_mx(h.to(DEV), fmt), R.reference(h, fmt, -1, torch.float16)[0])
    finally:
        qs.set_qsparse_options(preserve_dtype=False)
    d = randn((8, 100), torch.float64)                                     # float64 on the device: the package's ATen expression
    y, c, s = quantize_with_mx(d.to(DEV), "mxfp6_e3m2", -1, return_codes=True)
    ry, rc, rs = R.reference(d, "mxfp6_e3m2")
    assert y.is_cuda and R.same(y, ry) and R.same(c, rc) and R.same(s, rs)


def test_full_size_token_major_case():
    """256 x 197 x 3072 bf16 against the CPU reference, in slices of the leading dim (the reference works in float64)"""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(256, 197, 3072, generator=g, dtype=torch.float32) * torch.exp(torch.randn(256, 197, 1, generator=g) * 3)).bfloat16()
    y, c, s = quantize_with_mx(x.to(DEV), "mxfp8_e4m3", -1, return_codes=True)
    assert _hip.mx_last_route == VEC
    y, c, s = y.cpu(), c.cpu(), s.cpu()
    for i in range(0, 256, 16):
        ry, rc, rs = R.ref_grid(x[i:i + 16], "mxfp8_e4m3")
        assert R.same(y[i:i + 16], ry) and R.same(c[i:i + 16], rc) and R.same(s[i:i + 16], rs), i


def test_backward_passes_the_gradient_through_without_a_launch():
    x = randn((8, 64, 6, 6), torch.bfloat16).to(DEV).requires_grad_(True)
    g = torch.randn(8, 64, 6, 6, device=DEV)
    _hip.start_event_log()
    y = quantize_with_mx(x, "mxfp4_e2m1", 1)
    fwd = _hip.stop_event_log()
    assert list(fwd) == [f"mx_quant_fwd[{STRIDED}]"]
    _hip.start_event_log()
    y.backward(g)
    assert _hip.stop_event_log() == {}                                     # no kernel of this library
    assert x.grad.dtype == torch.bfloat16 and torch.equal(x.grad, g.bfloat16())


def test_layers_on_the_device_equal_the_reference():
    torch.manual_seed(0)
    for layer, x in ((nn.Linear(70, 12), torch.randn(5, 70)), (nn.Conv2d(40, 6, 3), torch.randn(2, 40, 8, 8))):
        ql = qs.quantize(copy.deepcopy(layer), bits=4, bias_bits=4, timeout=1, callback=MXQuantizer("mxfp4_e2m1", block_dim=1)).to(DEV).train()
        ql(x.to(DEV)), ql(x.to(DEV))
        assert R.same(ql.weight.detach(), R.reference(layer.weight, "mxfp4_e2m1", 1)[0])
        assert R.same(ql.bias.detach(), R.reference(layer.bias, "mxfp4_e2m1", -1)[0])
        ex = qs.export_integer(nn.Sequential(ql))["0"]
        ql.eval()
        assert ex.weight.kind == "mx" and ex.weight.codes.is_cuda and R.same(ex.weight.dequantize(), ql.weight.detach())
        assert R.same(ex.bias.dequantize(), ql.bias.detach())
    act = qs.quantize(bits=8, timeout=2, channelwise=-1, callback=MXQuantizer("mxfp8_e5m2", block_dim=1)).train()
    for s in range(4):
        x = randn((4, 48, 5, 5), torch.bfloat16, seed=s)
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
        y = act(xd)
        if s < 2:
            assert y is xd
        else:
            assert R.same(y, R.reference(x, "mxfp8_e5m2", 1)[0]) and y.is_contiguous(memory_format=torch.channels_last)


def _mlp():
    torch.manual_seed(1)
    net = nn.Sequential(nn.Linear(64, 96), nn.ReLU(), nn.Linear(96, 10))
    net = qs.convert(net, qs.quantize(bits=8, timeout=2, callback=MXQuantizer("mxfp8_e4m3", block_dim=1)), weight_layers=[nn.Linear])
    net = qs.convert(net, qs.quantize(bits=4, timeout=2, channelwise=-1, callback=MXQuantizer("mxfp4_e2m1", block_dim=1)),
                     activation_layers=[nn.ReLU])
    return net.to(DEV).train()


def test_graphed_step_replay_equals_eager():
    """an MX network is stateless apart from the layers' step counters: GraphedStep captures it and replays step for step"""
    qs.set_qsparse_options(graph_safe=True)
    try:
        K = 10
        g = torch.Generator().manual_seed(0)
        data = [(torch.randn(32, 64, generator=g).to(DEV), torch.randint(0, 10, (32,), generator=g).to(DEV)) for _ in range(K)]
        results = []
        for wrapped in (False, True):
            model = _mlp()
            opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)

            def train_step(x, y):
                opt.zero_grad(set_to_none=False)
                loss = nn.functional.cross_entropy(model(x), y)
                loss.backward()
                opt.step()
                return loss.detach()

            step = graphs.GraphedStep(model, train_step) if wrapped else train_step
            losses = [float(step(x, y)) for x, y in data]
            if wrapped:
                assert step.captured, "the wrapper never reached graph replay"
                step.finish()
            results.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
        (le, se), (lg, sg) = results
        assert le == lg
        for k in se:
            assert torch.equal(se[k], sg[k]), k
    finally:
        qs.set_qsparse_options(graph_safe=False)
