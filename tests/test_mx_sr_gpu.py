"""Stochastic rounding of the MX quantizers on the GPU.  The definition is integer arithmetic on counter-based random words, so every
comparison here is bit for bit: the kernels against the package's CPU path (which tests/test_mx_sr.py holds to tests/mx_sr_ref.py)
and, where the index base matters, against that reference directly.  Routes are asserted, so each kernel is known to have run."""
import copy
import ctypes

import pytest
import torch

import mx_ref as R
import mx_sr_ref as S
from mx_guard import PATTERN, guarded as _guarded, intact as _intact
from qsparse_amd import _hip
from qsparse_amd.mx_gemm import MXTrainLinear, mx_linear, mx_matmul, mx_quantize_2way
from qsparse_amd.quantize import quantize_with_mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMTS = list(R.FORMATS)
PAIRS = [(f, FMTS[(i + 2) % 5]) for i, f in enumerate(FMTS)]          # every format once per pair, the two always different
DTYPES = (torch.float32, torch.bfloat16)
IV, IP, ST = _hip.MX_ROUTE_INNER_VEC, _hip.MX_ROUTE_INNER_PLAIN, _hip.MX_ROUTE_STRIDED
VEC, PLAIN = _hip.MX_Q2_ROUTE_TILE_VEC, _hip.MX_Q2_ROUTE_TILE_PLAIN
ONE_WAY = [((4, 64), -1, IV), ((6, 96), -1, IV), ((5, 45), -1, IP), ((3, 40, 5), 1, ST)]
TWO_WAY = [((160, 96), VEC), ((70, 45), PLAIN), ((33, 1), PLAIN), ((1, 33), PLAIN)]
BASE = 2 ** 34 - 8            # j >> 2 passes 2^32 at the ninth code: the counter's high word carries inside the tensor


def randn(shape, dtype, seed=0, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.exp(torch.randn((shape[0],) + (1,) * (len(shape) - 1), generator=g) * spread)).to(dtype)


def same_all(got, want):
    return all((a is None and b is None) or R.same(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_one_way_equals_the_cpu_path_on_every_route(fmt, dtype):
    for i, (shape, dim, route) in enumerate(ONE_WAY):
        x = randn(shape, dtype, seed=i)
        if shape == (6, 96):
            x[0, :32] = 0
            x[1, 40], x[2, 70], x[3, 5], x[4, 3] = float("nan"), float("inf"), -0.0, 1e-30
        step = torch.tensor([5])
        dstep = step.to(DEV)
        want = quantize_with_mx(x, fmt, dim, True, "stochastic", 11, step, 1)
        got = quantize_with_mx(x.to(DEV), fmt, dim, True, "stochastic", 11, dstep, 1)
        assert _hip.mx_last_route == route, (shape, _hip.mx_last_route)
        assert same_all(got, want), (shape, fmt, dtype)
        assert int(dstep) == 5                                                # read, never written
        nearest = quantize_with_mx(x.to(DEV), fmt, dim, True)
        # nearest mode asked for by name, with rounding operands it must ignore: the same bytes
        again = _hip.mx_quant_fwd(x.to(DEV), fmt, dim % x.dim(), torch.float32, True, "nearest", 11, dstep, 1)
        assert _hip.mx_last_route == route and same_all(again, nearest)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
def test_two_way_equals_the_cpu_path_on_both_routes(row_fmt, col_fmt, dtype):
    for i, (shape, route) in enumerate(TWO_WAY):
        x = randn(shape, dtype, seed=10 + i)
        if shape == (160, 96):
            x[3, 40], x[150, 7], x[64:96, 70] = float("nan"), float("inf"), 0
        step = torch.tensor([2 ** 40 + 3])
        dstep = step.to(DEV)
        for rf, cf in ((row_fmt, col_fmt), (row_fmt, None), (None, col_fmt)):
            want = mx_quantize_2way(x, rf, cf, "stochastic", -7, step)
            got = mx_quantize_2way(x.to(DEV), rf, cf, "stochastic", -7, dstep)
            assert _hip.mx_quant2_last_route == route, (shape, rf, cf)
            assert same_all(got, want), (shape, rf, cf, dtype)
            nearest = _hip.mx_quant2(x.to(DEV), rf, cf)
            old_route = _hip.mx_quant2_last_route
            again = _hip.mx_quant2(x.to(DEV), rf, cf, "nearest", -7, dstep)
            assert _hip.mx_quant2_last_route == old_route and same_all(again, nearest)
        assert int(dstep) == 2 ** 40 + 3


@pytest.mark.parametrize("fmt", ["mxfp4_e2m1", "mxfp8_e4m3"])
def test_index_base_across_a_carry_of_the_counter_against_the_reference(fmt):
    x = randn((4, 64), torch.float32, seed=3)
    got = _hip.mx_quant_fwd(x.to(DEV), fmt, 1, torch.float32, True, "stochastic", 21, None, 2, BASE)
    assert _hip.mx_last_route == IV
    assert same_all(got, S.reference(x, fmt, -1, torch.float32, 21, 0, 2, BASE))
    assert not torch.equal(got[1], _hip.mx_quant_fwd(x.to(DEV), fmt, 1, torch.float32, True, "stochastic", 21, None, 2, 0)[1])
    x = randn((160, 96), torch.bfloat16, seed=4)
    other = FMTS[(FMTS.index(fmt) + 2) % 5]
    dstep = torch.tensor([9], device=DEV)
    rc, rs, cc, cs = _hip.mx_quant2(x.to(DEV), fmt, other, "stochastic", 21, dstep, BASE)
    assert _hip.mx_quant2_last_route == VEC
    _, c, s = S.reference(x, fmt, -1, torch.float32, 21, 9, 0, BASE)
    assert R.same(rc, c) and R.same(rs, s)
    _, c, s = S.reference(x.t().contiguous(), other, -1, torch.float32, 21, 9, 1, BASE)
    assert R.same(cc, c) and R.same(cs, s)


@pytest.mark.parametrize("dtype", DTYPES)
def test_margins_and_step_survive_the_stochastic_entry_points(dtype):
    """the canary scheme of tests/test_mx_quant2_canary_gpu.py: x, every output and the step counter are carved out of pattern-filled
    allocations; after the launch the margins are intact, x and step unchanged, the outputs those of the CPU path"""
    lib = _hip.load()
    esz = torch.empty(0, dtype=dtype).element_size()
    sraw, sbody = _guarded(8)
    step = torch.tensor([77])
    sbody.copy_(step.view(torch.uint8).to(DEV))
    seed, rf, cf = 2 ** 63 + 5, "mxfp4_e2m1", "mxfp6_e3m2"
    # two-way: R, C, element offset of x, byte offset of the outputs, route
    for R_, C, xoff, ooff, route in ((144, 200, 0, 0, VEC), (160, 72, 0, 16, VEC), (129, 65, 1, 7, PLAIN), (33, 31, 0, 1, PLAIN)):
        x = randn((R_, C), dtype, seed=R_)
        xraw, xbody = _guarded(R_ * C * esz, xoff * esz)
        xbody.copy_(x.view(torch.uint8).reshape(-1).to(DEV))
        nbr, nbc = -(-R_ // 32), -(-C // 32)
        sizes = dict(row_codes=R_ * C, row_scales=R_ * nbc, col_codes=C * R_, col_scales=C * nbr)
        out = {n: _guarded(sz, ooff) for n, sz in sizes.items()}
        a = _hip.MxQuant2Args()
        a.struct_size = ctypes.sizeof(a)
        a.row_format, a.col_format = _hip.MX_FORMATS.index(rf), _hip.MX_FORMATS.index(cf)
        a.x, a.xdt, a.R, a.C = xbody.data_ptr(), _hip._DT[dtype], R_, C
        for n in sizes:
            setattr(a, n, out[n][1].data_ptr())
        a.stream = _hip._stream(xbody)
        a.rounding, a.seed, a.step, a.index_base = 1, seed, sbody.data_ptr(), 4
        what = (dtype, R_, C, xoff, ooff)
        assert lib.qs_mx_quant2_route(ctypes.byref(a)) == route, what
        assert lib.qs_mx_quant2_v(ctypes.byref(a)) == 0, what
        torch.cuda.synchronize()
        assert _intact(xraw, R_ * C * esz, xoff * esz) and torch.equal(xbody.cpu(), x.view(torch.uint8).reshape(-1)), ("x", what)
        assert _intact(sraw, 8) and torch.equal(sbody.cpu(), step.view(torch.uint8)), ("step", what)
        for n, sz in sizes.items():
            assert _intact(out[n][0], sz, ooff), (n, what)
        _, c, s = S.reference(x, rf, -1, torch.float32, seed, 77, 0, 4) if R_ == 33 else (None,) + _cpu_pair(x, rf, seed, 77, 0, 4)
        assert torch.equal(out["row_codes"][1].cpu().view(R_, C), c) and torch.equal(out["row_scales"][1].cpu().view(R_, nbc), s), what
        _, c, s = (None,) + _cpu_pair(x.t().contiguous(), cf, seed, 77, 1, 4)
        assert torch.equal(out["col_codes"][1].cpu().view(C, R_), c) and torch.equal(out["col_scales"][1].cpu().view(C, nbr), s), what
    # one-way: shape as [outer, n, inner], element offset of x and y / byte offset of codes and scales, route
    for (outer, n, inner), off, route in (((6, 96, 1), 0, IV), ((5, 45, 1), 1, IP), ((3, 40, 5), 1, ST)):
        numel, nb = outer * n * inner, -(-n // 32)
        x = randn((outer, n, inner), dtype, seed=n)
        xraw, xbody = _guarded(numel * esz, off * esz)
        xbody.copy_(x.view(torch.uint8).reshape(-1).to(DEV))
        yraw, ybody = _guarded(numel * 4, off * 4)
        craw, cbody = _guarded(numel, off)
        scraw, scbody = _guarded(outer * nb * inner, off)
        a = _hip.MxQuantArgs()
        a.struct_size = ctypes.sizeof(a)
        a.format = _hip.MX_FORMATS.index(rf)
        a.x, a.y, a.codes, a.scales = xbody.data_ptr(), ybody.data_ptr(), cbody.data_ptr(), scbody.data_ptr()
        a.xdt, a.ydt, a.outer, a.n, a.inner = _hip._DT[dtype], _hip.F32, outer, n, inner
        a.stream = _hip._stream(xbody)
        a.rounding, a.rng_stream, a.seed, a.step, a.index_base = 1, 3, seed, sbody.data_ptr(), 8
        what = (dtype, outer, n, inner)
        assert lib.qs_mx_quant_route(ctypes.byref(a)) == route, what
        assert lib.qs_mx_quant_fwd_v(ctypes.byref(a)) == 0, what
        torch.cuda.synchronize()
        assert _intact(xraw, numel * esz, off * esz) and torch.equal(xbody.cpu(), x.view(torch.uint8).reshape(-1)), ("x", what)
        assert _intact(sraw, 8) and torch.equal(sbody.cpu(), step.view(torch.uint8)), ("step", what)
        assert _intact(yraw, numel * 4, off * 4) and _intact(craw, numel, off) and _intact(scraw, outer * nb * inner, off), what
        y, c, s = S.reference(x, rf, 1, torch.float32, seed, 77, 3, 8)
        assert torch.equal(cbody.cpu().view(outer, n, inner), c) and torch.equal(scbody.cpu().view(outer, nb, inner), s), what
        assert R.same(ybody.cpu().view(torch.float32).view(outer, n, inner), y), what


def _cpu_pair(x, fmt, seed, step, stream, base):
    """codes and scales of the package's CPU path with an index base (which the public call does not take)"""
    from qsparse_amd.quantize import _mx_aten, _mx_sr_words
    return _mx_aten(x, fmt, x.dim() - 1, torch.float32, True, _mx_sr_words(x.shape, seed, step, stream, base))[1:]


# sizeof(qs_mx_quant_args) / sizeof(qs_mx_quant2_args) as ABI v27 had them: where the fields appended in v28 begin
V27_SIZE_1, V27_SIZE_2 = _hip.MxQuantArgs.rounding.offset, _hip.MxQuant2Args.rounding.offset


def _raw_one_way(run, route, x, dim, fmt, size=None, **rounding_operands):
    """(y, codes, scales), route: one call of the C entry point `run` on a contiguous GPU tensor, outputs pre-filled with a pattern"""
    outer, n, inner, numel = _hip.split3(x.shape, dim)
    y = torch.zeros(x.shape, dtype=torch.float32, device=DEV)
    codes = torch.full(x.shape, PATTERN, dtype=torch.uint8, device=DEV)
    sshape = list(x.shape)
    sshape[dim] = -(-n // 32)
    scales = torch.full(sshape, PATTERN, dtype=torch.uint8, device=DEV)
    a = _hip.MxQuantArgs()
    a.struct_size = ctypes.sizeof(a) if size is None else size
    a.format = _hip.MX_FORMATS.index(fmt)
    a.x, a.y, a.codes, a.scales = x.data_ptr(), y.data_ptr(), codes.data_ptr(), scales.data_ptr()
    a.xdt, a.ydt, a.outer, a.n, a.inner = _hip._DT[x.dtype], _hip.F32, outer, n, inner
    a.stream = _hip._stream(x)
    for k, v in rounding_operands.items():
        setattr(a, k, v)
    r = route(ctypes.byref(a))
    assert run(ctypes.byref(a)) == 0
    torch.cuda.synchronize()
    return (y, codes, scales), r


def _raw_two_way(run, route, x, rf, cf, size=None, **rounding_operands):
    """(row_codes, row_scales, col_codes, col_scales), route: one call of the C entry point `run` on a contiguous GPU tensor [R, C]"""
    R_, C = x.shape
    out = [torch.full(shape, PATTERN, dtype=torch.uint8, device=DEV) for shape in ((R_, C), (R_, -(-C // 32)), (C, R_), (C, -(-R_ // 32)))]
    a = _hip.MxQuant2Args()
    a.struct_size = ctypes.sizeof(a) if size is None else size
    a.row_format, a.col_format = _hip.MX_FORMATS.index(rf), _hip.MX_FORMATS.index(cf)
    a.x, a.xdt, a.R, a.C = x.data_ptr(), _hip._DT[x.dtype], R_, C
    a.row_codes, a.row_scales, a.col_codes, a.col_scales = (t.data_ptr() for t in out)
    a.stream = _hip._stream(x)
    for k, v in rounding_operands.items():
        setattr(a, k, v)
    r = route(ctypes.byref(a))
    assert run(ctypes.byref(a)) == 0
    torch.cuda.synchronize()
    return tuple(out), r


@pytest.mark.parametrize("fmt", FMTS)
def test_a_v27_sized_descriptor_is_nearest_rounding(fmt):
    """a caller compiled against the v27 header passes the v27 struct_size; what lies behind it -- here rounding = 1, seed = 5 -- is
    never read: the bytes of the full descriptor with rounding = 0, and those of tests/mx_ref.py"""
    lib = _hip.load()
    for shape, dim, route in (((4, 64), 1, IV), ((3, 45), 1, IP), ((2, 40, 5), 1, ST)):
        x = randn(shape, torch.bfloat16, seed=len(shape))
        xd = x.to(DEV)
        old, r_old = _raw_one_way(lib.qs_mx_quant_fwd_v, lib.qs_mx_quant_route, xd, dim, fmt, V27_SIZE_1, rounding=1, seed=5)
        new, r_new = _raw_one_way(lib.qs_mx_quant_fwd_v, lib.qs_mx_quant_route, xd, dim, fmt, rounding=0, seed=5)
        assert r_old == r_new == route, (shape, r_old, r_new)
        assert same_all(old, new) and same_all(old, R.reference(x, fmt, dim)), (shape, fmt)
    other = FMTS[(FMTS.index(fmt) + 2) % 5]
    for shape, route in (((128, 64), VEC), ((33, 45), PLAIN)):
        x = randn(shape, torch.bfloat16, seed=shape[0])
        xd = x.to(DEV)
        old, r_old = _raw_two_way(lib.qs_mx_quant2_v, lib.qs_mx_quant2_route, xd, fmt, other, V27_SIZE_2, rounding=1, seed=5)
        new, r_new = _raw_two_way(lib.qs_mx_quant2_v, lib.qs_mx_quant2_route, xd, fmt, other, rounding=0, seed=5)
        assert r_old == r_new == route, (shape, r_old, r_new)
        want = R.reference(x, fmt, -1)[1:] + R.reference(x.t().contiguous(), other, -1)[1:]
        assert same_all(old, new) and same_all(old, want), (shape, fmt, other)


def test_the_v27_alias_symbols_are_the_call():
    lib = _hip.load()
    step = torch.tensor([9], device=DEV)
    sr = dict(rounding=1, seed=21, step=step.data_ptr(), index_base=8)
    x = randn((4, 64), torch.bfloat16, seed=1).to(DEV)
    alias, r_alias = _raw_one_way(lib.qs_mx_quant_sr_v, lib.qs_mx_quant_sr_route, x, 1, "mxfp4_e2m1", **sr)
    call, r_call = _raw_one_way(lib.qs_mx_quant_fwd_v, lib.qs_mx_quant_route, x, 1, "mxfp4_e2m1", **sr)
    assert r_alias == r_call == IV and same_all(alias, call)
    assert same_all(call, S.reference(x.cpu(), "mxfp4_e2m1", -1, torch.float32, 21, 9, 0, 8))      # (the operands were read)
    x = randn((128, 64), torch.bfloat16, seed=2).to(DEV)
    alias, r_alias = _raw_two_way(lib.qs_mx_quant2_sr_v, lib.qs_mx_quant2_sr_route, x, "mxfp4_e2m1", "mxfp6_e3m2", **sr)
    call, r_call = _raw_two_way(lib.qs_mx_quant2_v, lib.qs_mx_quant2_route, x, "mxfp4_e2m1", "mxfp6_e3m2", **sr)
    assert r_alias == r_call == VEC and same_all(alias, call)
    assert R.same(call[0], S.reference(x.cpu(), "mxfp4_e2m1", -1, torch.float32, 21, 9, 0, 8)[1])
    assert int(step) == 9


ALIGNED, RAGGED = (512, 576, 640), (530, 522, 542)        # the shapes of tests/test_mx_train_gpu.py


@pytest.mark.parametrize("shape,dtype", [(ALIGNED, torch.bfloat16), (RAGGED, torch.float32)])
def test_mx_linear_rounds_the_two_forms_of_dy_and_nothing_else(shape, dtype):
    M, N, K = shape
    FX, FW, FG, seed = "mxfp8_e4m3", "mxfp8_e4m3", "mxfp4_e2m1", 1234
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(M, K, generator=g) * 2).to(dtype).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    dy = (torch.randn(M, N, generator=g) / N).to(dtype).to(DEV)
    step = torch.tensor([3], device=DEV)
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = mx_linear(xg, wg, None, FX, FW, FG, "stochastic", seed, step)
    y.backward(dy)
    assert int(step) == 4
    xn, wn = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yn = mx_linear(xn, wn, None, FX, FW, FG)
    yn.backward(dy)
    assert torch.equal(y, yn) and not torch.equal(xg.grad, xn.grad) and not torch.equal(wg.grad, wn.grad)
    three = torch.tensor([3], device=DEV)
    with torch.no_grad():
        _, g_row, g_rs = quantize_with_mx(dy, FG, -1, True, "stochastic", seed, three, 0)
        _, g_col, g_cs = quantize_with_mx(dy.t().contiguous(), FG, -1, True, "stochastic", seed, three, 1)
        _, w_col, w_cs = quantize_with_mx(w.t().contiguous(), FW, -1, True)
        _, x_col, x_cs = quantize_with_mx(x.t().contiguous(), FX, -1, True)
    assert torch.equal(xg.grad, mx_matmul(g_row, g_rs, FG, w_col, w_cs, FW, None, dtype))
    assert torch.equal(wg.grad, mx_matmul(g_col, g_cs, FG, x_col, x_cs, FX, None, torch.float32))
    cpu = mx_quantize_2way(dy.cpu(), FG, FG, "stochastic", seed, torch.tensor([3]))
    assert same_all((g_row, g_rs, g_col, g_cs), cpu)


def test_captured_step_draws_new_words_on_every_replay():
    """forward + backward of one stochastic MXTrainLinear under torch.cuda.graph (a single layer: no parallel branches).  The seed
    is a launch argument and frozen into the graph; the step counter is device memory the kernel reads and the captured add_ advances"""
    g = torch.Generator().manual_seed(11)
    M, K, N = 256, 192, 128
    x = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    t = torch.randn(M, N, generator=g).bfloat16().to(DEV)
    torch.manual_seed(0)
    init = MXTrainLinear(K, N, grad_fmt="mxfp4_e2m1", grad_rounding="stochastic", seed=99).to(DEV)
    assert init.sr_step.device.type == "cuda" and int(init.sr_step) == 0

    def step(layer, x, t):
        y = layer(x)
        gy = ((y - t) / y.numel()).detach()
        for p in layer.parameters():
            p.grad = None
        y.backward(gy)
        return y.detach()

    layer = copy.deepcopy(init)
    static_x, static_t = x.clone(), t.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(layer, static_x, static_t)
    torch.cuda.current_stream().wait_stream(side)
    assert int(layer.sr_step) == 1                          # the warm-up
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(layer, static_x, static_t)
    grads = []
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(layer.sr_step) == 2 + i                  # warm-ups plus replays
        grads.append(layer.weight.grad.clone())
    assert not torch.equal(grads[0], grads[1]) and not torch.equal(grads[1], grads[2]) and not torch.equal(grads[0], grads[2])
    for i, got in enumerate(grads):                         # replay i ran at step 1 + i
        eager = copy.deepcopy(init)
        eager.sr_step.fill_(1 + i)
        step(eager, x, t)
        assert torch.equal(eager.weight.grad, got), i
        assert int(eager.sr_step) == 2 + i
