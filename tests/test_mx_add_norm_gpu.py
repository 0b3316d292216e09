"""The residual add fused into the MX norm family, on the GPU: qs_mx_add_norm_quant_v against the CPU path bit for bit (h, both pairs,
rstd, mean) and against the composition of the existing GPU calls, its routes; qs_mx_norm_bwd_res_v against the CPU path for every
pair of dtypes and every subset of the outputs; the training step of ``mx_add_norm_linear`` / ``MXTrainAddNormLinear`` against the CPU
and under graph capture.  The checks shared with the CPU are ``test_mx_add_norm.py``'s, on the device."""
import copy

import pytest
import torch
import torch.nn as nn

import mx_norm_bwd_ref as BR
import test_mx_add_norm as A
from mx_norm_ref import DTS, EPS, FMTS, NORMS, WB, same
from qsparse_amd import MXTrainAddNormLinear, _hip, mx_add_norm_quantize, mx_norm_backward, mx_norm_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_NORM_ROUTE_VEC, _hip.MX_NORM_ROUTE_PLAIN
ROWS, COLS = (1, 4, 33, 128, 129, 257), (1, 31, 32, 64, 96, 520, 1024, 4104)
_quiet = A._quiet


def dev(t):
    return None if t is None else t.to(DEV)


# ---- the forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdt,rdt", A.PAIRS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_gpu_equals_cpu(norm, xdt, rdt):
    """every R x C, (weight, bias) and the formats walking; the route is VEC exactly where C % 32 == 0 (torch's allocations are
    16-byte aligned); and the fused call equals torch.add + mx_norm_quantize on the GPU"""
    i = 0
    for R in ROWS:
        for C in COLS:
            has_w, has_b = WB[i % 4]
            x, res, w, b = A.add_inputs(1000 * R + C, R, C, xdt, rdt, has_w, has_b)
            kw = dict(norm=norm, eps=EPS, fmt=FMTS[i % 5], col_fmt=FMTS[(i + 2) % 5], return_stats=True)
            i += 1
            want = mx_add_norm_quantize(x, res, w, b, **kw)
            got = mx_add_norm_quantize(dev(x), dev(res), dev(w), dev(b), **kw)
            assert _hip.mx_add_norm_last_route == (VEC if C % 32 == 0 else PLAIN), (R, C)
            A.agree(got, want, (R, C, has_w, has_b, kw["fmt"]))
            h = torch.add(dev(res), dev(x)) if xdt == rdt else (dev(x).float() + dev(res).float()).to(rdt)
            A.agree(got, (h,) + tuple(mx_norm_quantize(h, dev(w), dev(b), **kw)), (R, C, "composition"))


@pytest.mark.parametrize("xdt,rdt", A.PAIRS, ids=str)
def test_offset_by_one_element_takes_the_plain_route(xdt, rdt):
    """each of x, residual, h alone one element off 16 bytes: PLAIN, the same bits (h through the binding's own allocation cannot be
    offset: it goes through the descriptor)"""
    import ctypes
    lib = _hip.load()
    for norm in NORMS:
        for R, C in ((129, 96), (33, 1024)):
            x, res, w, b = A.add_inputs(R + C, R, C, xdt, rdt)
            kw = dict(norm=norm, eps=EPS, fmt="mxfp8_e4m3", col_fmt="mxfp6_e3m2", return_stats=True)
            want = mx_add_norm_quantize(x, res, w, b, **kw)
            xbuf, rbuf = torch.zeros(R * C + 1, dtype=xdt, device=DEV), torch.zeros(R * C + 1, dtype=rdt, device=DEV)
            xbuf[1:] = dev(x).reshape(-1)
            rbuf[1:] = dev(res).reshape(-1)
            for xo, ro in ((xbuf[1:].view(R, C), dev(res)), (dev(x), rbuf[1:].view(R, C))):
                got = mx_add_norm_quantize(xo, ro, dev(w), dev(b), **kw)
                assert _hip.mx_add_norm_last_route == PLAIN
                A.agree(got, want, (norm, R, C))
            # h one element into its buffer, everything else aligned
            hbuf = torch.zeros(R * C + 1, dtype=rdt, device=DEV)
            outs = _hip._mx_quant2_outs((), R, C, kw["fmt"], kw["col_fmt"], DEV)
            rstd, mean = torch.empty(R, device=DEV), torch.empty(R, device=DEV)
            xd, rd, wd, bd = dev(x), dev(res), dev(w), dev(b)
            a = _hip.MxAddNormQuantArgs()
            a.struct_size = ctypes.sizeof(a)
            a.mode, a.row_format, a.col_format = NORMS.index(norm), _hip.MX_FORMATS.index(kw["fmt"]), _hip.MX_FORMATS.index(kw["col_fmt"])
            a.xdt, a.rdt, a.eps = _hip._DT[xdt], _hip._DT[rdt], EPS
            a.x, a.residual, a.h, a.weight, a.bias = xd.data_ptr(), rd.data_ptr(), hbuf[1:].data_ptr(), wd.data_ptr(), bd.data_ptr()
            a.row_codes, a.row_scales, a.col_codes, a.col_scales = [t.data_ptr() for t in outs]
            a.rstd, a.mean, a.R, a.C, a.stream = rstd.data_ptr(), mean.data_ptr(), R, C, _hip._stream(xd)
            assert lib.qs_mx_add_norm_quant_route(ctypes.byref(a)) == PLAIN and lib.qs_mx_add_norm_quant_v(ctypes.byref(a)) == 0
            torch.cuda.synchronize()
            got = (hbuf[1:].view(R, C),) + outs + (rstd, mean if norm == "layer" else None)
            A.agree(got, want, (norm, R, C, "h"))


def test_rounding_comes_before_the_sums_gpu():
    A.check_rounding_shows(DEV)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("xdt,rdt", A.PAIRS, ids=str)
def test_special_values_gpu(xdt, rdt, norm):
    A.check_special_values(DEV, xdt, rdt, norm)


def test_empty_and_devices():
    e = mx_add_norm_quantize(torch.zeros(0, 40, device=DEV), torch.zeros(0, 40, device=DEV), return_stats=True)
    assert _hip.mx_add_norm_last_route is None and e[0].shape == (0, 40) and e[1].shape == (0, 40) and e[3].shape == (0,)
    with pytest.raises(ValueError, match="x is on cuda:0 but residual on cpu"):
        mx_add_norm_quantize(torch.zeros(4, 40, device=DEV), torch.zeros(4, 40))


# ---- the backward with dresidual ---------------------------------------------------------------------------------------------------------
SUBSETS = ((True, False, False), (True, True, False), (True, False, True), (True, True, True))


@pytest.mark.parametrize("gdt", DTS, ids=str)
@pytest.mark.parametrize("xdt", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_backward_gpu_equals_cpu(norm, xdt, gdt):
    """the forward's shapes, every (xdt, gdt), every subset of the outputs that has dx; VEC exactly where C % 32 == 0; and
    dresidual=None is today's mx_norm_backward bit for bit"""
    i = 0
    for R in ROWS:
        for C in COLS:
            has_w = bool(i & 1)
            i += 1
            key = (R, C, xdt, norm, has_w, gdt)
            case, dres = BR.case(*key), A.dres_of(R, C, xdt)
            want = A.run_bwd("cpu", case, norm, dres)
            for needs in SUBSETS:
                got = A.run_bwd(DEV, case, norm, dres, need_dx=needs[0], need_dweight=needs[1], need_dbias=needs[2])
                assert _hip.mx_norm_bwd_last_route == (VEC if C % 32 == 0 else PLAIN), (R, C)
                for need, a, r in zip(needs, got, want):
                    assert (a is None) == (not need) and (a is None or same(a, r)), (R, C, has_w, needs)
            plain = A.run_bwd(DEV, case, norm, None)
            assert all(same(a, r) for a, r in zip(plain, A.run_bwd("cpu", case, norm, None))), (R, C, has_w)


def test_backward_checks_on_the_device():
    A.check_one_rounding(DEV)
    A.check_needs_with_dresidual(DEV)
    A.check_needs_with_dresidual(DEV, (129, 96, torch.float32, "rms"))
    x = torch.zeros(4, 40, device=DEV)
    with pytest.raises(ValueError, match="x is on cuda:0 but dresidual on cpu"):
        mx_norm_backward(x, x, torch.zeros(4, device=DEV), None, None, dresidual=torch.zeros(4, 40))


@pytest.mark.parametrize("dtype", DTS, ids=str)
def test_offset_dresidual_takes_the_plain_route(dtype):
    for norm in NORMS:
        for R, C in ((129, 96), (67, 1056)):
            dxhat, x, rstd, mean, w = A.to(DEV, BR.case(R, C, dtype, norm))
            dres = A.dres_of(R, C, dtype).to(DEV)
            want = mx_norm_backward(dxhat, x, rstd, mean, w, norm=norm, dresidual=dres)
            assert _hip.mx_norm_bwd_last_route == _hip.MX_NORM_BWD_ROUTE_VEC
            buf = torch.zeros(R * C + 1, dtype=dtype, device=DEV)
            buf[1:] = dres.reshape(-1)
            got = mx_norm_backward(dxhat, x, rstd, mean, w, norm=norm, dresidual=buf[1:].view(R, C))
            assert _hip.mx_norm_bwd_last_route == _hip.MX_NORM_BWD_ROUTE_PLAIN
            assert all(same(a, r) for a, r in zip(got, want)), (norm, R, C)


# ---- the training step ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("fused", "torch"))
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape,N", [((2, 33, 96), 64), ((129, 128), 32)])
def test_add_norm_linear_f32_gpu(shape, N, norm, mode):
    A.check_add_norm_linear_f32(DEV, shape, N, norm, mode)


@pytest.mark.parametrize("mode", ("fused", "torch"))
@pytest.mark.parametrize("norm", NORMS)
def test_add_norm_linear_dtypes_gpu(norm, mode):
    A.check_add_norm_linear_mixed(DEV, norm, mode)
    A.check_add_norm_linear_mixed(DEV, norm, mode, torch.bfloat16, torch.float32)
    if mode == "fused":
        A.bf16_dh_definition(DEV, norm)


@pytest.mark.parametrize("xdt", (torch.float32, torch.bfloat16), ids=str)
@pytest.mark.parametrize("mode", ("fused", "torch"))
@pytest.mark.parametrize("norm", NORMS)
def test_training_step_gpu_equals_cpu(norm, mode, xdt):
    """one step (nearest rounding) on both devices: y, h and every gradient bit for bit, on the operands of
    test_mx_add_norm.exact_step_case -- see there why the step's operands are drawn so that every sum is exact: the MX products
    accumulate in another order on the GPU than on the CPU, and torch's own reductions (norm_backward="torch", db) do as well.  The
    count of elements whose bits differ is printed before it is asserted"""
    got, want = A.exact_step(DEV, norm, mode, xdt), A.exact_step("cpu", norm, mode, xdt)
    differ = {}
    for name, a, r in zip(A.STEP_NAMES, got, want):
        assert (a is None) == (r is None), name
        if a is not None:
            assert a.dtype == r.dtype and a.shape == r.shape, name
            differ[name] = int((a.cpu().view(torch.uint8) != r.view(torch.uint8)).reshape(a.shape + (-1,)).any(-1).sum())
    print(f"{norm} {mode} x {xdt}: elements that differ between the GPU and the CPU: {differ}")
    assert all(v == 0 for v in differ.values()), differ


@pytest.mark.parametrize("norm", NORMS)
def test_captured_step_replays_bit_for_bit(norm):
    """forward and backward of one MXTrainAddNormLinear (the fused backward, a loss that uses y and h) under torch.cuda.graph, replayed on
    new inputs: equal to eager"""
    g = torch.Generator().manual_seed(12)
    M, K, N = 64, 128, 64
    draws = [[torch.randn(M, n, generator=g).to(DEV) for n in (K, K, N, K)] for _ in range(3)]      # x, residual, dy, dh
    torch.manual_seed(0)
    fnorm = (nn.RMSNorm(K, eps=1e-5) if norm == "rms" else nn.LayerNorm(K)).to(DEV)
    init = MXTrainAddNormLinear.from_float(fnorm, nn.Linear(K, N).to(DEV))
    assert init.norm_backward == "fused"

    def step(layer, x, res, dy, dh):
        for p in layer.parameters():
            p.grad = None
        xg, rg = x.detach().requires_grad_(True), res.detach().requires_grad_(True)
        y, h = layer(xg, rg)
        torch.autograd.backward((y, h), (dy, dh))
        return (y.detach(), h.detach(), xg.grad, rg.grad) + tuple(p.grad for p in layer.parameters())

    eager = copy.deepcopy(init)
    want = [tuple(t.clone() for t in step(eager, *d)) for d in draws]

    layer = copy.deepcopy(init)
    static = [t.clone() for t in draws[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(layer, *static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step(layer, *static)
    for d, ref in zip(draws, want):
        for s, t in zip(static, d):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert len(static_out) == len(ref) and all(same(a, r) for a, r in zip(static_out, ref))


def test_layers_gpu():
    A.check_layers(DEV)


# ---- the error codes of both entry points, in the header's order ---------------------------------------------------------------------------
def test_error_codes_with_a_device_present():
    A.test_add_norm_checks_in_the_documented_order()
    A.test_backward_res_checks_in_the_documented_order()
