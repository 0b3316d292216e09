"""``mx_norm_backward`` on the GPU: qs_mx_norm_bwd_v against the CPU path bit for bit (every shape, mode and dtype, a bfloat16 dxhat,
every subset of the outputs, the PLAIN route on offset tensors), against float64, special values, the fused backward of
``mx_norm_linear`` / ``MXTrainNormLinear`` (the checks of ``test_mx_norm_bwd.py`` on the device) and graph capture."""
import copy

import pytest
import torch
import torch.nn as nn

import mx_norm_bwd_ref as BR
import test_mx_norm_bwd as B
from mx_norm_ref import DTS, NORMS, same
from qsparse_amd import MXTrainNormLinear, _hip, mx_norm_backward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_NORM_BWD_ROUTE_VEC, _hip.MX_NORM_BWD_ROUTE_PLAIN
_quiet = B._quiet


# ---- test 3: GPU against CPU, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_gpu_equals_cpu(norm, dtype):
    """every shape, with and without weight; the route is VEC exactly where C % 32 == 0 (torch's allocations are 16-byte aligned)"""
    for R, C in BR.SHAPES:
        for has_w in (True, False):
            case = BR.case(R, C, dtype, norm, has_w)
            want = B.run("cpu", case, norm)
            got = B.run(DEV, case, norm)
            assert _hip.mx_norm_bwd_last_route == (VEC if C % 32 == 0 else PLAIN), (R, C)
            for name, a, r in zip(B.NAMES, got, want):
                assert same(a, r), (name, R, C, has_w)


@pytest.mark.parametrize("norm", NORMS)
def test_bfloat16_dxhat(norm):
    for R, C, dtype in ((300, 520, torch.bfloat16), (129, 96, torch.float32)):
        case = BR.case(R, C, dtype, norm, True, torch.bfloat16)
        assert case[0].dtype == torch.bfloat16
        assert all(same(a, r) for a, r in zip(B.run(DEV, case, norm), B.run("cpu", case, norm)))


def test_every_subset_of_the_outputs():
    B.check_every_subset(DEV, (300, 520, torch.bfloat16, "layer"))
    B.check_every_subset(DEV, (129, 96, torch.float32, "rms"))


@pytest.mark.parametrize("dtype", DTS, ids=str)
def test_offset_by_one_element_takes_the_plain_route(dtype):
    for norm in NORMS:
        for R, C in ((129, 96), (67, 1056)):
            dxhat, x, rstd, mean, w = B.to(DEV, BR.case(R, C, dtype, norm))
            want = mx_norm_backward(dxhat, x, rstd, mean, w, norm=norm)
            assert _hip.mx_norm_bwd_last_route == VEC
            xbuf = torch.zeros(R * C + 1, dtype=dtype, device=DEV)
            xbuf[1:] = x.reshape(-1)
            gbuf = torch.zeros(R * C + 1, device=DEV)
            gbuf[1:] = dxhat.reshape(-1)
            for xo, go in ((xbuf[1:].view(R, C), dxhat), (x, gbuf[1:].view(R, C)), (xbuf[1:].view(R, C), gbuf[1:].view(R, C))):
                got = mx_norm_backward(go, xo, rstd, mean, w, norm=norm)
                assert _hip.mx_norm_bwd_last_route == PLAIN
                assert all(same(a, r) for a, r in zip(got, want)), (norm, R, C)


# ---- tests 2 and 4 on the device -----------------------------------------------------------------------------------------------------
def test_against_float64_gpu():
    B.check_against_float64(DEV)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("dtype", DTS, ids=str)
def test_special_values_gpu(dtype, norm):
    B.check_special_values(DEV, dtype, norm)


@pytest.mark.parametrize("norm", NORMS)
def test_f16_row_of_65504_gpu(norm):
    case = B.f16_max_case(norm)
    assert all(same(a, r) for a, r in zip(B.run(DEV, case, norm), B.run("cpu", case, norm)))


def test_empty_tensors_enqueue_nothing():
    e = mx_norm_backward(torch.zeros(0, 40, device=DEV), torch.zeros(0, 40, device=DEV), torch.zeros(0, device=DEV), None, None)
    assert _hip.mx_norm_bwd_last_route is None
    assert e[0].shape == (0, 40) and same(e[1].cpu(), torch.zeros(40)) and same(e[2].cpu(), torch.zeros(40))
    with pytest.raises(ValueError, match="x is on cuda:0 but rstd on cpu"):
        mx_norm_backward(torch.zeros(4, 40, device=DEV), torch.zeros(4, 40, device=DEV), torch.zeros(4), None, None)


# ---- test 5 on the device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape,N", [((2, 33, 96), 64), ((129, 128), 32)])
def test_fused_norm_linear_gpu(shape, N, norm):
    B.check_fused_norm_linear(DEV, shape, N, norm)


def test_needs_reach_the_call_gpu(monkeypatch):
    B.check_needs_reach_the_call(DEV, monkeypatch)


def test_fused_layer_gpu():
    B.check_fused_layer(DEV)


# ---- test 6: graph capture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
def test_captured_fused_step_replays_bit_for_bit(norm):
    """forward and backward of one MXTrainNormLinear with the fused norm backward under torch.cuda.graph (a single layer: no parallel
    branches), replayed on three inputs"""
    g = torch.Generator().manual_seed(12)
    M, K, N = 64, 128, 64
    xs = [torch.randn(M, K, generator=g).to(DEV) for _ in range(3)]
    dys = [torch.randn(M, N, generator=g).to(DEV) for _ in range(3)]
    torch.manual_seed(0)
    fnorm = (nn.RMSNorm(K, eps=1e-5) if norm == "rms" else nn.LayerNorm(K)).to(DEV)
    init = MXTrainNormLinear.from_float(fnorm, nn.Linear(K, N).to(DEV), norm_backward="fused")

    def step(layer, x, dy):
        for p in layer.parameters():
            p.grad = None
        xg = x.detach().requires_grad_(True)
        y = layer(xg)
        y.backward(dy)
        return (y.detach(), xg.grad) + tuple(p.grad for p in layer.parameters())

    eager = copy.deepcopy(init)
    want = [tuple(t.clone() for t in step(eager, x, dy)) for x, dy in zip(xs, dys)]

    layer = copy.deepcopy(init)
    static_x, static_dy = xs[0].clone(), dys[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(layer, static_x, static_dy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step(layer, static_x, static_dy)
    for x, dy, ref in zip(xs, dys, want):
        static_x.copy_(x)
        static_dy.copy_(dy)
        graph.replay()
        torch.cuda.synchronize()
        assert len(static_out) == len(ref) and all(same(a, r) for a, r in zip(static_out, ref))
