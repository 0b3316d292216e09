"""``mx_softmax_quantize`` on the GPU: the bytes of qs_mx_softmax_quant_v against the CPU path (tests/test_mx_softmax.py pins that to
the definition) over the CPU tests' matrix and the shapes at which the kernel changes its path, the routes, the empty tensor,
``mx_attention(softmax="fused")`` against its composition on the device, and graph capture."""
import pytest
import torch

import mx_softmax_ref as SR
import test_mx_softmax as TS
from qsparse_amd import _hip, mx_attention, mx_softmax_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_SOFTMAX_ROUTE_VEC, _hip.MX_SOFTMAX_ROUTE_PLAIN


def to_dev(kw):
    return {k: v.to(DEV) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}


def check(s, fmt, scale=TS.SCALE, route=None, **kw):
    """one GPU call against the CPU path of the same call, bit for bit"""
    want = mx_softmax_quantize(s, scale=scale, fmt=fmt, **kw)
    got = mx_softmax_quantize(s.to(DEV), scale=scale, fmt=fmt, **to_dev(kw))
    if route is not None:
        assert _hip.mx_softmax_last_route == route, (tuple(s.shape), fmt, _hip.mx_softmax_last_route)
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == torch.uint8 and torch.equal(g.cpu(), w), (tuple(s.shape), s.dtype, fmt, sorted(kw))


@pytest.mark.parametrize("S", SR.SIZES)
@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
def test_gpu_equals_the_cpu_path(dtype, S):
    for variant in TS.VARIANTS:
        s, kw, _ = TS.case(dtype, S, variant)
        for fmt in SR.FMTS:
            check(s, fmt, **kw)


@pytest.mark.parametrize("S,route", ((1024, VEC), (1025, PLAIN), (1032, PLAIN), (1056, VEC)))
@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
def test_rows_past_the_registers(dtype, S, route):
    """S <= 1024 is walked in registers, a longer row three times from memory: the same bytes on either side of the bound, both routes"""
    s = SR.scores(S, (2, 3, S), dtype)
    for fmt in ("mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e3m2"):
        check(s, fmt, route=route)
        check(s, fmt, route=route, mask=SR.float_mask(S + 1, (3, S)))
        check(s, fmt, route=route, mask=SR.bool_mask(S + 2, (2, 3, S)))
    s5 = SR.scores(S + 3, (1, 5, S), dtype)
    check(s5, "mxfp8_e5m2", route=route, is_causal=True)


@pytest.mark.parametrize("T", (1, 4, 5))
@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
def test_rows_per_work_group(dtype, T):
    """four rows per work-group: a last group of one, of four, and a fifth row"""
    for G, S in ((1, 197), (3, 197), (6, 64), (3, 40)):
        s = SR.scores(10 * T + G, (G, T, S), dtype)
        for fmt in ("mxfp8_e4m3", "mxfp6_e2m3"):
            check(s, fmt)
            check(s, fmt, is_causal=True)
            check(s, fmt, mask=SR.float_mask(T, (G, T, S)))


def test_routes():
    for S, route in ((64, VEC), (72, PLAIN), (197, PLAIN), (32, VEC), (31, PLAIN)):
        s = SR.scores(S, (2, 5, S), torch.bfloat16)
        check(s, "mxfp8_e4m3", route=route)
        check(s, "mxfp8_e4m3", route=route, mask=SR.float_mask(S, (5, S)))
    # a base off its 16 bytes by one element: PLAIN at an S that would take VEC, for s and for the mask alone
    for dtype in SR.DTS:
        s = SR.scores(5, (2, 5, 64), dtype)
        flat = torch.empty(s.numel() + 1, dtype=dtype, device=DEV)
        off = flat[1:].view(2, 5, 64).copy_(s)
        assert off.data_ptr() % 16 != 0 and off.is_contiguous()
        want = mx_softmax_quantize(s, scale=TS.SCALE)
        got = mx_softmax_quantize(off, scale=TS.SCALE)
        assert _hip.mx_softmax_last_route == PLAIN and all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
    s = SR.scores(6, (2, 5, 64), torch.float32)
    mask = SR.float_mask(7, (5, 64))
    mflat = torch.empty(mask.numel() + 1, dtype=torch.float32, device=DEV)
    moff = mflat[1:].view(5, 64).copy_(mask)
    want = mx_softmax_quantize(s, mask, scale=TS.SCALE)
    got = mx_softmax_quantize(s.to(DEV), moff, scale=TS.SCALE)
    assert _hip.mx_softmax_last_route == PLAIN and all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
    got = mx_softmax_quantize(s.to(DEV), mask.to(DEV), scale=TS.SCALE)
    assert _hip.mx_softmax_last_route == VEC and all(torch.equal(g.cpu(), w) for g, w in zip(got, want))


@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
def test_exceptional_rows_on_the_gpu(dtype):
    s, mask, _ = TS._special_rows(dtype)
    for fmt in SR.FMTS:
        check(s, fmt, mask=mask)
    check(SR.scores(11, (2, 3, 70), dtype), "mxfp8_e4m3", scale=0.0)
    check(SR.scores(11, (2, 3, 70), dtype), "mxfp8_e4m3", scale=-0.37)


def test_empty_tensor():
    for shape in ((0, 4, 33), (2, 0, 33), (2, 4, 0)):
        codes, scales = mx_softmax_quantize(torch.zeros(shape, device=DEV))
        assert _hip.mx_softmax_last_route is None
        assert codes.shape == shape and scales.shape == shape[:2] + ((shape[2] + 31) // 32,) and codes.is_cuda and scales.is_cuda


def test_mask_on_the_wrong_device_is_refused():
    with pytest.raises(ValueError):
        mx_softmax_quantize(torch.zeros(2, 4, 33, device=DEV), torch.zeros(4, 33))


def test_fused_attention_equals_its_composition_on_the_gpu():
    q, k, v = (t.to(DEV) for t in TS._qkv(5, (2, 3, 37, 16), 37, 16))
    got = mx_attention(q, k, v, is_causal=True, softmax="fused")
    assert torch.equal(got, TS.fused_composition(q, k, v, is_causal=True))
    q, k, v = (t.to(DEV) for t in TS._qkv(6, (2, 2, 33, 40), 45, 24, torch.bfloat16))
    mask = SR.float_mask(9, (33, 45)).to(DEV)
    got = mx_attention(q, k, v, mask, softmax="fused")
    assert torch.equal(got, TS.fused_composition(q, k, v, mask))
    assert not torch.equal(got, torch.zeros_like(got)) and bool(got.isfinite().all())


def test_captured_call_replays_bit_for_bit():
    """one linear capture (no parallel branches) of the call, replayed once on new scores"""
    first, second = SR.scores(1, (3, 7, 197), torch.float32), SR.scores(2, (3, 7, 197), torch.float32)
    mask = SR.float_mask(3, (7, 197))
    want = mx_softmax_quantize(second, mask, scale=TS.SCALE)
    static_s, dmask = first.to(DEV), mask.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mx_softmax_quantize(static_s, dmask, scale=TS.SCALE)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mx_softmax_quantize(static_s, dmask, scale=TS.SCALE)
    static_s.copy_(second.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o.cpu(), w) for o, w in zip(out, want))
