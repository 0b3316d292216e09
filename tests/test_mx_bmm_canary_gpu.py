"""Out-of-bounds check for the batched MX products, in the manner of tests/test_mx_gemm_canary_gpu.py: ``y``, ``out_codes`` and
``out_scales`` are carved out of larger allocations whose margins hold a byte pattern (tests/mx_guard.py); after the launch not a byte
outside the G slices may have changed, and the bodies equal the stacked per-slice ``mx_matmul``.  G = 3 with M and N no multiples
of the 128-row tile, N % 4 != 0 and N % 32 != 0: single-element stores and a short last block in every slice, where a slice
stride or a tile edge that is off by a row would write into the next slice or past the last one.  ``tail``: the last slice ends at
the allocation's last byte, with the margin in front only."""
import pytest
import torch

import mx_gemm_ref as G
from mx_guard import PAD, PATTERN, guarded, intact
from qsparse_amd import _hip, mx_matmul, quantize_with_mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GN = 3
SHAPES = [(130, 33, 100), (5, 131, 64), (197, 67, 197)]       # M, N, K


def carve(nbytes, tail):
    """(raw, body, check): `body` of nbytes inside a pattern-filled allocation -- margins on both sides, or (tail) in front only"""
    if not tail:
        raw, body = guarded(nbytes)
        return raw, body, lambda: intact(raw, nbytes)
    raw = torch.full((PAD + nbytes,), PATTERN, dtype=torch.uint8, device=DEV)
    return raw, raw[PAD:], lambda: bool((raw[:PAD] == PATTERN).all())


def operands(g, M, N, K, fa, fb):
    x, w = torch.randn(GN, M, K, generator=g) * 2, torch.randn(GN, N, K, generator=g) / K ** 0.5
    return (tuple(quantize_with_mx(x.to(DEV), fa, -1, return_codes=True)[1:]) + (fa,) +
            tuple(quantize_with_mx(w.to(DEV), fb, -1, return_codes=True)[1:]) + (fb,))


def stacked(ops, bias, dt=torch.float32, **kw):
    ac, asc, fa, bc, bsc, fb = ops
    outs = [mx_matmul(ac[s], asc[s], fa, bc[s], bsc[s], fb, None if bias is None else bias[s], dt, **kw) for s in range(GN)]
    return torch.stack(outs) if kw.get("out_fmt") is None else tuple(torch.stack([o[j] for o in outs]) for j in range(2))


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("fa,fb", [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4_e2m1")])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_y_margins_survive(fa, fb, dt, tail):
    osz = torch.empty(0, dtype=dt).element_size()
    for M, N, K in SHAPES:
        assert M % 128 and N % 128 and N % 4 and N % 32
        g = torch.Generator().manual_seed(M + N + K)
        ops = operands(g, M, N, K, fa, fb)
        bias = torch.randn(GN, N, generator=g).to(DEV)
        raw, body, ok = carve(GN * M * N * osz, tail)
        y = _hip.mx_bmm(*ops, bias, dt, out=body.view(dt))
        torch.cuda.synchronize()
        assert y.data_ptr() == body.data_ptr() and _hip.mx_bmm_last_route == (_hip.MX_GEMM_ROUTE_VEC if K % 16 == 0 else _hip.MX_GEMM_ROUTE_PLAIN)
        assert ok(), ("y", fa, fb, dt, M, N, K, tail)
        assert G.same(y, stacked(ops, bias, dt)), (fa, fb, dt, M, N, K, tail)


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("act", [None, "relu"])
def test_codes_and_scales_margins_survive(act, tail):
    fa, fb, out_fmt = "mxfp8_e4m3", "mxfp6_e2m3", "mxfp4_e2m1"
    for M, N, K in SHAPES:
        g = torch.Generator().manual_seed(M + N + K + 1)
        ops = operands(g, M, N, K, fa, fb)
        bias = torch.randn(GN, N, generator=g).to(DEV)
        nb = (N + 31) // 32
        craw, cbody, cok = carve(GN * M * N, tail)
        sraw, sbody, sok = carve(GN * M * nb, tail)
        codes, scales = _hip.mx_bmm_q(*ops, bias, out_fmt, act, out=(cbody, sbody))
        torch.cuda.synchronize()
        assert codes.data_ptr() == cbody.data_ptr() and scales.data_ptr() == sbody.data_ptr()
        assert cok(), ("out_codes", act, M, N, K, tail)
        assert sok(), ("out_scales", act, M, N, K, tail)
        want = stacked(ops, bias, out_fmt=out_fmt, act=act)
        assert torch.equal(cbody.view(GN, M, N), want[0]) and torch.equal(sbody.view(GN, M, nb), want[1]), (act, M, N, K, tail)
