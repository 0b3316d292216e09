"""Out-of-bounds check for the MX matrix product, in the manner of tests/test_mx_canary_gpu.py: all five operands and the output
of every call are carved out of larger allocations whose margins hold a byte pattern; after the launch the margins must be
intact (y: nothing written past it; the inputs: unchanged) and the body equal the CPU reference.  Margins on both sides also mean
that a read past an operand would pick up the pattern instead of zeros and show in the result.  Ragged M, N, K and unaligned
bases are where this kernel would reach too far."""
import ctypes

import pytest
import torch

import mx_gemm_ref as G
from mx_guard import guarded as _guarded, intact as _intact
from qsparse_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


CASES = [  # M, N, K, byte offset of the code bases, expected route
    (128, 128, 128, 0, _hip.MX_GEMM_ROUTE_VEC), (1, 1, 16, 0, _hip.MX_GEMM_ROUTE_VEC), (129, 127, 144, 0, _hip.MX_GEMM_ROUTE_VEC),
    (37, 301, 400, 0, _hip.MX_GEMM_ROUTE_VEC), (5, 3, 1, 0, _hip.MX_GEMM_ROUTE_PLAIN), (130, 67, 129, 0, _hip.MX_GEMM_ROUTE_PLAIN),
    (17, 129, 31, 3, _hip.MX_GEMM_ROUTE_PLAIN), (64, 64, 256, 1, _hip.MX_GEMM_ROUTE_PLAIN), (200, 9, 1000, 0, _hip.MX_GEMM_ROUTE_PLAIN),
]


@pytest.mark.parametrize("fa,fb", [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp8_e5m2"), ("mxfp6_e3m2", "mxfp6_e3m2")])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_margins_survive_every_route(fa, fb, out_dtype):
    lib = _hip.load()
    osz = torch.empty(0, dtype=out_dtype).element_size()
    for M, N, K, off, route in CASES:
        g = torch.Generator().manual_seed(M * 1000 + N + K)
        ra, rb = G.scale_windows(K, fa, fb)
        G.assert_exact_class(K, fa, fb, ra, rb)
        ops = G.exact_operand(g, M, K, fa, ra) + G.exact_operand(g, N, K, fb, rb)
        bias = torch.randint(-16, 16, (N,), generator=g).float()
        guarded = []
        for t in ops:
            raw, body = _guarded(t.numel(), off)
            body.copy_(t.reshape(-1).to(DEV))
            guarded.append((raw, body, t.numel(), off))
        braw, bbody = _guarded(N * 4)
        bbody.copy_(bias.view(torch.uint8).to(DEV))
        yoff = osz if off else 0                                                # y needs its element's alignment, nothing more
        yraw, ybody = _guarded(M * N * osz, yoff)
        a = _hip.MxMatmulArgs()
        a.struct_size = ctypes.sizeof(a)
        a.a_format, a.b_format = _hip.MX_FORMATS.index(fa), _hip.MX_FORMATS.index(fb)
        a.a_codes, a.a_scales, a.b_codes, a.b_scales = (b.data_ptr() for _, b, _, _ in guarded)
        a.bias, a.y, a.ydt = bbody.data_ptr(), ybody.data_ptr(), _hip._DT[out_dtype]
        a.M, a.N, a.K = M, N, K
        a.stream = _hip._stream(ybody)
        what = (fa, fb, out_dtype, M, N, K, off)
        assert lib.qs_mx_matmul_route(ctypes.byref(a)) == route, what
        assert lib.qs_mx_matmul_v(ctypes.byref(a)) == 0, what
        torch.cuda.synchronize()
        assert _intact(yraw, M * N * osz, yoff), ("y", what)
        for name, (raw, body, n, o), t in zip(("a_codes", "a_scales", "b_codes", "b_scales"), guarded, ops):
            assert _intact(raw, n, o) and torch.equal(body.cpu(), t.reshape(-1)), (name, what)
        assert _intact(braw, N * 4), ("bias", what)
        want = G.reference(*ops[:2], fa, *ops[2:], fb, bias, out_dtype)[0]
        assert G.same(ybody.clone().view(out_dtype).view(M, N), want), what
