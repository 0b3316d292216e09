"""Out-of-bounds WRITE check for the MX kernels, in the manner of tests/test_canary_gpu.py: y, codes and scales of every call
are carved out of larger allocations whose margins hold a byte pattern; after the launch the margins must be intact and the
bodies equal the CPU reference.  Partial last blocks and unaligned bases are where these kernels would write too far."""
import ctypes
from functools import partial

import pytest
import torch

import mx_ref as R
from mx_guard import guarded, intact
from qsparse_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_guarded, _intact = partial(guarded, pad=256), partial(intact, pad=256)          # bytes on either side


CASES = [  # shape, block dim, byte offset of the bases (in elements of the tensor's dtype), expected route
    ((8, 64), 1, 0, _hip.MX_ROUTE_INNER_VEC), ((3, 4, 96), 2, 0, _hip.MX_ROUTE_INNER_VEC), ((520, 32), 1, 0, _hip.MX_ROUTE_INNER_VEC),
    ((8, 64), 1, 1, _hip.MX_ROUTE_INNER_PLAIN), ((5, 31), 1, 0, _hip.MX_ROUTE_INNER_PLAIN), ((5, 33), 1, 3, _hip.MX_ROUTE_INNER_PLAIN),
    ((7, 56), 1, 0, _hip.MX_ROUTE_INNER_PLAIN), ((9, 100), 1, 1, _hip.MX_ROUTE_INNER_PLAIN), ((1, 1), 1, 0, _hip.MX_ROUTE_INNER_PLAIN),
    ((4, 3, 7, 7), 1, 0, _hip.MX_ROUTE_STRIDED), ((2, 33, 5), 1, 1, _hip.MX_ROUTE_STRIDED), ((100, 3), 0, 0, _hip.MX_ROUTE_STRIDED),
    ((3, 64, 129), 1, 0, _hip.MX_ROUTE_STRIDED),
]


@pytest.mark.parametrize("fmt", ["mxfp8_e4m3", "mxfp4_e2m1"])
@pytest.mark.parametrize("dtype,out_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.float16, torch.float16)])
def test_margins_survive_every_route(fmt, dtype, out_dtype):
    lib = _hip.load()
    for shape, dim, off, route in CASES:
        g = torch.Generator().manual_seed(len(shape) * 100 + shape[-1])
        x = (torch.randn(shape, generator=g) * 8).to(dtype)
        numel, n = x.numel(), shape[dim]
        outer = int(torch.tensor(shape[:dim]).prod()) if dim else 1
        inner = int(torch.tensor(shape[dim + 1:]).prod()) if dim + 1 < len(shape) else 1
        nb = -(-n // 32)
        isz, osz = x.element_size(), torch.empty(0, dtype=out_dtype).element_size()
        xraw, xbody = _guarded(numel * isz, off * isz)
        xbody.copy_(x.contiguous().view(torch.uint8).reshape(-1).to(DEV))
        yraw, ybody = _guarded(numel * osz, off * osz)
        craw, cbody = _guarded(numel, off)
        sraw, sbody = _guarded(outer * nb * inner, off)
        a = _hip.MxQuantArgs()
        a.struct_size = ctypes.sizeof(a)
        a.format = _hip.MX_FORMATS.index(fmt)
        a.x, a.y, a.codes, a.scales = xbody.data_ptr(), ybody.data_ptr(), cbody.data_ptr(), sbody.data_ptr()
        a.xdt, a.ydt = _hip._DT[dtype], _hip._DT[out_dtype]
        a.outer, a.n, a.inner = outer, n, inner
        a.stream = _hip._stream(xbody)
        assert lib.qs_mx_quant_route(ctypes.byref(a)) == route, (shape, dim, off)
        assert lib.qs_mx_quant_fwd_v(ctypes.byref(a)) == 0
        torch.cuda.synchronize()
        what = (fmt, dtype, shape, dim, off)
        assert _intact(yraw, numel * osz, off * osz), ("y", what)
        assert _intact(craw, numel, off), ("codes", what)
        assert _intact(sraw, outer * nb * inner, off), ("scales", what)
        assert _intact(xraw, numel * isz, off * isz), ("x", what)
        ry, rc, rs = R.reference(x, fmt, dim, out_dtype)
        assert R.same(ybody.clone().view(out_dtype).view(shape), ry), what
        assert R.same(cbody.view(shape), rc) and R.same(sbody.view(rs.shape), rs), what
