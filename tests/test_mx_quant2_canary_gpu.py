"""Out-of-bounds check for the two-way MX quantizer, in the manner of tests/test_mx_gemm_canary_gpu.py: x and all four outputs of
every call are carved out of larger allocations whose margins hold a byte pattern; after the launch the margins must be intact,
x unchanged and the outputs equal the CPU reference.  Ragged R and C, single rows and columns and unaligned bases are where a
tiled kernel would reach too far."""
import ctypes

import pytest
import torch

import mx_ref as R
from mx_guard import guarded as _guarded, intact as _intact
from qsparse_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_Q2_ROUTE_TILE_VEC, _hip.MX_Q2_ROUTE_TILE_PLAIN


CASES = [  # R, C, element offset of x's base, byte offset of the output bases, which pairs, expected route
    (128, 64, 0, 0, "both", VEC), (256, 128, 0, 0, "both", VEC), (16, 8, 0, 0, "both", VEC), (144, 200, 0, 0, "both", VEC),
    (1, 8, 0, 0, "row", VEC), (130, 72, 0, 0, "row", VEC), (130, 72, 0, 0, "both", PLAIN), (160, 72, 0, 3, "row", VEC),
    (160, 72, 0, 16, "both", VEC), (160, 72, 0, 3, "both", PLAIN), (160, 72, 0, 3, "col", PLAIN), (128, 64, 1, 0, "both", PLAIN),
    (1, 1, 0, 0, "both", PLAIN), (33, 31, 0, 1, "both", PLAIN), (300, 1, 1, 5, "both", PLAIN), (1, 300, 0, 0, "col", PLAIN),
    (129, 65, 1, 7, "both", PLAIN), (5, 200, 0, 0, "both", PLAIN),
]


@pytest.mark.parametrize("row_fmt,col_fmt", [("mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp4_e2m1", "mxfp6_e2m3"), ("mxfp6_e3m2", "mxfp4_e2m1")])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_margins_survive_every_route(row_fmt, col_fmt, dtype):
    lib = _hip.load()
    esz = torch.empty(0, dtype=dtype).element_size()
    for R_, C, xoff, ooff, pairs, route in CASES:
        g = torch.Generator().manual_seed(R_ * 1000 + C)
        x = (torch.randn(R_, C, generator=g) * torch.exp(torch.randn(R_, 1, generator=g) * 3)).to(dtype)
        xraw, xbody = _guarded(R_ * C * esz, xoff * esz)
        xbody.copy_(x.view(torch.uint8).reshape(-1).to(DEV))
        nbr, nbc = -(-R_ // 32), -(-C // 32)
        sizes = dict(row_codes=R_ * C, row_scales=R_ * nbc, col_codes=C * R_, col_scales=C * nbr)
        given = [n for n in sizes if pairs == "both" or n.startswith(pairs)]
        out = {n: _guarded(sizes[n], ooff) for n in given}
        a = _hip.MxQuant2Args()
        a.struct_size = ctypes.sizeof(a)
        a.row_format, a.col_format = _hip.MX_FORMATS.index(row_fmt), _hip.MX_FORMATS.index(col_fmt)
        a.x, a.xdt = xbody.data_ptr(), _hip._DT[dtype]
        for n in given:
            setattr(a, n, out[n][1].data_ptr())
        a.R, a.C = R_, C
        a.stream = _hip._stream(xbody)
        what = (row_fmt, col_fmt, dtype, R_, C, xoff, ooff, pairs)
        # the documented rule; the table's route is that of the two-byte dtypes (float32 needs C % 4 == 0 only)
        col = "col_codes" in out
        want_route = VEC if (C % (16 // esz) == 0 and xbody.data_ptr() % 16 == 0
                             and (not col or (R_ % 16 == 0 and out["col_codes"][1].data_ptr() % 16 == 0))) else PLAIN
        assert esz == 4 or want_route == route, what
        assert lib.qs_mx_quant2_route(ctypes.byref(a)) == want_route, what
        assert lib.qs_mx_quant2_v(ctypes.byref(a)) == 0, what
        torch.cuda.synchronize()
        assert _intact(xraw, R_ * C * esz, xoff * esz) and torch.equal(xbody.cpu(), x.view(torch.uint8).reshape(-1)), ("x", what)
        for n in given:
            assert _intact(out[n][0], sizes[n], ooff), (n, what)
        if "row_codes" in out:
            _, c, s = R.reference(x, row_fmt, -1)
            assert torch.equal(out["row_codes"][1].cpu().view(R_, C), c) and torch.equal(out["row_scales"][1].cpu().view(R_, nbc), s), what
        if "col_codes" in out:
            _, c, s = R.reference(x.t().contiguous(), col_fmt, -1)
            assert torch.equal(out["col_codes"][1].cpu().view(C, R_), c) and torch.equal(out["col_scales"][1].cpu().view(C, nbr), s), what
