"""The two-way, codes-only MX quantizer on the GPU (qs_mx_quant2_v) against the float64 CPU reference of tests/mx_ref.py, bit for
bit on both pairs: the row pair is ``reference(x, fmt)``, the col pair ``reference(x.t().contiguous(), fmt)``.  The route of every
launch is asserted."""
import pytest
import torch

import mx_ref as R
from qsparse_amd import _hip
from qsparse_amd.mx_gemm import mx_quantize_2way

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMTS = list(R.FORMATS)
VEC, PLAIN = _hip.MX_Q2_ROUTE_TILE_VEC, _hip.MX_Q2_ROUTE_TILE_PLAIN
# the tile is 128 x 64: full tiles, ragged edges in R, in C and in both, single rows and columns
SHAPES = [(128, 64), (256, 192), (130, 64), (128, 70), (16, 8), (48, 40), (144, 200), (33, 31), (1, 1), (1, 300), (300, 1), (129, 65),
          (5, 200), (64, 96), (17, 128), (512, 32)]


def randn(shape, dtype, seed=0, spread=4.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.exp(torch.randn(shape[0], 1, generator=g) * spread)
            * torch.exp(torch.randn(1, shape[1], generator=g) * spread)).to(dtype)


def expected_route(x, row, col):
    R_, C = x.shape
    v = 4 if x.dtype == torch.float32 else 8
    ok = C % v == 0 and x.data_ptr() % 16 == 0 and (not col or R_ % 16 == 0)      # (torch's allocator aligns the outputs)
    return VEC if ok else PLAIN


def check(x_cpu, row_fmt, col_fmt, what="", x_dev=None, route=None):
    xd = x_cpu.to(DEV) if x_dev is None else x_dev
    rc, rs, cc, cs = mx_quantize_2way(xd, row_fmt, col_fmt)
    want = expected_route(xd, row_fmt is not None, col_fmt is not None) if route is None else route
    assert _hip.mx_quant2_last_route == want, (what, x_cpu.shape, _hip.mx_quant2_last_route, want)
    if row_fmt is None:
        assert rc is None and rs is None
    else:
        _, c, s = R.reference(x_cpu, row_fmt, -1)
        assert rc.is_cuda and rc.dtype == torch.uint8 and not rc.requires_grad
        assert R.same(rc, c), (row_fmt, what, tuple(x_cpu.shape), "row codes")
        assert R.same(rs, s), (row_fmt, what, tuple(x_cpu.shape), "row scales")
    if col_fmt is None:
        assert cc is None and cs is None
    else:
        _, c, s = R.reference(x_cpu.t().contiguous(), col_fmt, -1)
        assert R.same(cc, c), (col_fmt, what, tuple(x_cpu.shape), "col codes")
        assert R.same(cs, s), (col_fmt, what, tuple(x_cpu.shape), "col scales")
    return want


def offset_by_one(t):
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() and view.is_contiguous()
    return view


@pytest.mark.parametrize("row_fmt", FMTS)
@pytest.mark.parametrize("col_fmt", FMTS)
def test_every_format_pair(row_fmt, col_fmt):
    for dtype in R.DTYPES:
        assert check(randn((272, 136), dtype, seed=3), row_fmt, col_fmt, "pairs") == VEC


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_every_format_on_every_shape(fmt, dtype):
    routes = set()
    for i, shape in enumerate(SHAPES):
        routes.add(check(randn(shape, dtype, seed=i), fmt, fmt, "shapes"))
    assert routes == {VEC, PLAIN}
    for shape in ((0, 64), (64, 0), (0, 0)):
        rc, rs, cc, cs = mx_quantize_2way(torch.empty(shape, dtype=dtype, device=DEV), fmt, fmt)
        assert _hip.mx_quant2_last_route is None and rc.shape == shape and cc.shape == shape[::-1]
        assert rs.shape == (shape[0], -(-shape[1] // 32)) and cs.shape == (shape[1], -(-shape[0] // 32))


@pytest.mark.parametrize("fmt", FMTS)
def test_row_only_col_only_and_offset_bases(fmt):
    for dtype in R.DTYPES:
        for shape in ((256, 128), (130, 72), (37, 50)):
            x = randn(shape, dtype, seed=9)
            check(x, fmt, None, "row only")
            check(x, None, fmt, "col only")
        # R % 16 != 0 is no obstacle when only the row pair is written
        assert check(randn((130, 72), dtype, seed=1), fmt, None, "row only, ragged R") == VEC
        assert check(randn((130, 72), dtype, seed=1), fmt, fmt, "both, ragged R") == PLAIN
        # a base one element past a 16-byte boundary: the element-access route, also on an aligned shape
        x = randn((256, 128), dtype, seed=2)
        for rf, cf in ((fmt, fmt), (fmt, None), (None, fmt)):
            check(x, rf, cf, "offset base", x_dev=offset_by_one(x), route=PLAIN)
    nc = randn((96, 160), torch.bfloat16, seed=4)
    check(nc.t().contiguous(), fmt, fmt, "non-contiguous input", x_dev=nc.to(DEV).t(), route=VEC)      # one .contiguous(), then the kernel


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_exhaustive_two_byte_patterns(fmt, dtype):
    for x in (R.all_patterns(dtype), R.permuted_finite_patterns(dtype)):
        assert check(x.reshape(-1, 32), fmt, fmt, "exhaustive, blocks along C") == VEC
        assert check(x.reshape(-1, 32).t().contiguous(), fmt, fmt, "exhaustive, blocks along R") == VEC
        assert check(x[:65472].reshape(-1, 31), fmt, fmt, "exhaustive, ragged") == PLAIN


@pytest.mark.parametrize("fmt", FMTS)
def test_ties_clamp_zeros_nonfinite_and_exponent_clamps(fmt):
    eb, mb, bias, emax, top = R.FORMATS[fmt]
    m = R.midpoints(fmt)
    for k in (-126, -60, -3, 0, 7, 100, 118):
        blk = torch.zeros(-(-len(m) // 16) * 16, 32)
        blk[:len(m), 0], blk[:len(m), 1], blk[:len(m), 2] = top, m, -m
        assert check(blk * 2.0 ** k, fmt, fmt, f"ties at 2^{k}") == VEC
        assert check((blk * 2.0 ** k).t().contiguous(), fmt, fmt, f"ties at 2^{k}, along R") == VEC
        assert check((blk * 2.0 ** k)[:len(m), :31].contiguous(), fmt, fmt, f"ties at 2^{k}") == PLAIN
    z = torch.zeros(32, 64)
    z[0, ::2] = -0.0
    z[1, 40:] = -0.0
    z[5:, 3] = -0.0
    check(z, fmt, fmt, "zeros")
    sub = torch.arange(1, 65).float().reshape(2, 32) * 2.0 ** -149
    subs = torch.cat([sub, -sub * 2 ** 10, sub * 2 ** 24, torch.zeros(10, 32)])
    big = torch.cat([torch.full((1, 32), 3.0e38), -torch.arange(1, 33).float().reshape(1, 32) * 1.0e37, randn((14, 32), torch.float32) * 2.0 ** 100])
    for x in (subs, big):
        assert check(x, fmt, fmt, "exponent clamps") == VEC
        assert check(x.t().contiguous(), fmt, fmt, "exponent clamps, along R") == VEC
        check(torch.cat([x, x[:, :1]], 1), fmt, fmt, "exponent clamps, ragged")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_nonfinite_marks_its_block_of_each_direction_and_only_that(fmt, bad):
    for dtype in R.DTYPES:
        for shape, (i, j) in (((160, 96), (70, 40)), ((100, 75), (99, 74)), ((33, 31), (32, 0))):
            x = randn(shape, dtype, seed=6, spread=1.0)
            x[i, j] = bad
            xd = x.to(DEV)
            rc, rs, cc, cs = mx_quantize_2way(xd, fmt, fmt)
            row_ff = torch.zeros(rs.shape, dtype=torch.bool)
            row_ff[i, j // 32] = True
            col_ff = torch.zeros(cs.shape, dtype=torch.bool)
            col_ff[j, i // 32] = True
            assert torch.equal(rs.cpu() == 255, row_ff) and torch.equal(cs.cpu() == 255, col_ff)
            assert not rc[i, j // 32 * 32:j // 32 * 32 + 32].any() and not cc[j, i // 32 * 32:i // 32 * 32 + 32].any()
            check(x, fmt, fmt, f"one {bad}")


def test_large_and_on_a_side_stream():
    x = randn((4096, 768), torch.bfloat16, seed=11, spread=3.0)
    assert check(x, "mxfp8_e4m3", "mxfp8_e5m2", "large") == VEC
    xd = x.to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = mx_quantize_2way(xd, "mxfp4_e2m1", "mxfp6_e2m3")
    s.synchronize()
    assert R.same(out[0], R.reference(x, "mxfp4_e2m1")[1]) and R.same(out[2], R.reference(x.t().contiguous(), "mxfp6_e2m3")[1])
