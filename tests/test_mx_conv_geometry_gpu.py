"""Geometries of the implicit-GEMM convolution on MX codes (qs_mx_conv2d_v) that the ten CASES of test_mx_conv_gpu.py do not reach:
kernels with KW == 1 or KH == 1 (a carry into kh on every period of the walk along k'), windows that lie wholly in the padding,
strides larger than the kernel (pixels that no window may read), a dilated kernel as large as the padded image, and four tiles along
M with three along N with image boundaries inside tiles.  Every case is checked with test_mx_conv_gpu.check_against_im2col -- bit for
bit against mx_matmul on the host-built im2col operands, with and without bias, in the three dtypes, route asserted -- and the
padding and stride cases also directly, without the im2col operands."""
import pytest
import torch

import mx_conv_ref as R
import mx_gemm_ref as G
import qsparse_amd as qs
from test_mx_conv_gpu import ALL_PAIRS, DEV, DTYPES, PAIRS, PLAIN, VEC, check_against_im2col, conv, quantized_case

pytestmark = pytest.mark.gpu
# B, H, W, C, Cout, (KH, KW), stride, padding, dilation, route
KW_ONE = (2, 7, 9, 32, 20, (5, 1), 1, (2, 0), 1, VEC)                    # Cp = 32: four carries into kh per step
KH_ONE = (2, 7, 9, 16, 20, (1, 5), 1, (0, 2), 1, VEC)                    # Cp = 32, half of every tap is channel padding
KH_ONE_STEM = (2, 7, 9, 3, 20, (1, 7), 1, (0, 3), 1, PLAIN)              # the degenerate kernel on the byte-load route
IN_PADDING = (2, 5, 4, 32, 17, (2, 2), 1, (3, 4), 1, VEC)                # windows wholly in the padding
BIG_STRIDES = [(2, 10, 11, 64, 17, (2, 2), (3, 4), 0, 1, VEC), (2, 10, 11, 40, 17, (2, 2), (3, 4), 0, 1, PLAIN),
               (2, 9, 7, 64, 17, (1, 1), 2, 0, 1, VEC)]                   # (a strided 1x1 is on the VEC route, not the GEMM route)
DILATED_FULL = (2, 9, 9, 32, 17, (3, 3), 1, 1, 5, VEC)                   # the dilated kernel spans 11 = H + 2: OH = OW = 1, M = 2
MANY_TILES = (5, 9, 10, 32, 260, (3, 3), 1, 1, 1, VEC)                   # M = 450: 4 tiles, N = 260: 3; images end at multiples of 90


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def seed(base, fx, fw):
    return torch.Generator().manual_seed(base + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))


@pytest.mark.parametrize("fx,fw", ALL_PAIRS)
def test_kw_one_every_format_pair(fx, fw):
    check_against_im2col(seed(600, fx, fw), KW_ONE, fx, fw)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_kh_one(fx, fw):
    g = seed(700, fx, fw)
    check_against_im2col(g, KH_ONE, fx, fw)
    check_against_im2col(g, KH_ONE_STEM, fx, fw)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_windows_wholly_in_the_padding(fx, fw):
    """besides the im2col check: an output whose window has no tap inside the image is bias[n] rounded to the dtype, +0.0 without
    a bias (sign included)"""
    g = seed(800, fx, fw)
    check_against_im2col(g, IN_PADDING, fx, fw)
    B, H, W, C, Cout, (KH, KW), stride, padding, dilation, route = IN_PADDING
    ops = quantized_case(g, B, H, W, C, Cout, KH, KW, fx, fw)
    empty = R.padding_only(H, W, KH, KW, stride, padding, dilation)
    assert 0 < int(empty.sum()) < empty.numel()
    bias = torch.randn(Cout, generator=g)
    for dt in DTYPES:
        for b in (None, bias):
            y = conv(ops, fx, fw, route, None if b is None else b.to(DEV), stride, padding, dilation, dt).cpu()
            assert y.shape[1:3] == empty.shape
            want = (torch.zeros(Cout) if b is None else b).to(dt).expand(B, int(empty.sum()), Cout)
            assert G.same(y[:, empty], want.contiguous()), (dt, b is not None)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_strides_larger_than_the_kernel_read_no_pixel_between_the_windows(fx, fw):
    """every pixel that no window covers is given the scale byte 0xFF and random codes: y must stay free of NaN and equal, bit for
    bit, what the clean tensor gives"""
    g = seed(900, fx, fw)
    for case in BIG_STRIDES:
        check_against_im2col(g, case, fx, fw)
        B, H, W, C, Cout, (KH, KW), stride, padding, dilation, route = case
        xc, xs, wc, ws = quantized_case(g, B, H, W, C, Cout, KH, KW, fx, fw)
        unread = ~R.pixels_read(H, W, KH, KW, stride, padding, dilation)
        assert 0 < int(unread.sum()) < unread.numel()
        pc, psc = xc.clone(), xs.clone()
        pc[:, unread.to(DEV)] = torch.randint(0, 256, (B, int(unread.sum()), C), generator=g).to(torch.uint8).to(DEV)
        psc[:, unread.to(DEV)] = 255
        bias = torch.randn(Cout, generator=g).to(DEV)
        for dt in DTYPES:
            clean = conv((xc, xs, wc, ws), fx, fw, route, bias, stride, padding, dilation, dt)
            y = conv((pc, psc, wc, ws), fx, fw, route, bias, stride, padding, dilation, dt)
            assert not bool(y.isnan().any()) and G.same(y, clean), (case, dt)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_dilated_kernel_as_large_as_the_padded_image(fx, fw):
    B, H, W, C, Cout, (KH, KW), stride, padding, dilation, route = DILATED_FULL
    assert R.out_size(H, KH, stride, padding, dilation) == 1 and R.out_size(W, KW, stride, padding, dilation) == 1
    check_against_im2col(seed(1000, fx, fw), DILATED_FULL, fx, fw)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_four_tiles_along_m_and_three_along_n(fx, fw):
    g = seed(1100, fx, fw)
    check_against_im2col(g, MANY_TILES, fx, fw)
    check_against_im2col(g, MANY_TILES, fx, fw, (torch.float32,), shift=True)      # the byte-load kernel
