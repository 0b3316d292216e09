"""Convolutions on MX codes over activation tensors of more than 2^31 and more than 2^32 bytes (qs_mx_conv2d_v addresses a piece as
((b H + ih) W + iw) C + c in 64 bits; nothing else in the suite comes near the limits).  A 3x3 convolution with stride 100 reads 59 x
59 (83 x 83) windows of a 5890 x 5890 (8290 x 8290) x 64 image of 2.2 (4.4) GB, the last of them past the 2^31 (2^32) byte mark; a
third case has four images of 1.5 GB, so that the base of the last image, b H W C with b = 3, itself lies past 2^32 (asserted) while
ih and iw stay small -- with three images only the full offset would cross it.  The reference operands are
gathered from the windows that are read alone, by test-owned 64-bit index arithmetic on the device (mx_conv_ref.gather_windows), and
go through mx_matmul: the result must be the same bits.  A 0xFF scale byte on one covered pixel past the mark must turn exactly
that output pixel NaN."""
import pytest
import torch

import mx_conv_ref as R
import mx_gemm_ref as G
from qsparse_amd import _hip
from qsparse_amd.mx_conv import mx_conv2d
from qsparse_amd.mx_gemm import mx_matmul

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, COUT, STRIDE = 64, 17, 100
# B, H = W, the byte offset that a read must exceed
CASES = [(1, 5890, 2 ** 31), (1, 8290, 2 ** 32), (4, 4850, 2 ** 32)]


def fill(B, H, fmt, g):
    """codes [B, H, H, 64] drawn on the device in pieces (FP4: 0..15; E4M3: every byte but the two NaN patterns) and scale bytes
    [B, H, H, 2] in 120..134"""
    codes = torch.empty(B * H * H * C, dtype=torch.uint8, device=DEV)
    step = 2 ** 28
    for i in range(0, codes.numel(), step):
        n = min(step, codes.numel() - i)
        if fmt == "mxfp4_e2m1":
            part = torch.randint(0, 16, (n,), dtype=torch.uint8, device=DEV, generator=g)
        else:
            part = torch.randint(0, 256, (n,), dtype=torch.int16, device=DEV, generator=g).to(torch.uint8)
            part = torch.where((part & 0x7F) == 0x7F, part & 0x80 | 0x38, part)         # 0x7F / 0xFF -> +-1.0
        codes[i:i + n] = part
    del part
    scales = torch.randint(120, 135, (B, H, H, C // 32), dtype=torch.uint8, device=DEV, generator=g)
    return codes.view(B, H, H, C), scales


@pytest.mark.parametrize("fmt", ["mxfp4_e2m1", "mxfp8_e4m3"])
@pytest.mark.parametrize("B,H,mark", CASES)
def test_windows_past_the_byte_marks(B, H, mark, fmt):
    need = B * H * H * C
    assert need > mark
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * need + 2 ** 30:
        pytest.skip(f"needs {(2 * need + 2 ** 30) / 2 ** 30:.0f} GiB of free device memory")
    g = torch.Generator(device=DEV).manual_seed(B * H)
    xc, xs = fill(B, H, fmt, g)
    cpu = torch.Generator().manual_seed(H)
    wc, ws = G.exact_operand(cpu, COUT * 9, C, fmt, 3)
    wc, ws = wc.view(COUT, 3, 3, C).to(DEV), ws.view(COUT, 3, 3, 2).to(DEV)
    bias = torch.randn(COUT, generator=cpu).to(DEV)
    O = R.out_size(H, 3, STRIDE, 1, 1)
    # the 0xFF byte: block 1 of the centre pixel of the last window of the last image -- past the mark, read by that window alone
    ih = iw = (O - 1) * STRIDE
    assert ((((B - 1) * H + ih) * H + iw) * C) > mark and ih < H
    assert B == 1 or (B - 1) * H * H * C > mark                  # several images: the last one's base alone is past the mark
    xs[B - 1, ih, iw, 1] = 255
    A, SA, last = R.gather_windows(xc, xs, 3, 3, STRIDE, 1, 1)
    assert last > mark and A.shape == (B * O * O, 9 * C), (last, mark)
    Wp, SWp = wc.view(COUT, 9 * C), ws.view(COUT, 18)
    for dt, b in ((torch.float32, None), (torch.bfloat16, bias)):
        y = mx_conv2d(xc, xs, fmt, wc, ws, fmt, b, STRIDE, 1, 1, dt)
        assert _hip.mx_conv_last_route == _hip.MX_CONV_ROUTE_VEC and y.shape == (B, O, O, COUT)
        want = mx_matmul(A, SA, fmt, Wp, SWp, fmt, b, dt)
        assert _hip.mx_gemm_last_route == _hip.MX_GEMM_ROUTE_VEC and _hip.mx_gemm_last_split == 1
        assert bool(G.bits_equal(y.view(-1, COUT), want).all()), (B, H, fmt, dt)
        nan = torch.zeros(B, O, O, COUT, dtype=torch.bool, device=DEV)
        nan[B - 1, O - 1, O - 1, :] = True
        assert torch.equal(y.isnan(), nan)
        assert float(y[~nan].float().abs().max()) > 0
