"""Out-of-bounds check for the MX products that write MX codes, in the manner of tests/test_mx_gemm_canary_gpu.py: ``out_codes`` and
``out_scales`` are carved out of larger allocations whose margins hold a byte pattern (tests/mx_guard.py); after the launch not a byte
outside ``M * N`` / ``M * ceil(N / 32)`` may have changed, and the bodies equal the composition.  N = 33: a short last block of one
column, single-byte code stores; a base offset of 0 and of 1 byte."""
import pytest
import torch

import mx_codes_out_ref as R
from mx_guard import guarded, intact
from qsparse_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FX, FW, OUT = "mxfp8_e4m3", "mxfp6_e2m3", "mxfp4_e2m1"


def _outputs(rows, N, off):
    nb = (N + 31) // 32
    craw, cbody = guarded(rows * N, off)
    sraw, sbody = guarded(rows * nb, off)
    return (craw, rows * N), (sraw, rows * nb), (cbody, sbody)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("act", [None, "relu"])
def test_gemm_writes_nothing_outside_its_outputs(off, act):
    M, N, K = 5, 33, 200
    g = torch.Generator().manual_seed(off)
    ops = R.operand(g, (M, K), FX, DEV) + (FX,) + R.operand(g, (N, K), FW, DEV) + (FW,)
    bias = torch.randn(N, generator=g).to(DEV)
    codes, scales, out = _outputs(M, N, off)
    got = _hip.mx_matmul_q(*ops, bias, OUT, act, out=out)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out[0].data_ptr() and got[0].data_ptr() % 4 == off
    for name, (raw, n) in (("out_codes", codes), ("out_scales", scales)):
        assert intact(raw, n, off), (name, off, act)
    want = R.matmul_composition(*ops, bias, OUT, act)
    assert torch.equal(out[0].view(M, N), want[0]) and torch.equal(out[1].view(M, 2), want[1])


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("act", [None, "relu"])
def test_conv_writes_nothing_outside_its_outputs(off, act):
    C, Cout, geo = 5, 33, ((2, 2), (1, 1), (1, 2))
    g = torch.Generator().manual_seed(10 + off)
    ops = R.operand(g, (2, 13, 11, C), FX, DEV) + (FX,) + R.operand(g, (Cout, 3, 3, C), FW, DEV) + (FW,)
    bias = torch.randn(Cout, generator=g).to(DEV)
    rows = 2 * 7 * 5
    codes, scales, out = _outputs(rows, Cout, off)
    _hip.mx_conv2d_q(*ops, bias, *geo, OUT, act, out=out)
    torch.cuda.synchronize()
    assert _hip.mx_conv_q_last_route == _hip.MX_CONV_ROUTE_PLAIN
    for name, (raw, n) in (("out_codes", codes), ("out_scales", scales)):
        assert intact(raw, n, off), (name, off, act)
    want = R.conv_composition(*ops, bias, *geo, OUT, act)
    assert torch.equal(out[0].view(want[0].shape), want[0]) and torch.equal(out[1].view(want[1].shape), want[1])
