"""The CPU twin of tests/test_mx_one_term_gpu.py: the one-term construction -- every valid code crossed with scale bytes over the
whole E8M0 range -- through the CPU paths of mx_matmul and mx_conv2d, on the strict class (exact value zero or of a magnitude in
[2^-126, 2^128)).  It proves the construction and its float64 reference without a GPU."""
import pytest
import torch

import mx_gemm_ref as G
from qsparse_amd.mx_conv import mx_conv2d
from qsparse_amd.mx_gemm import mx_matmul

ALL_PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
PAIRS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp6_e2m3", "mxfp8_e5m2"), ("mxfp8_e4m3", "mxfp4_e2m1"),
         ("mxfp6_e3m2", "mxfp8_e4m3")]
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
COUNTS = {"mxfp8_e4m3": 254, "mxfp8_e5m2": 248, "mxfp6_e2m3": 64, "mxfp6_e3m2": 64, "mxfp4_e2m1": 16}


def signed_zeros(g, N):
    return torch.where(torch.rand(N, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))


def test_the_rows_are_every_valid_code_times_nine_scale_bytes():
    g = torch.Generator().manual_seed(0)
    for fmt, n in COUNTS.items():
        codes, scales, val = G.one_term_operand(g, fmt, 127, 70)
        assert len(G.valid_codes(fmt)) == n and codes.shape == (9 * n, 127) and scales.shape == (9 * n, 4) and not val.isnan().any()
        assert int(codes.count_nonzero()) == int(codes[:, 70].count_nonzero()) == 9 * (n - 1)         # all but the zero byte
        assert sorted(set(scales[:, 2].tolist())) == sorted(G.ONE_TERM_SCALES) and int(scales.max()) < 255
        assert torch.equal(val, G.values(codes, scales, fmt)[:, 70]) and float(val.abs().max()) == float(G.table(fmt).nan_to_num().max()) * 2.0 ** 127


@pytest.mark.parametrize("fa,fb", ALL_PAIRS)
def test_matmul_cpu_path_on_the_strict_class(fa, fb):
    g = torch.Generator().manual_seed(1200 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    ref = None
    for K, k0, with_bias in ((128, 37, False), (127, 126, True)):
        ac, asc, va = G.one_term_operand(g, fa, K, k0)
        bc, bsc, vb = G.one_term_operand(g, fb, K, k0)
        if ref is None:                # the values of the rows depend on neither K nor k0
            ref = G.OneTerm(va, vb)
            assert ref.strict.float().mean() >= 0.65
        assert torch.equal(ref.p, G.OneTerm(va, vb).p)
        bias = signed_zeros(g, len(vb)) if with_bias else None
        for dt in DTYPES if (fa, fb) in PAIRS and with_bias else (torch.float32,):
            want = ref.expected(bias, dt)[0]
            y = mx_matmul(ac, asc, fa, bc, bsc, fb, bias, dt)
            assert y.dtype == dt and bool(G.bits_equal(y, want)[ref.strict].all()), (fa, fb, K, dt)
        if len(va) * len(vb) < 10 ** 6:    # the float64 sum of the definition, zeros and all, says the same as the one product
            y64 = G.reference(ac, asc, fa, bc, bsc, fb, bias)[0]
            assert bool(G.bits_equal(y64, ref.expected(bias, torch.float32)[0])[ref.strict].all()), (fa, fb, K)


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_conv_cpu_path_on_the_strict_class(fx, fw):
    g = torch.Generator().manual_seed(1400 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    k0 = (2 * 3 + 1) * 32 + 5
    xc, xs, vx = G.one_term_operand(g, fx, 288, k0)
    wc, ws, vw = G.one_term_operand(g, fw, 288, k0)
    ref = G.OneTerm(vx, vw)
    for bias, dt in ((None, torch.float32), (signed_zeros(g, len(vw)), torch.float16), (None, torch.bfloat16)):
        want = ref.expected(bias, dt)[0]
        y = mx_conv2d(xc.view(-1, 3, 3, 32), xs.view(-1, 3, 3, 1), fx, wc.view(-1, 3, 3, 32), ws.view(-1, 3, 3, 1), fw, bias, 1, 0, 1, dt)
        assert y.shape == (len(vx), 1, 1, len(vw)) and bool(G.bits_equal(y.view(len(vx), -1), want)[ref.strict].all()), (fx, fw, dt)
