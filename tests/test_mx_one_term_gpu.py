"""One-term products through the three kernels on MX codes (qs_mx_matmul_v, qs_mx_matmul_splitk_v, qs_mx_conv2d_v): every row of
either operand holds a single code that may be nonzero, all at one column k0, so y[m, n] = val_a 2^(sa - 127) val_b 2^(sb - 127) with
no summation and the float64 reference of tests/mx_gemm_ref.py is exact.  The rows run over EVERY valid code of the format -- the top
binades and the subnormals included, which the exact class of the other tests leaves out -- crossed with scale bytes over the whole
E8M0 range (0, 1, 64, 126, 127, 128, 190, 253, 254); the blocks that hold only zero codes carry random scale bytes, which must not
matter.  Outputs whose exact value is zero or has a magnitude in [2^-126, 2^128) -- at least 65 % for every format pair -- must be
the float64 value cast once, bit for bit, in the three output dtypes (fp16 / bf16 subnormals, overflow to Inf and ties included).
Outside that range the outputs are pinned to what was measured on the MI355X (mx_gemm_ref.OneTerm.expected): gradual underflow,
a float32 sum of +0 for whatever rounds to zero in float32, Inf of the right sign -- the same for all 25 pairs.  The two-byte
outputs are the cast of that float32 sum, which keeps the sign: a negative sum too small for fp16 / bf16 is -0."""
import pytest
import torch

import mx_conv_ref as R
import mx_gemm_ref as G
from qsparse_amd import _hip
from qsparse_amd.mx_conv import mx_conv2d
from qsparse_amd.mx_gemm import mx_matmul

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
PAIRS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp6_e2m3", "mxfp8_e5m2"), ("mxfp8_e4m3", "mxfp4_e2m1"),
         ("mxfp6_e3m2", "mxfp8_e4m3")]
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# (K, k0): K = 128 is the 16-bytes-per-load kernel -- k0 in the first and the last lane group and in both halves of an FP8 fragment
# (k0 = 37: registers 0..3 of lane group 2, k0 = 127: registers 4..7 of lane group 3); K = 127 is the byte-load kernel
WHERE = [(128, 0, _hip.MX_GEMM_ROUTE_VEC), (128, 37, _hip.MX_GEMM_ROUTE_VEC), (128, 127, _hip.MX_GEMM_ROUTE_VEC),
         (127, 0, _hip.MX_GEMM_ROUTE_PLAIN), (127, 70, _hip.MX_GEMM_ROUTE_PLAIN), (127, 126, _hip.MX_GEMM_ROUTE_PLAIN)]


def biases(g, N):
    """no bias; +0.0 and -0.0 mixed at random: round(acc + bias) must hold for the sign of a zero too"""
    return (None, torch.where(torch.rand(N, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0)))


class Wants:
    """the expected outputs of one format pair on the device, computed once: they depend on neither K, k0 nor the kernel"""

    def __init__(self, fa, fb, bias_list):
        self.va = G.one_term_operand(torch.Generator().manual_seed(0), fa, 32, 0)[2]
        self.vb = G.one_term_operand(torch.Generator().manual_seed(0), fb, 32, 0)[2]
        self.ref = G.OneTerm(self.va, self.vb)
        assert self.ref.strict.float().mean() >= 0.65, (fa, fb, float(self.ref.strict.float().mean()))
        self.strict = self.ref.strict.to(DEV)
        by = {(i, dt): self.ref.expected(b, dt) for i, b in enumerate(bias_list) for dt in DTYPES}
        for (i, dt), (_, measured) in by.items():    # -0: never in float32 (+0 + -0 = +0), but the cast to fp16 keeps a small sum's sign
            neg0 = int(((measured == 0) & torch.signbit(measured)).sum())
            assert neg0 == 0 if dt == torch.float32 else neg0 > 0 or dt == torch.bfloat16, (fa, fb, i, dt, neg0)
        self.by = {k: tuple(t.to(DEV) for t in v) for k, v in by.items()}

    def check(self, y, i, dt, what):
        (strict_want, measured), strict = self.by[i, dt], self.strict
        assert y.dtype == dt and y.shape == measured.shape, what
        ok = G.bits_equal(y, strict_want)
        assert bool(ok[strict].all()), ("strict class", what, int((~ok & strict).sum()))
        assert not bool(y[~strict].isnan().any()), ("NaN outside float32's range", what)
        ok = G.bits_equal(y, measured)
        assert bool(ok.all()), ("outside float32's range", what, int((~ok).sum()))


@pytest.mark.parametrize("fa,fb", ALL_PAIRS)
def test_matmul_every_code_and_the_whole_scale_range(fa, fb):
    g = torch.Generator().manual_seed(1200 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    N = len(G.valid_codes(fb)) * len(G.ONE_TERM_SCALES)
    bl = biases(g, N)
    wants = Wants(fa, fb, bl)
    for K, k0, route in WHERE:
        ac, asc, va = G.one_term_operand(g, fa, K, k0)
        bc, bsc, vb = G.one_term_operand(g, fb, K, k0)
        assert torch.equal(va, wants.va) and torch.equal(vb, wants.vb)
        dev = (ac.to(DEV), asc.to(DEV), bc.to(DEV), bsc.to(DEV))
        for i, b in enumerate(bl):
            for dt in DTYPES:
                y = mx_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, None if b is None else b.to(DEV), dt)
                assert _hip.mx_gemm_last_route == route and _hip.mx_gemm_last_split == 1
                wants.check(y, i, dt, (fa, fb, K, k0, dt, b is not None))


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_split_k_with_an_all_zero_slice(fa, fb):
    """K = 256 in two slices, the term in slice 1: slice 0 holds zero codes under random scale bytes and its partial is +0 -- the
    sum of the partials is the unsplit result, bit for bit, over the whole range (Inf and subnormal partials included)"""
    g = torch.Generator().manual_seed(1300 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    N = len(G.valid_codes(fb)) * len(G.ONE_TERM_SCALES)
    bl = biases(g, N)
    wants = Wants(fa, fb, bl)
    ac, asc, _ = G.one_term_operand(g, fa, 256, 128 + 37)
    bc, bsc, _ = G.one_term_operand(g, fb, 256, 128 + 37)
    dev = (ac.to(DEV), asc.to(DEV), bc.to(DEV), bsc.to(DEV))
    for i, b in enumerate(bl):
        for dt in DTYPES:
            bd = None if b is None else b.to(DEV)
            y = mx_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, bd, dt, split_k=2)
            assert _hip.mx_gemm_last_route == _hip.MX_GEMM_ROUTE_VEC and _hip.mx_gemm_last_split == 2
            one = mx_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, bd, dt)
            assert _hip.mx_gemm_last_route == _hip.MX_GEMM_ROUTE_VEC and _hip.mx_gemm_last_split == 1
            assert bool(G.bits_equal(y, one).all()), (fa, fb, dt, b is not None)
            wants.check(y, i, dt, (fa, fb, "split", dt, b is not None))


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_conv_3x3_on_a_3x3_image(fx, fw):
    """the same operands as a 3x3 convolution with C = 32 on 3x3 images without padding: one output pixel per image (M = B, K' =
    288), the term at tap (2, 1), channel 5"""
    g = torch.Generator().manual_seed(1400 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    Cout = len(G.valid_codes(fw)) * len(G.ONE_TERM_SCALES)
    bl = biases(g, Cout)
    wants = Wants(fx, fw, bl)
    k0 = (2 * 3 + 1) * 32 + 5
    xc, xs, _ = G.one_term_operand(g, fx, 288, k0)
    wc, ws, _ = G.one_term_operand(g, fw, 288, k0)
    ops = tuple(t.to(DEV) for t in (xc.view(-1, 3, 3, 32), xs.view(-1, 3, 3, 1), wc.view(-1, 3, 3, 32), ws.view(-1, 3, 3, 1)))
    assert int(ops[0][:, 2, 1, 5].count_nonzero()) > 0 and int(ops[0].count_nonzero()) == int(ops[0][:, 2, 1, 5].count_nonzero())
    A, SA, Wp, SWp = R.im2col_codes(*ops, 3, 3)
    assert torch.equal(A.cpu(), xc) and torch.equal(SWp.cpu(), ws)
    for i, b in enumerate(bl):
        for dt in DTYPES:
            bd = None if b is None else b.to(DEV)
            y = mx_conv2d(ops[0], ops[1], fx, ops[2], ops[3], fw, bd, 1, 0, 1, dt)
            assert _hip.mx_conv_last_route == _hip.MX_CONV_ROUTE_VEC and y.shape == (xc.shape[0], 1, 1, Cout)
            y = y.view(-1, Cout)
            want = mx_matmul(A, SA, fx, Wp, SWp, fw, bd, dt)
            assert _hip.mx_gemm_last_route == _hip.MX_GEMM_ROUTE_VEC and _hip.mx_gemm_last_split == 1
            assert bool(G.bits_equal(y, want).all()), (fx, fw, dt, b is not None)
            wants.check(y, i, dt, (fx, fw, "conv", dt, b is not None))
