"""The MX products that write MX codes on the GPU (``qs_mx_matmul_q_v``, ``qs_mx_conv2d_q_v``): codes and scale bytes are BIT-IDENTICAL to
the composition they replace -- the float32 kernel, the activation, ``quantize_with_mx`` along the last axis, all on the GPU at the same
commit.  No tolerance anywhere.  Shapes are the smallest that reach each edge of the 128 x 128 tile, the 64 x 64 corner of a wave, the
block of 32 and the 4-code store."""
import pytest
import torch

import mx_codes_out_ref as R
import mx_conv_ref as CR
from qsparse_amd import _hip
from qsparse_amd.mx_conv import mx_conv2d
from qsparse_amd.mx_gemm import MXActivation, mx_matmul
from qsparse_amd.quantize import quantize_with_mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (17, 31), (16, 32), (5, 33), (65, 65), (129, 130), (130, 257)]
PAIRS = [(fa, fb) for fa in R.FORMATS for fb in R.FORMATS]
OPTIONS = [(False, None), (True, None), (False, "relu"), (True, "relu")]       # bias, act
_cache = {}


def _off1(t):
    """the same bytes one byte off the allocation's alignment: takes the predicated-byte-load kernel whatever K is"""
    raw = torch.empty(t.numel() + 1, dtype=torch.uint8, device=t.device)
    raw[1:].copy_(t.reshape(-1))
    return raw[1:].view(t.shape)


def _operands(M, N, K, fmt_a, fmt_b, off):
    """quantized seeded randn with a wide per-row scale, computed once per (shape, format) and left unchanged"""
    key = (M, N, K, fmt_a, fmt_b, off)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
        ac, asc = R.operand(g, (M, K), fmt_a, DEV)
        bc, bsc = R.operand(g, (N, K), fmt_b, DEV)
        bias = (torch.randn(N, generator=g) * 4).to(DEV)
        _cache[key] = ((_off1(ac) if off else ac), asc, fmt_a, bc, bsc, fmt_b), bias
    return _cache[key]


def _check(ops, bias, out_fmt, act, route, what):
    got = mx_matmul(*ops, bias, out_fmt=out_fmt, act=act)
    assert _hip.mx_gemm_q_last_route == route, what
    want = R.matmul_composition(*ops, bias, out_fmt, act)
    assert _hip.mx_gemm_last_route == route, what                   # the float kernel took the same route
    assert R.same(got, want), what


# K = 128 with 16-byte aligned bases is the 16-byte-load kernel by the route's rule (K % 16 == 0); it is put on the byte-load kernel
# by a code base one byte off, so that the list covers PLAIN at 1, 128 (one whole step), 200 (a short last block) and VEC at 256
KS = [(1, False, _hip.MX_GEMM_ROUTE_PLAIN), (128, True, _hip.MX_GEMM_ROUTE_PLAIN), (200, False, _hip.MX_GEMM_ROUTE_PLAIN),
      (256, False, _hip.MX_GEMM_ROUTE_VEC)]


@pytest.mark.parametrize("K,off,route", [KS[2], KS[3]])
def test_every_pair_and_output_format(K, off, route):
    """all 25 input pairs x 5 output formats x bias / act on and off at (129, 130): two tiles each way, a short last block, N % 4 != 0"""
    M, N = 129, 130
    for fa, fb in PAIRS:
        ops, bias = _operands(M, N, K, fa, fb, off)
        for out_fmt in R.FORMATS:
            for use_bias, act in OPTIONS:
                _check(ops, bias if use_bias else None, out_fmt, act, route, (fa, fb, out_fmt, use_bias, act, K))


@pytest.mark.parametrize("K,off,route", KS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_shapes_routes_bias_and_act(M, N, K, off, route):
    """every shape x K with bias / act on and off; input pairs and output formats are sampled round robin"""
    n = SHAPES.index((M, N)) * 7 + K
    for use_bias, act in OPTIONS:
        for _ in range(2):
            (fa, fb), out_fmt = PAIRS[n % 25], R.FORMATS[(n // 3) % 5]
            n += 11
            ops, bias = _operands(M, N, K, fa, fb, off)
            _check(ops, bias if use_bias else None, out_fmt, act, route, (M, N, K, fa, fb, out_fmt, use_bias, act))


@pytest.mark.parametrize("N", [64, 66])                              # the 4-code store and the single-byte one
def test_leading_dimensions_and_n_mod_4(N):
    g = torch.Generator().manual_seed(N)
    ac, asc = R.operand(g, (2, 3, 96), "mxfp8_e4m3", DEV)
    bc, bsc = R.operand(g, (N, 96), "mxfp4_e2m1", DEV)
    got = mx_matmul(ac, asc, "mxfp8_e4m3", bc, bsc, "mxfp4_e2m1", out_fmt="mxfp6_e3m2", act="relu")
    assert got[0].shape == (2, 3, N) and got[1].shape == (2, 3, (N + 31) // 32)
    assert R.same(got, R.matmul_composition(ac, asc, "mxfp8_e4m3", bc, bsc, "mxfp4_e2m1", None, "mxfp6_e3m2", "relu"))
    empty = mx_matmul(ac[:0], asc[:0], "mxfp8_e4m3", bc, bsc, "mxfp4_e2m1", out_fmt="mxfp6_e3m2")
    assert empty[0].shape == (0, 3, N) and _hip.mx_gemm_q_last_route is None


@pytest.mark.parametrize("out_fmt", R.FORMATS)
def test_special_values(out_fmt):
    """what the quantizer does with zero, NaN / Inf and subnormal blocks, reached from inside the product; each also by identity"""
    M, N, K = 5, 70, 64
    fa = fb = "mxfp8_e4m3"
    g = torch.Generator().manual_seed(7)
    ac, asc = R.operand(g, (M, K), fa, DEV, 2)
    bc, bsc = R.operand(g, (N, K), fb, DEV, 2)
    bias = torch.randn(N, generator=g).to(DEV)

    def run(ac, asc, bc, bsc, bias, act):
        got = mx_matmul(ac, asc, fa, bc, bsc, fb, bias, out_fmt=out_fmt, act=act)
        assert R.same(got, R.matmul_composition(ac, asc, fa, bc, bsc, fb, bias, out_fmt, act)), (out_fmt, act)
        return got

    for act in (None, "relu"):
        zc = ac.clone()
        zc[2] = 0                                                   # an all-zero row of A: all-zero blocks, scale byte 0
        codes, scales = run(zc, asc, bc, bsc, None, act)
        assert not scales[2].any() and not codes[2].any() and scales[1].any()
        ib = bias.clone()
        ib[40] = float("inf")                                       # +Inf in one column: block 1 of every row, its neighbours untouched
        codes, scales = run(ac, asc, bc, bsc, ib, act)
        plain = run(ac, asc, bc, bsc, bias, act)
        assert (scales[:, 1] == 255).all() and not codes[:, 32:64].any()
        assert torch.equal(scales[:, [0, 2]], plain[1][:, [0, 2]]) and torch.equal(codes[:, :32], plain[0][:, :32])
        assert torch.equal(codes[:, 64:], plain[0][:, 64:])
        ns = asc.clone()
        ns[3, 1] = 255                                              # a 0xFF input scale byte: a NaN row, with and without the ReLU
        codes, scales = run(ac, ns, bc, bsc, bias, act)
        assert (scales[3] == 255).all() and not codes[3].any() and (scales[2] != 255).all()
        codes, scales = run(ac, torch.full_like(asc, 254), bc, torch.full_like(bsc, 254), None, act)     # overflow to Inf in the sum
        assert (scales == 255).any()
        codes, scales = run(ac, torch.zeros_like(asc), bc, torch.zeros_like(bsc), None, act)             # 2^-254: every sum rounds to zero
        assert not scales.any() and not codes.any()
        # 2^-146 times sums of about 2^17: float32-subnormal sums around 2^-129, which the byte 0 (2^-127) leaves above every
        # format's smallest subnormal but FP4's
        codes, scales = run(ac, torch.zeros_like(asc), bc, torch.full_like(bsc, 108), None, act)
        assert not scales.any() and (codes.any() or out_fmt == "mxfp4_e2m1")
    neg = torch.full((N,), -1e6, device=DEV)                        # every sum negative
    codes, scales = run(ac, asc, bc, bsc, neg, "relu")
    assert not codes.any() and not scales.any()
    codes, scales = run(ac, asc, bc, bsc, neg, None)
    sign = {"mxfp8_e4m3": 7, "mxfp8_e5m2": 7, "mxfp6_e2m3": 5, "mxfp6_e3m2": 5, "mxfp4_e2m1": 3}[out_fmt]
    assert ((codes >> sign) == 1).all()


@pytest.mark.parametrize("out_fmt", R.FORMATS)
def test_inf_code_in_a_row_with_a_short_last_block(out_fmt):
    """an E5M2 Inf code in a row of A, N = 33: the columns past N of the last block are Inf times zero codes in the accumulator, and
    must not reach the block's maximum -- the one real column of that block is -Inf, which the ReLU makes +0"""
    M, N, K = 5, 33, 64
    fa, fb = "mxfp8_e5m2", "mxfp8_e4m3"
    g = torch.Generator().manual_seed(33)
    ac, asc = R.operand(g, (M, K), fa, DEV, 2)
    bc, bsc = R.operand(g, (N, K), fb, DEV, 2)
    ac, bc = ac.clone(), bc.clone()
    ac[1, 7] = 0x7C                                                  # +Inf in E5M2
    bc[32, 7] = 0xB8                                                 # -1.0 in E4M3: column 32 of row 1 sums to -Inf
    for act in (None, "relu"):
        for bias in (None, torch.randn(N, generator=g).to(DEV)):
            got = mx_matmul(ac, asc, fa, bc, bsc, fb, bias, out_fmt=out_fmt, act=act)
            assert R.same(got, R.matmul_composition(ac, asc, fa, bc, bsc, fb, bias, out_fmt, act)), (out_fmt, act, bias is not None)
    y = mx_matmul(ac, asc, fa, bc, bsc, fb)
    if bool(torch.isneginf(y[1, 32])):                               # (the value of a code the quantizer never writes is unspecified)
        codes, scales = mx_matmul(ac, asc, fa, bc, bsc, fb, out_fmt=out_fmt, act="relu")
        assert scales[1, 1] == 0 and codes[1, 32] == 0 and scales[1, 0] == 255


GEO = (2, 1, (1, 2))                                                 # stride, padding, dilation


@pytest.mark.parametrize("C,Cout,route", [(5, 33, _hip.MX_CONV_ROUTE_PLAIN), (48, 130, _hip.MX_CONV_ROUTE_VEC), (32, 64, _hip.MX_CONV_ROUTE_VEC)])
def test_conv_is_the_composition_and_the_gemm_on_im2col(C, Cout, route):
    g = torch.Generator().manual_seed(C)
    bias = torch.randn(Cout, generator=g).to(DEV)
    n = C
    for fx, fw in (("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp6_e2m3"), ("mxfp6_e3m2", "mxfp8_e5m2"), ("mxfp4_e2m1", "mxfp4_e2m1")):
        xc, xs = R.operand(g, (2, 13, 11, C), fx, DEV)
        wc, ws = R.operand(g, (Cout, 3, 3, C), fw, DEV)
        A, SA, Wp, SWp = CR.im2col_codes(xc, xs, wc, ws, 3, 3, *GEO)
        for use_bias, act in OPTIONS:
            out_fmt = R.FORMATS[n % 5]
            n += 1
            b = bias if use_bias else None
            got = mx_conv2d(xc, xs, fx, wc, ws, fw, b, *GEO, out_fmt=out_fmt, act=act)
            what = (C, Cout, fx, fw, out_fmt, use_bias, act)
            assert _hip.mx_conv_q_last_route == route, what
            assert got[0].shape == (2, 7, 5, Cout) and got[1].shape == (2, 7, 5, (Cout + 31) // 32), what
            assert R.same(got, R.conv_composition(xc, xs, fx, wc, ws, fw, b, *GEO, out_fmt, act)), what
            gemm = mx_matmul(A, SA, fx, Wp, SWp, fw, b, out_fmt=out_fmt, act=act)
            assert torch.equal(got[0].reshape(-1, Cout), gemm[0]) and torch.equal(got[1].reshape(gemm[1].shape), gemm[1]), what


def test_conv_1x1_is_forwarded_to_the_gemm():
    g = torch.Generator().manual_seed(11)
    xc, xs = R.operand(g, (2, 13, 11, 32), "mxfp8_e4m3", DEV)
    wc, ws = R.operand(g, (64, 1, 1, 32), "mxfp6_e2m3", DEV)
    bias = torch.randn(64, generator=g).to(DEV)
    for out_fmt, act in (("mxfp4_e2m1", "relu"), ("mxfp8_e5m2", None)):
        got = mx_conv2d(xc, xs, "mxfp8_e4m3", wc, ws, "mxfp6_e2m3", bias, out_fmt=out_fmt, act=act)
        assert _hip.mx_conv_q_last_route == _hip.MX_CONV_ROUTE_GEMM
        assert R.same(got, R.conv_composition(xc, xs, "mxfp8_e4m3", wc, ws, "mxfp6_e2m3", bias, 1, 0, 1, out_fmt, act))
        gemm = mx_matmul(xc.view(-1, 32), xs.view(-1, 1), "mxfp8_e4m3", wc.view(64, 32), ws.view(64, 1), "mxfp6_e2m3", bias, out_fmt=out_fmt, act=act)
        assert torch.equal(got[0].view(-1, 64), gemm[0]) and torch.equal(got[1].view(-1, 2), gemm[1])


@pytest.mark.parametrize("chain,channels_last", [(R.linear_chain, False), (R.conv_chain, False), (R.conv_chain, True)])
def test_layer_chain_on_the_gpu(chain, channels_last):
    """no float tensor between the layers, and bit for bit the two layers with a float ReLU between them"""
    fused, plain, second, x = chain(DEV)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    mid = fused[0](x)
    assert isinstance(mid, MXActivation) and mid.codes.is_cuda and mid.codes.dtype == torch.uint8
    want = second(R.relu(plain(x)))
    got = fused(x)
    assert got.dtype == torch.float32 and torch.equal(got, want) and bool(got.isfinite().all())
    deq = mid.dequantize()
    assert deq.shape == plain(x).shape and torch.equal(deq, quantize_with_mx(R.relu(plain(x)), mid.fmt, 1 if x.dim() == 4 else -1))
