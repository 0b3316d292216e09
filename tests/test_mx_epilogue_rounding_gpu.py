"""The one rounding to the output dtype that ends every MX product, bit for bit at full mantissas.  The operands are built so that the
float32 value before the cast is known exactly and carries 24 significant bits chosen by the test (mx_gemm_ref.rounding_targets: the
kept lsb even and odd, the discarded part 0 / ulp / half - ulp / half / half + ulp / all ones, in the lowest, middle, far and top
binades of bfloat16 and float16, the overflow edge and float16's underflow edge, both signs).  METHOD A (mx_gemm_ref.method_a) puts
one power of two into the accumulator and the rest of the mantissa into the bias; METHOD B (method_b) sums up to four signed powers
of two from different blocks of 32, every addition exact.  Every float32 output must be the target's own bits, every bfloat16 /
float16 output those of round_once_bits -- no output is left out: the strict share is asserted to be 1.0.

Covered, by the name of the code that rounds and stores:
  * the written-out epilogue of mx_gemm_kernel (qs_mx_gemm.h), vector (`y_vec`) and scalar store: test_matmul_*
  * mx_gemm_reduce_kernel (qs_mx_gemm_splitk.h) -> mx_store4 with `y_vec` set and clear, `ws_vec` set and clear, as compiled in
    api_mx_gemm_splitk.hip: test_split_k_*; as compiled in api_mx_conv_wgrad.hip: test_conv_weight_grad (B = 256, split_k = 2)
  * mx_epilogue -> mx_store4 with `y_vec` set and clear: mx_bmm (also with `y_vec` clear at N % 4 == 0, from an output base off by one
    element), mx_conv2d, mx_conv_transpose2d, mx_conv2d_input_grad, the unsplit mx_conv2d_weight_grad
  * mx_epilogue_codes (the codes-out entry points): one check that method-A operands give the codes of quantize_with_mx(t)."""
import pytest
import torch

import mx_gemm_ref as G
from qsparse_amd import _hip
from qsparse_amd.mx_bmm import mx_bmm
from qsparse_amd.mx_conv import mx_conv2d
from qsparse_amd.mx_conv_train import mx_conv2d_weight_grad
from qsparse_amd.mx_conv_transpose import mx_conv2d_input_grad, mx_conv_transpose2d
from qsparse_amd.mx_gemm import mx_matmul
from qsparse_amd.quantize import quantize_with_mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN
ALL_PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
PAIRS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp6_e2m3", "mxfp8_e5m2"), ("mxfp8_e4m3", "mxfp4_e2m1"),
         ("mxfp6_e3m2", "mxfp8_e4m3")]
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
M = 130                     # two tiles along M; every (i, j, lane) of a wave's 64 x 64 corner stores rounding cases
ZERO_ROWS = (0, 77, 129)    # rows of A without a term: round(+0 + bias)
TARGETS = {dt: G.rounding_targets(dt) for dt in G.TWO_BYTE}


def seed(base, fa, fb):
    return torch.Generator().manual_seed(base + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))


def to_dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def offset_by_one(t):
    """the same bytes on the device at a base one byte past a 16-byte boundary (a slice of a larger allocation)"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    return view


def widths(t):
    """(N % 4 == 0, that plus 1, 2, 3), each past the number of targets `t`: cycle() then repeats some and leaves none out"""
    base = (len(t) // 4 + 1) * 4
    return base, base + 1, base + 2, base + 3


def cycle(seq, n, shift=0):
    """n entries of the tensor or list `seq`, cyclically from `shift` on"""
    idx = [(i + shift) % len(seq) for i in range(n)]
    return seq[torch.tensor(idx)] if isinstance(seq, torch.Tensor) else [seq[i] for i in idx]


def check(y, want32, dt, what):
    """y is, bit for bit, the float32 values `want32` rounded once to `dt`; every output takes part in the comparison"""
    want = G.expected_rounded(want32, dt).reshape(y.shape)
    strict = G.strict_class(want32)
    assert float(strict.float().mean()) == 1.0, what            # the strict share: nothing is left to a looser comparison
    assert y.dtype == dt, what
    ok = G.bits_equal(y, want.to(DEV)).cpu()
    if not bool(ok[strict.reshape(y.shape)].all()):
        bad = (~ok).reshape(-1).nonzero().reshape(-1)[:6]
        bits = lambda t: [hex(int(v)) for v in (t.reshape(-1)[bad].view(torch.int32 if t.element_size() == 4 else torch.int16).to(torch.int64)
                                                & ((1 << 8 * t.element_size()) - 1))]
        raise AssertionError((what, int((~ok).sum()), "of", ok.numel(), "at", bad.tolist(), "before the cast", bits(want32.contiguous()),
                              "got", bits(y.cpu().contiguous()), "want", bits(want.contiguous())))


def matmul_all_dtypes(dev, fa, fb, bias, want, route, what, split_k=1, slices=1):
    for dt in DTYPES:
        y = mx_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, bias, dt, split_k=split_k)
        assert _hip.mx_gemm_last_route == route and _hip.mx_gemm_last_split == slices, what
        check(y, want, dt, what + (dt,))


# ---- mx_matmul ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fa,fb", ALL_PAIRS)
def test_matmul_one_term_plus_bias_every_pair(fa, fb):
    g = seed(2100, fa, fb)
    for tdt, N, K, k0, route in ((torch.bfloat16, 306, 128, 37, VEC), (torch.float16, 308, 127, 126, PLAIN)):
        ac, asc, bc, bsc, bias, want = G.method_a(g, fa, fb, M, K, k0, G.tile_targets(TARGETS[tdt], N, 5), ZERO_ROWS)
        matmul_all_dtypes(to_dev(ac, asc, bc, bsc), fa, fb, bias.to(DEV), want, route, (fa, fb, tdt, N, K))


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_matmul_one_term_plus_bias_every_store_path(fa, fb):
    """N % 4 = 0 (the vector store) and 1, 2, 3 (the scalar store and the short last group), the targets shifted along N from case to
    case; the 16-byte loads, the byte loads of K = 127 and those of an operand base off by one byte"""
    g = seed(2200, fa, fb)
    for tdt in G.TWO_BYTE:
        T = len(TARGETS[tdt])
        for i, (N, K, k0, off) in enumerate(((320, 128, 0, False), (321, 128, 127, False), (322, 127, 70, False), (323, 127, 0, False),
                                             (320, 127, 126, False), (321, 128, 64, True), (320, 128, 31, True))):
            assert N > T
            ac, asc, bc, bsc, bias, want = G.method_a(g, fa, fb, M, K, k0, G.tile_targets(TARGETS[tdt], N, 3 * i), ZERO_ROWS)
            dev = to_dev(ac, asc, bc, bsc)
            if off:
                dev = (offset_by_one(ac), dev[1], dev[2], dev[3]) if N % 2 else (dev[0], dev[1], offset_by_one(bc), dev[3])
            matmul_all_dtypes(dev, fa, fb, bias.to(DEV), want, VEC if K == 128 and not off else PLAIN, (fa, fb, tdt, N, K, k0, off))


B_LAYOUTS = ((128, (0, 1, 2, 3)), (384, (1, 5, 6, 10)), (256, (0, 3, 4, 7)))     # one step; across the steps of the K loop


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_matmul_sum_of_powers_of_two(fa, fb):
    """method B, no bias: the accumulator itself holds the 24 bits.  K = 128: the four blocks of one instruction; K = 384, 256: blocks
    of different steps"""
    g = seed(2300, fa, fb)
    for tdt in G.TWO_BYTE:
        t, terms, _ = G.method_b_targets(tdt)
        for K, blocks in B_LAYOUTS:
            for n in widths(t)[::3]:                                          # N % 4 == 0 and 3
                dev = to_dev(*G.method_b(g, fa, fb, M, K, blocks, cycle(terms, n, K)))
                matmul_all_dtypes(dev, fa, fb, None, cycle(t, n, K).repeat(M, 1), VEC, (fa, fb, tdt, K, n))


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_split_k_sum_of_powers_of_two(fa, fb):
    """the terms in different slices: mx_gemm_reduce_kernel adds the partial sums (exactly), then -- second half -- a bias that makes the
    last bits, and rounds once.  N both ways: `ws_vec` and `y_vec` set and clear"""
    g = seed(2400, fa, fb)
    for tdt in G.TWO_BYTE:
        for with_bias in (False, True):
            t, terms, bias = G.method_b_targets(tdt, with_bias)
            for K, blocks, split in ((256, (0, 3, 4, 7), 2), (384, (2, 4, 7, 11), 3), (384, (0, 1, 9, 10), 3)):
                for n in widths(t)[:2]:
                    dev = to_dev(*G.method_b(g, fa, fb, M, K, blocks, cycle(terms, n, 7)))
                    matmul_all_dtypes(dev, fa, fb, cycle(bias, n, 7).to(DEV) if with_bias else None, cycle(t, n, 7).repeat(M, 1), VEC,
                                      (fa, fb, tdt, K, n, split, with_bias), split_k=split, slices=split)


# ---- mx_bmm -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fa,fb", PAIRS)
def test_bmm_one_term_plus_a_bias_per_slice(fa, fb):
    """G = 3 with other targets, and so another [N] row of the bias, in every slice; both routes; N both ways; and the scalar store at
    N % 4 == 0, from an output base off by one element"""
    g = seed(2500, fa, fb)
    for tdt in G.TWO_BYTE:
        for N, K, k0, route in ((308, 128, 99, VEC), (310, 127, 33, PLAIN), (309, 128, 5, VEC)):
            cases = [G.method_a(g, fa, fb, M, K, k0, G.tile_targets(TARGETS[tdt], N, 101 * s), ZERO_ROWS) for s in range(3)]
            ac, asc, bc, bsc, bias, want = (torch.stack([c[j] for c in cases]) for j in range(6))
            assert not torch.equal(bias[0], bias[1])
            dev = to_dev(ac, asc, bc, bsc, bias)
            for dt in DTYPES:
                y = mx_bmm(dev[0], dev[1], fa, dev[2], dev[3], fb, dev[4], dt)
                assert _hip.mx_bmm_last_route == route
                check(y, want, dt, (fa, fb, tdt, N, K, dt))
                if N % 4 == 0:
                    flat = torch.zeros(3 * M * N + 8 // y.element_size(), dtype=dt, device=DEV)
                    out = flat[1:1 + 3 * M * N]
                    assert out.data_ptr() % (4 * y.element_size()) != 0
                    z = _hip.mx_bmm(dev[0], dev[1], fa, dev[2], dev[3], fb, dev[4], dt, out=out)
                    assert _hip.mx_bmm_last_route == route
                    check(z, want, dt, (fa, fb, tdt, N, K, dt, "output off by one element"))


# ---- the convolutions -------------------------------------------------------------------------------------------------------------------
MC = 70          # images, one output pixel each: more than one wave's 64 rows


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_conv_3x3_on_a_3x3_image(fx, fw):
    """C = 32, no padding: one output pixel per image, K' = 288 = nine taps of one block each.  Method A with the term at tap (2, 1),
    channel 5; method B with the terms at four different taps; Cout % 4 both ways"""
    g = seed(2600, fx, fw)
    k0 = (2 * 3 + 1) * 32 + 5
    for tdt in G.TWO_BYTE:
        for N in (304, 307):
            xc, xs, wc, ws, bias, want = G.method_a(g, fx, fw, MC, 288, k0, G.tile_targets(TARGETS[tdt], N, N), (3, 69))
            ops = to_dev(xc.view(-1, 3, 3, 32), xs.view(-1, 3, 3, 1), wc.view(-1, 3, 3, 32), ws.view(-1, 3, 3, 1))
            for dt in DTYPES:
                y = mx_conv2d(ops[0], ops[1], fx, ops[2], ops[3], fw, bias.to(DEV), 1, 0, 1, dt)
                assert _hip.mx_conv_last_route == _hip.MX_CONV_ROUTE_VEC and y.shape == (MC, 1, 1, N)
                check(y.view(MC, N), want, dt, (fx, fw, tdt, N, dt, "A"))
        t, terms, _ = G.method_b_targets(tdt)
        for n in widths(t)[::3]:
            xc, xs, wc, ws = G.method_b(g, fx, fw, MC, 288, (0, 3, 4, 8), cycle(terms, n, 9))
            ops = to_dev(xc.view(-1, 3, 3, 32), xs.view(-1, 3, 3, 1), wc.view(-1, 3, 3, 32), ws.view(-1, 3, 3, 1))
            for dt in DTYPES:
                y = mx_conv2d(ops[0], ops[1], fx, ops[2], ops[3], fw, None, 1, 0, 1, dt)
                assert _hip.mx_conv_last_route == _hip.MX_CONV_ROUTE_VEC
                check(y.view(MC, n), cycle(t, n, 9).repeat(MC, 1), dt, (fx, fw, tdt, n, dt, "B"))


@pytest.mark.parametrize("fx,fw", PAIRS[:3])
def test_conv_transpose_one_tap_per_output_pixel(fx, fw):
    """a 1 x 1 image under a 2 x 2 kernel, stride 1: output pixel (oh, ow) reads the tap (oh, ow) of the one input pixel and nothing
    else.  Method A at three taps; the fourth holds zero codes, so its pixel is round(bias)"""
    g = seed(2700, fx, fw)
    for tdt in G.TWO_BYTE:
        for N in (304, 306):
            xc, xs, wc, ws, bias, want = G.method_a(g, fx, fw, MC, 32, 9, G.tile_targets(TARGETS[tdt], N, 17), (5,))
            w4, s4 = wc.view(N, 1, 1, 32).repeat(1, 2, 2, 1), ws.view(N, 1, 1, 1).repeat(1, 2, 2, 1)
            w4[:, 1, 1] = 0
            want4 = want.view(MC, 1, 1, N).repeat(1, 2, 2, 1)
            want4[:, 1, 1] = torch.zeros(N) + bias
            ops = to_dev(xc.view(MC, 1, 1, 32), xs.view(MC, 1, 1, 1), w4, s4)
            for dt in DTYPES:
                y = mx_conv_transpose2d(ops[0], ops[1], fx, ops[2], ops[3], fw, bias.to(DEV), 1, 0, 0, 1, dt)
                assert _hip.mx_conv_transpose_last_route == _hip.MX_CONV_ROUTE_VEC and y.shape == (MC, 2, 2, N)
                check(y, want4, dt, (fx, fw, tdt, N, dt))


@pytest.mark.parametrize("fg,fw", PAIRS[:3])
def test_conv_input_grad_one_tap_per_input_pixel(fg, fw):
    """the input gradient takes no bias: method B along the 128 output channels of the one tap that each pixel of a 2 x 2 input under a
    2 x 2 kernel reads"""
    g = seed(2800, fg, fw)
    for tdt in G.TWO_BYTE:
        t, terms, _ = G.method_b_targets(tdt)
        for n in widths(t)[::2]:
            gc, gs, wc, ws = G.method_b(g, fg, fw, MC, 128, (0, 1, 2, 3), cycle(terms, n, 13))
            ops = to_dev(gc.view(MC, 1, 1, 128), gs.view(MC, 1, 1, 4), wc.view(n, 1, 1, 128).repeat(1, 2, 2, 1), ws.view(n, 1, 1, 4).repeat(1, 2, 2, 1))
            for dt in DTYPES:
                y = mx_conv2d_input_grad(ops[0], ops[1], fg, ops[2], ops[3], fw, (2, 2), 1, 0, 1, dt)
                assert _hip.mx_conv_transpose_last_route == _hip.MX_CONV_ROUTE_VEC and y.shape == (MC, 2, 2, n)
                check(y, cycle(t, n, 13).view(1, 1, 1, n).repeat(MC, 2, 2, 1), dt, (fg, fw, tdt, n, dt))


@pytest.mark.parametrize("fg,fx", PAIRS[:3])
def test_conv_weight_grad(fg, fx):
    """no bias: method B with the terms in different blocks of 32 along the batch.  A 3 x 3 kernel on 3 x 3 images (one output pixel):
    dW [Cout, 3, 3, C] is the product [Cout, Bp] . [9 C, Bp]^T.  B = 128 unsplit (mx_epilogue); B = 256 in two slices: the
    mx_gemm_reduce_kernel that api_mx_conv_wgrad.hip compiles.  9 C % 4 both ways"""
    g = seed(2900, fg, fx)
    Cout = 70
    for tdt in G.TWO_BYTE:
        t, terms, _ = G.method_b_targets(tdt)
        for C in (24, 25):
            n = 9 * C
            assert n > len(t)
            for B, blocks, split in ((128, (0, 1, 2, 3), 1), (256, (1, 2, 5, 6), 2)):
                at = B + C
                gc, gs, xc, xs = G.method_b(g, fg, fx, Cout, B, blocks, cycle(terms, n, at))
                ops = to_dev(gc.view(1, 1, Cout, B), gs.view(1, 1, Cout, -1), xc.view(3, 3, C, B), xs.view(3, 3, C, -1))
                for dt in DTYPES:
                    dw = mx_conv2d_weight_grad(ops[0], ops[1], fg, ops[2], ops[3], fx, (3, 3), 1, 0, 1, dt, split_k=split)
                    assert _hip.mx_conv_wgrad_last_route == _hip.MX_CONV_ROUTE_VEC and _hip.mx_conv_wgrad_last_split == split
                    check(dw.view(Cout, n), cycle(t, n, at).repeat(Cout, 1), dt, (fg, fx, tdt, C, B, split, dt))


# ---- codes out --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_fmt", G.FMTS)
def test_codes_out_quantizes_the_exact_sum(out_fmt):
    """the quantizing epilogue sees the same float32 value: its codes are those of the quantizer on the targets"""
    fa, fb = "mxfp8_e4m3", "mxfp6_e2m3"
    g = seed(3000, fa, fb)
    for tdt, N in ((torch.bfloat16, 320), (torch.float16, 321)):
        ac, asc, bc, bsc, bias, want = G.method_a(g, fa, fb, M, 128, 77, G.tile_targets(TARGETS[tdt], N, 11), ZERO_ROWS)
        dev = to_dev(ac, asc, bc, bsc, bias)
        codes, scales = mx_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, dev[4], out_fmt=out_fmt)
        assert _hip.mx_gemm_q_last_route == VEC
        _, wc, ws = quantize_with_mx(want.to(DEV), out_fmt, -1, return_codes=True)
        assert torch.equal(codes, wc) and torch.equal(scales, ws), (out_fmt, tdt)
