"""The CPU twin of tests/test_mx_epilogue_rounding_gpu.py: the helpers of mx_gemm_ref that state the output rounding bit for bit
(rounding_targets, round_once_bits, method_a, method_b), proved without a GPU -- the bias construction is exact, every subset of a
method-B sum is held by 24 bits in every order, the two definitions of the cast agree, no case leaves the strict comparison -- the same
cases through the package's CPU paths, and the mutations: each wrong epilogue an implementation could plausibly have is applied to
the exact float32 values here and must differ from the expected bits on at least one target, so the target set can see the bugs it
is meant to see."""
import itertools

import pytest
import torch

import mx_gemm_ref as G
from qsparse_amd.mx_bmm import mx_bmm
from qsparse_amd.mx_conv import mx_conv2d
from qsparse_amd.mx_conv_train import mx_conv2d_weight_grad
from qsparse_amd.mx_conv_transpose import mx_conv2d_input_grad, mx_conv_transpose2d
from qsparse_amd.mx_gemm import mx_matmul

ALL_PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
PAIRS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp6_e2m3", "mxfp8_e5m2")]
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
TARGETS = {dt: G.rounding_targets(dt) for dt in G.TWO_BYTE}


def check(y, want32, dt, what):
    want = G.expected_rounded(want32, dt).reshape(y.shape)
    strict = G.strict_class(want32)
    assert float(strict.float().mean()) == 1.0, what
    assert y.dtype == dt and bool(G.bits_equal(y, want).all()), what


# ---- the helpers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", G.TWO_BYTE)
def test_targets_cover_what_they_claim(dt):
    t = TARGETS[dt]
    bits = G.f32_bits(t)
    assert len(set(bits.tolist())) == len(t) and bool((((bits >> 23) & 0xFF) >= 1).all()) and bool((((bits >> 23) & 0xFF) <= 254).all())
    assert float(G.strict_class(t).float().mean()) == 1.0                    # the strict share: every target is compared bit for bit
    drop = 23 - (G.MANT[dt] - 1)
    half = 1 << (drop - 1)
    e, lsb, d = ((bits >> 23) & 0xFF) - 127, (bits >> drop) & 1, bits & ((1 << drop) - 1)
    for binade in G.BINADES[dt]:
        for parity in (0, 1):
            for part in (0, 1, half - 1, half, half + 1, 2 * half - 1):
                for sign in (0, 1):
                    assert bool(((e == binade) & (lsb == parity) & (d == part) & (bits >> 31 == sign)).any()), (binade, parity, part, sign)
    r = G.expected_rounded(t, dt).double()
    if dt == torch.float16:
        for v, to in ((65504.0, 65504.0), (65520.0 - 2.0 ** -8, 65504.0), (65520.0, float("inf")), (65536.0, float("inf")), (2.0 ** -14, 2.0 ** -14),
                      (2.0 ** -14 - 2.0 ** -25, 2.0 ** -14), (2.0 ** -24, 2.0 ** -24), (1.5 * 2.0 ** -24, 2.0 ** -23), (2.0 ** -25, 0.0),
                      (2.0 ** -25 + 2.0 ** -48, 2.0 ** -24), (2.0 ** -26, 0.0)):
            for s in (1.0, -1.0):
                at = (t.double() == s * v).nonzero()
                assert len(at) == 1 and float(r[at[0, 0]]) == s * to and bool(torch.signbit(r[at[0, 0]])) == (s < 0), (v, s)
    else:
        big = 2.0 ** 127 * (2 - 2.0 ** -7)
        for v, to in ((big, big), (big + 0x7FFF * 2.0 ** 104, big), (big + 0x8000 * 2.0 ** 104, float("inf")), (float(torch.finfo(torch.float32).max), float("inf"))):
            for s in (1.0, -1.0):
                at = (t.double() == s * v).nonzero()
                assert len(at) == 1 and float(r[at[0, 0]]) == s * to, (v, s)


@pytest.mark.parametrize("dt", G.TWO_BYTE)
def test_both_definitions_of_the_cast_agree(dt):
    t = TARGETS[dt]
    assert torch.equal(G.round_once_bits(t, dt), G.cast_bits(t, dt))
    g = torch.Generator().manual_seed(5)
    x = G.f32_from_bits(torch.randint(0, 2 ** 32, (8000,), generator=g, dtype=torch.int64))
    x = torch.cat([x, G.f32_from_bits([0, 1 << 31, 0x7F800000, 0xFF800000, 1, 0x007FFFFF, 0x00800000, 0x33000000, 0x33000001, 0x387FC000, 0x387FE000])])
    a, b = G.round_once_bits(x, dt), G.cast_bits(x, dt)
    fin = ~x.isnan()
    assert int(fin.sum()) > 7000 and torch.equal(a[fin], b[fin])
    assert bool(G.two_byte_from_bits(a[~fin], dt).isnan().all())


def test_method_a_is_exact_for_every_pair_and_knows_its_zero_rows():
    g = torch.Generator().manual_seed(1)
    for dt in G.TWO_BYTE:
        t = TARGETS[dt]
        ac, asc, bc, bsc, bias, want = G.method_a(g, "mxfp4_e2m1", "mxfp6_e3m2", 5, 127, 70, t, (2,))      # (asserts p + bias = t itself)
        assert int(((bias == 0) & torch.signbit(bias)).sum()) > 0 and int(((bias == 0) & ~torch.signbit(bias)).sum()) > 0
        assert not bool(torch.signbit(want[2][bias == 0]).any())             # +0 + -0 = +0
        y64 = G.reference(ac, asc, "mxfp4_e2m1", bc, bsc, "mxfp6_e3m2", bias)[1]
        assert torch.equal(y64, want.double())                              # the float64 sum of the definition is the target, exactly
        assert int(ac.count_nonzero()) == 4 and int(bc.count_nonzero()) == len(t)


@pytest.mark.parametrize("dt", G.TWO_BYTE)
def test_method_b_sums_are_exact_in_every_subset_and_order(dt):
    every = G.f32_bits(TARGETS[dt]).tolist()
    for with_bias in (False, True):
        t, terms, bias = G.method_b_targets(dt, with_bias)
        assert len(t) >= len(every) // 2
        acc = t if bias is None else t - bias
        for b, tn in zip(G.f32_bits(acc).tolist(), terms):
            assert 1 <= len(tn) <= 4 and len({e for _, e in tn}) == len(tn) and all(-126 <= e <= 127 for _, e in tn)
            floor = min(e for _, e in tn)
            value = sum((-1 if s else 1) * 2.0 ** e for s, e in tn)
            assert value == float(G.f32_from_bits([b]).double())
            for k in range(len(tn) + 1):
                for sub in itertools.combinations(tn, k):
                    assert G.representable24(G._as_int(list(sub), floor)) if sub else True
            for order in itertools.permutations(tn):                         # the same in float32 arithmetic, addition by addition
                s = torch.zeros((), dtype=torch.float32)
                for sg, e in order:
                    s = s + torch.tensor((-1.0 if sg else 1.0) * 2.0 ** e, dtype=torch.float32)
                assert float(s.double()) == value
        # what the method leaves to method A: the forms that need more than four terms or 2^128, and nothing in the middle binades
        # whose kept bits are a single one or none
        drop = 23 - (G.MANT[dt] - 1)
        got = set(G.f32_bits(t).tolist())
        for b in every:
            e, hi = ((b >> 23) & 0xFF) - 127, (b >> drop) & ((1 << (G.MANT[dt] - 1)) - 1)
            if e in G.BINADES[dt][1:-1] and hi in (0, 1):
                assert b in got, hex(b)


def test_the_emulated_instruction_returns_the_targets():
    """model_emulate follows the measured accumulation of the MFMA (cuts inside groups, alignment of the block sums): on method B's
    operands it loses nothing, for every layout the GPU test uses"""
    g = torch.Generator().manual_seed(2)
    fa, fb = "mxfp8_e4m3", "mxfp6_e2m3"
    for dt in G.TWO_BYTE:
        t, terms, _ = G.method_b_targets(dt)
        for K, blocks in ((128, (0, 1, 2, 3)), (384, (1, 5, 6, 10)), (256, (0, 3, 4, 7)), (288, (0, 3, 4, 8))):
            ops = G.method_b(g, fa, fb, 2, K, blocks, terms)
            y = G.model_emulate(ops[0], ops[1], fa, ops[2], ops[3], fb)
            assert torch.equal(y, t.double().repeat(2, 1)), (dt, K)
            assert torch.equal(G.reference(ops[0], ops[1], fa, ops[2], ops[3], fb)[1], t.double().repeat(2, 1))


# ---- the same cases through the CPU paths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fa,fb", ALL_PAIRS)
def test_matmul_cpu_path_one_term_plus_bias(fa, fb):
    g = torch.Generator().manual_seed(2100 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    for tdt, N, K, k0 in ((torch.bfloat16, 306, 128, 37), (torch.float16, 308, 127, 126)):
        ac, asc, bc, bsc, bias, want = G.method_a(g, fa, fb, 9, K, k0, G.tile_targets(TARGETS[tdt], N, 5), (0, 4))
        for dt in DTYPES:
            check(mx_matmul(ac, asc, fa, bc, bsc, fb, bias, dt), want, dt, (fa, fb, tdt, dt))


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_matmul_cpu_path_sum_of_powers_of_two(fa, fb):
    g = torch.Generator().manual_seed(2300 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    for tdt in G.TWO_BYTE:
        for with_bias in (False, True):
            t, terms, bias = G.method_b_targets(tdt, with_bias)
            ops = G.method_b(g, fa, fb, 3, 384, (2, 4, 7, 11), terms)
            for dt in DTYPES:
                check(mx_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, bias, dt, split_k=3), t.repeat(3, 1), dt, (fa, fb, tdt, dt, with_bias))


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_bmm_cpu_path(fa, fb):
    g = torch.Generator().manual_seed(2500 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    for tdt in G.TWO_BYTE:
        cases = [G.method_a(g, fa, fb, 6, 127, 33, G.tile_targets(TARGETS[tdt], 310, 101 * s), (1,)) for s in range(3)]
        ac, asc, bc, bsc, bias, want = (torch.stack([c[j] for c in cases]) for j in range(6))
        for dt in DTYPES:
            check(mx_bmm(ac, asc, fa, bc, bsc, fb, bias, dt), want, dt, (fa, fb, tdt, dt))


@pytest.mark.parametrize("fx,fw", PAIRS)
def test_conv_cpu_paths(fx, fw):
    """the geometries of the GPU test -- forward, transposed, input gradient, weight gradient -- say what the GPU test takes them to say"""
    g = torch.Generator().manual_seed(2600 + G.FMTS.index(fx) * 5 + G.FMTS.index(fw))
    MC = 4
    for tdt in G.TWO_BYTE:
        N = 307
        xc, xs, wc, ws, bias, want = G.method_a(g, fx, fw, MC, 288, (2 * 3 + 1) * 32 + 5, G.tile_targets(TARGETS[tdt], N, N), (3,))
        for dt in DTYPES:
            y = mx_conv2d(xc.view(-1, 3, 3, 32), xs.view(-1, 3, 3, 1), fx, wc.view(-1, 3, 3, 32), ws.view(-1, 3, 3, 1), fw, bias, 1, 0, 1, dt)
            check(y.view(MC, N), want, dt, (fx, fw, tdt, dt, "conv A"))
        t, terms, _ = G.method_b_targets(tdt)
        n = len(t)
        xc, xs, wc, ws = G.method_b(g, fx, fw, MC, 288, (0, 3, 4, 8), terms)
        for dt in DTYPES:
            y = mx_conv2d(xc.view(-1, 3, 3, 32), xs.view(-1, 3, 3, 1), fx, wc.view(-1, 3, 3, 32), ws.view(-1, 3, 3, 1), fw, None, 1, 0, 1, dt)
            check(y.view(MC, n), t.repeat(MC, 1), dt, (fx, fw, tdt, dt, "conv B"))
        # transposed: a 1 x 1 image under a 2 x 2 kernel, the fourth tap empty
        xc, xs, wc, ws, bias, want = G.method_a(g, fx, fw, MC, 32, 9, G.tile_targets(TARGETS[tdt], N, 17), (1,))
        w4, s4 = wc.view(N, 1, 1, 32).repeat(1, 2, 2, 1), ws.view(N, 1, 1, 1).repeat(1, 2, 2, 1)
        w4[:, 1, 1] = 0
        want4 = want.view(MC, 1, 1, N).repeat(1, 2, 2, 1)
        want4[:, 1, 1] = torch.zeros(N) + bias
        y = mx_conv_transpose2d(xc.view(MC, 1, 1, 32), xs.view(MC, 1, 1, 1), fx, w4, s4, fw, bias, 1, 0, 0, 1, tdt)
        check(y, want4, tdt, (fx, fw, tdt, "transposed"))
        # input gradient: method B along the 128 output channels of the one tap
        gc, gs, wc, ws = G.method_b(g, fx, fw, MC, 128, (0, 1, 2, 3), terms)
        y = mx_conv2d_input_grad(gc.view(MC, 1, 1, 128), gs.view(MC, 1, 1, 4), fx, wc.view(n, 1, 1, 128).repeat(1, 2, 2, 1),
                                 ws.view(n, 1, 1, 4).repeat(1, 2, 2, 1), fw, (2, 2), 1, 0, 1, tdt)
        check(y, t.view(1, 1, 1, n).repeat(MC, 2, 2, 1), tdt, (fx, fw, tdt, "input grad"))
        # weight gradient: the terms in blocks along the batch
        C, B = 13, 256
        tt, tm = t[: 9 * C], terms[: 9 * C]
        gc, gs, xc, xs = G.method_b(g, fx, fw, 5, B, (1, 2, 5, 6), tm)
        dw = mx_conv2d_weight_grad(gc.view(1, 1, 5, B), gs.view(1, 1, 5, -1), fx, xc.view(3, 3, C, B), xs.view(3, 3, C, -1), fw, (3, 3), 1, 0, 1,
                                   tdt, split_k=2)
        check(dw.view(5, 9 * C), tt.repeat(5, 1), tdt, (fx, fw, tdt, "weight grad"))


# ---- the mutations ----------------------------------------------------------------------------------------------------------------------
def _bf16_style(u, rule):
    """a wrong bfloat16 cast on the bit pattern: the upper 16 bits, moved by `rule`(kept, discarded, sign)"""
    kept, d = (u & 0x7FFFFFFF) >> 16, u & 0xFFFF
    return (u >> 31) << 15 | (kept + rule(kept, d, u >> 31).to(torch.int64))


def _f16_style(t, rule):
    """a wrong float16 cast by value, for |t| inside float16's normal range (elsewhere: the right one): the multiple of the spacing
    2^(e - 10) that `rule`(kept, remainder, half, sign) picks"""
    right = G.round_once_bits(t, torch.float16)
    x = t.double()
    mag = x.abs()
    inside = (mag >= 2.0 ** -14) & (mag < 65504.0)
    e = torch.frexp(torch.where(inside, mag, torch.ones_like(mag)))[1] - 1
    q = torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 10).double())
    kept = torch.floor(mag / q)
    frac = mag / q - kept                                                      # exact: a float32 divided by a power of two
    kept = kept + rule(kept.to(torch.int64), frac, torch.signbit(x)).double()
    wrong = G.cast_bits((kept * q * torch.where(torch.signbit(x), -1.0, 1.0)).float(), torch.float16)          # kept q is a float16: the cast is exact
    return torch.where(inside, wrong, right)


MUTATIONS_BF16 = {
    "truncation": lambda k, d, s: torch.zeros_like(k, dtype=torch.bool),
    "half up": lambda k, d, s: torch.where(s == 0, d >= 0x8000, d > 0x8000),
    "half away from zero": lambda k, d, s: d >= 0x8000,
    "half to odd": lambda k, d, s: (d > 0x8000) | ((d == 0x8000) & (k & 1 == 0)),
}
MUTATIONS_F16 = {
    "truncation": lambda k, f, neg: torch.zeros_like(neg),
    "half up": lambda k, f, neg: torch.where(neg, f > 0.5, f >= 0.5),
    "half away from zero": lambda k, f, neg: f >= 0.5,
    "half to odd": lambda k, f, neg: (f > 0.5) | ((f == 0.5) & (k & 1 == 0)),
}


def caught(wrong_bits, t, dt):
    """the number of targets on which the wrong epilogue's bits differ from the expected ones"""
    return int((wrong_bits != G.round_once_bits(t, dt)).sum())


@pytest.mark.parametrize("name", list(MUTATIONS_BF16))
def test_a_wrong_rounding_rule_is_caught(name):
    t = TARGETS[torch.bfloat16]
    n = caught(_bf16_style(G.f32_bits(t), MUTATIONS_BF16[name]), t, torch.bfloat16)
    t = TARGETS[torch.float16]
    m = caught(_f16_style(t, MUTATIONS_F16[name]), t, torch.float16)
    print(name, "differs on", n, "bfloat16 and", m, "float16 targets")
    assert n > 0 and m > 0


@pytest.mark.parametrize("dt", G.TWO_BYTE)
def test_rounding_the_accumulator_before_the_bias_is_caught(dt):
    """round(round(acc) + bias).  Method A hardly sees it -- its accumulator is a power of two, which the dtype holds unless it is
    below float16's subnormals -- so the cases that must catch it are the split-K ones with a bias (method B's sum plus a bias that
    makes the last bits): there the accumulator is an exact tie, or an odd multiple of the spacing"""
    def wrong(acc, bias):
        first = G.two_byte_from_bits(G.round_once_bits(acc, dt), dt).float()
        return G.round_once_bits(first + bias, dt)
    t, _, bias = G.method_b_targets(dt, True)
    n = caught(wrong(t - bias, bias), t, dt)
    print(dt, "differs on", n, "of", len(t), "targets of method B with a bias")
    assert n > 0
    everything = TARGETS[dt]
    p = G.f32_from_bits(G.f32_bits(everything) & 0xFF800000)
    print(dt, "method A alone differs on", caught(wrong(p, everything - p), everything, dt), "of", len(everything))


def test_float16_saturation_flush_and_lost_zero_sign_are_caught():
    """bfloat16 has the range of float32: it neither overflows before float32 does nor has subnormals or zero results among the
    targets (those are float32 subnormals, the one-term test's), so these three are float16's"""
    t = TARGETS[torch.float16]
    right = G.round_once_bits(t, torch.float16)
    saturating = torch.where(right & 0x7FFF == 0x7C00, right & 0x8000 | 0x7BFF, right)                    # 65504 instead of Inf
    flushing = torch.where(right & 0x7C00 == 0, right & 0x8000, right)                                      # subnormals to zero
    unsigned_zero = torch.where(right & 0x7FFF == 0, torch.zeros_like(right), right)                        # -0 stored as +0
    for name, wrong in (("saturating", saturating), ("flushing", flushing), ("unsigned zero", unsigned_zero)):
        assert caught(wrong, t, torch.float16) > 0, name
    overflowing = G.round_once_bits(TARGETS[torch.bfloat16], torch.bfloat16)
    assert caught(torch.where(overflowing & 0x7FFF == 0x7F80, overflowing & 0x8000 | 0x7F7F, overflowing), TARGETS[torch.bfloat16], torch.bfloat16) > 0


def test_bfloat16_by_adding_half_and_cutting_is_caught():
    t = TARGETS[torch.bfloat16]
    u = G.f32_bits(t)
    assert caught((u + 0x8000) >> 16, t, torch.bfloat16) > 0
