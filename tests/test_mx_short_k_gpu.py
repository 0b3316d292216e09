"""MX product kernels at SHORT contraction lengths against the float64 reference, on data with real dynamic range, within
``mx_gemm_ref.model_bound``: the bound that follows the measured accumulation of v_mfma_scale_f32_16x16x128_f8f6f4 (DESIGN 3b,
"Accumulation") and so holds at every K -- the L-proportional bound of tests/test_mx_gemm_gpu.py does not below L ~ 512.  Operands
come from the GPU quantizer, from normal deviates and from a heavy-tailed draw ``randn * exp(2 randn)`` whose products inside a group
of eight differ by many binades.  Every test prints its largest |err| / bound.  The convolutions are held to the bound on the im2col /
gathered operands that tests/mx_conv_ref.py, mx_conv_transpose_ref.py and mx_conv_wgrad_ref.py build: the k order is theirs."""
import pytest
import torch

import mx_conv_ref as C
import mx_conv_transpose_ref as T
import mx_conv_wgrad_ref as W
import mx_gemm_ref as G
import qsparse_amd as qs
from qsparse_amd import _hip, mx_bmm, mx_bmm_train, mx_quantize_2way_batched, quantize_with_mx
from qsparse_amd.mx_conv import mx_conv2d
from qsparse_amd.mx_conv_train import mx_conv2d_train, mx_conv2d_weight_grad
from qsparse_amd.mx_conv_transpose import mx_conv_transpose2d
from qsparse_amd.mx_gemm import mx_linear, mx_matmul, mx_quantize_2way

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
VEC, PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN
MNS = [(45, 33), (130, 70)]
KS = [8, 33, 40, 64, 90, 128, 129, 200, 320]
PER_PAIR = 4
THREE = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp8_e5m2", "mxfp4_e2m1"), ("mxfp6_e3m2", "mxfp8_e5m2")]
KINDS = ("randn", "heavy")


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def draw(g, kind, *shape):
    x = torch.randn(*shape, generator=g)
    return x if kind == "randn" else x * torch.exp(2 * torch.randn(*shape, generator=g))


def codes_of(x, fmt):
    with torch.no_grad():
        return tuple(quantize_with_mx(x.contiguous(), fmt, -1, return_codes=True)[1:])


def quantized_case(g, kind, lead, M, N, K, fa, fb):
    """codes and scales as the GPU quantizer writes them: activations of `kind`, weights of `kind` / sqrt(K)"""
    return codes_of(draw(g, kind, *lead, M, K).to(DEV), fa) + codes_of((draw(g, kind, *lead, N, K) / K ** 0.5).to(DEV), fb)


def ks_of(fa, fb):
    """PER_PAIR of the 9 contraction lengths for the pair, walking the list by the pair's index (as test_mx_bmm_gpu.shapes_of)"""
    p = G.FMTS.index(fa) * 5 + G.FMTS.index(fb)
    return [(i, KS[i % len(KS)]) for i in range(PER_PAIR * p, PER_PAIR * p + PER_PAIR)]


def test_every_k_meets_every_width():
    for width in ("fp8", "fp6", "fp4"):
        seen = {K for fa, fb in PAIRS if width in fa or width in fb for _, K in ks_of(fa, fb)}
        assert seen == set(KS), width


def check(y, cpu, fa, fb, bias, dt, what, slices=1, old=False, inside=None):
    """y [M, N] against the float64 reference on the CPU copies of the codes that entered the product, within model_bound"""
    _, y64, S = G.reference(*cpu[:2], fa, *cpu[2:], fb, bias, dt)
    assert y.dtype == dt and y.shape == y64.shape
    bound = G.model_bound(*cpu[:2], fa, *cpu[2:], fb, y64, S, bias, dt, slices, inside)
    if dt != torch.float32:
        # the heavy-tailed sums leave fp16's range: from `top` = largest finite + half an ulp on, the cast gives Inf of the sum's
        # sign.  Inf is REQUIRED where the sum lies past `top` by more than the bound, ALLOWED where it lies within the bound of it
        top = torch.finfo(dt).max * (1 + 2.0 ** -G.MANT[dt])
        yd = y.detach().cpu().double()
        inf = yd.isinf() & (yd.sign() == y64.sign())
        assert bool((inf | (y64.abs() - bound < top)).all()) and bool((~yd.isinf() | (inf & (y64.abs() + bound >= top))).all()), what
        y = torch.where(inf, y64, yd)
    ok, ratio = G.within(y, y64, bound)
    line = f"{what}: largest |err| / bound {ratio:.4f}"
    if old:
        K = cpu[0].shape[-1]
        line += f"; / (2 K 2^-23 S + ulp) {G.within(y, y64, 2 * K * 2.0 ** -23 * S + G.ulp(y64, dt))[1]:.4f}"
    print(line)
    assert ok, (what, ratio)
    return ratio


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_mx_matmul(fa, fb):
    g = torch.Generator().manual_seed(900 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    for i, K in ks_of(fa, fb):
        M, N = MNS[i % 2]
        route = VEC if K % 16 == 0 else PLAIN
        for kind in KINDS:
            dev = quantized_case(g, kind, (), M, N, K, fa, fb)
            cpu = tuple(t.cpu() for t in dev)
            bias = torch.randn(N, generator=g)
            inside = G.inside_groups(*cpu[:2], fa, *cpu[2:], fb)
            for dt in (torch.float32,) + ((torch.bfloat16, torch.float16) if i % 3 == 0 else ()):
                for b in (None, bias):
                    y = mx_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, None if b is None else b.to(DEV), dt)
                    assert _hip.mx_gemm_last_route == route, (_hip.mx_gemm_last_route, route)
                    check(y, cpu, fa, fb, b, dt, (fa, fb, kind, (M, N, K), dt, b is not None), inside=inside)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(100, 70, 90), (100, 90, 70)])
def test_the_shape_recorded_above_the_old_bound(shape, kind):
    """(100, 70, 90) with E5M2 gradients: DESIGN recorded 1.14 of the L-proportional bound for dx, the product [100, 70] x [90, 70]"""
    g = torch.Generator().manual_seed(90)
    M, N, K = shape
    for fa, fb in (("mxfp8_e5m2", "mxfp8_e4m3"), ("mxfp8_e5m2", "mxfp8_e5m2")):
        dev = quantized_case(g, kind, (), M, N, K, fa, fb)
        y = mx_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb)
        assert _hip.mx_gemm_last_route == PLAIN
        check(y, tuple(t.cpu() for t in dev), fa, fb, None, torch.float32, (fa, fb, kind, shape), old=True)


@pytest.mark.parametrize("fa,fb", THREE)
@pytest.mark.parametrize("split_k", [2, 3])
def test_split_k(fa, fb, split_k):
    g = torch.Generator().manual_seed(320 + split_k)
    M, N, K = 130, 70, 320
    for kind in KINDS:
        dev = quantized_case(g, kind, (), M, N, K, fa, fb)
        bias = torch.randn(N, generator=g)
        y = mx_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, bias.to(DEV), split_k=split_k)
        assert _hip.mx_gemm_last_split == split_k and _hip.mx_gemm_last_route == VEC
        check(y, tuple(t.cpu() for t in dev), fa, fb, bias, torch.float32, (fa, fb, kind, "split_k", split_k), slices=split_k)


@pytest.mark.parametrize("fa,fb", THREE)
@pytest.mark.parametrize("shape", [(37, 50, 40), (45, 33, 64), (197, 64, 197)])
def test_mx_bmm(fa, fb, shape):
    g = torch.Generator().manual_seed(sum(shape))
    Gn, (M, N, K) = 3, shape
    for kind in KINDS:
        dev = quantized_case(g, kind, (Gn,), M, N, K, fa, fb)
        cpu = tuple(t.cpu() for t in dev)
        for bias in (torch.randn(N, generator=g), torch.randn(Gn, N, generator=g)):
            y = mx_bmm(dev[0], dev[1], fa, dev[2], dev[3], fb, bias.to(DEV))
            assert _hip.mx_bmm_last_route == (VEC if K % 16 == 0 else PLAIN)
            for s in range(Gn):
                check(y[s], tuple(t[s] for t in cpu), fa, fb, bias if bias.dim() == 1 else bias[s], torch.float32,
                      (fa, fb, kind, shape, tuple(bias.shape), "slice", s))


@pytest.mark.parametrize("S", [37, 50])
@pytest.mark.parametrize("d", [40, 64])
def test_the_two_products_of_attention(S, d):
    """the public calls of test_mx_bmm_gpu.attention_composition, taken apart: q k^T over d, then softmax(s) v over S -- each product
    against the reference on the codes that entered it; the softmax stays outside the bound"""
    g = torch.Generator().manual_seed(S + d)
    B, h, T = 2, 3, 37
    f = "mxfp8_e4m3"
    for kind in KINDS:
        q, k, v = (draw(g, kind, B * h, n, d).to(DEV) for n in (T, S, S))
        qc, kc = codes_of(q, f), codes_of(k, f)
        s = mx_bmm(*qc, f, *kc, f)
        pc, vc = codes_of(torch.softmax(s * d ** -0.5, -1), f), codes_of(v.transpose(-1, -2), f)
        o = mx_bmm(*pc, f, *vc, f)
        assert _hip.mx_bmm_last_route == (VEC if S % 16 == 0 else PLAIN)
        for name, y, ops in (("q k^T", s, qc + kc), ("p v", o, pc + vc)):
            cpu = tuple(t.cpu() for t in ops)
            for j in range(B * h):
                check(y[j], tuple(t[j] for t in cpu), f, f, None, torch.float32, (name, kind, S, d, "slice", j))


FX, FW, FG = "mxfp8_e4m3", "mxfp4_e2m1", "mxfp8_e5m2"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(100, 70, 90), (45, 33, 40)])
def test_mx_linear(shape, kind):
    """y, dx, dW of mx_linear against the reference on the two-way quantizer's bytes taken from the CPU path (row pair: blocks
    along the last axis; column pair: the transpose's), which the GPU's are asserted to equal here"""
    g = torch.Generator().manual_seed(sum(shape))
    M, N, K = shape
    x, w, b, dy = draw(g, kind, M, K), draw(g, kind, N, K) / K ** 0.5, torch.randn(N, generator=g), draw(g, kind, M, N) / N
    cpu = {n: mx_quantize_2way(t, f, f) for n, t, f in (("x", x, FX), ("w", w, FW), ("dy", dy, FG))}
    for n, t, f in (("x", x, FX), ("w", w, FW), ("dy", dy, FG)):
        for got, want in zip(mx_quantize_2way(t.to(DEV), f, f), cpu[n]):
            assert torch.equal(got.cpu(), want), n
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = mx_linear(xd, wd, bd, FX, FW, FG)
    dx, dw = torch.autograd.grad(y, (xd, wd), dy.to(DEV))
    slices = _hip.mx_gemm_last_split                                      # (the weight gradient is the backward's last product)
    row, col = (lambda p: p[:2]), (lambda p: p[2:])
    check(y.detach(), row(cpu["x"]) + row(cpu["w"]), FX, FW, b, torch.float32, ("mx_linear y", shape, kind))
    check(dx, row(cpu["dy"]) + col(cpu["w"]), FG, FW, None, torch.float32, ("mx_linear dx", shape, kind), old=True)
    check(dw, col(cpu["dy"]) + col(cpu["x"]), FG, FX, None, torch.float32, ("mx_linear dW", shape, kind), slices=slices)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("shape", [(100, 70, 90), (45, 33, 40)])
def test_mx_bmm_train(shape, layout, kind):
    """y, da, db of mx_bmm_train against the reference on the batched two-way quantizer's bytes taken from the CPU path"""
    g = torch.Generator().manual_seed(sum(shape))
    Gn, (M, N, K), kn = 2, shape, layout == "kn"
    a, b, dy = draw(g, kind, Gn, M, K), (draw(g, kind, Gn, K, N) if kn else draw(g, kind, Gn, N, K)) / K ** 0.5, draw(g, kind, Gn, M, N) / N
    cpu = {n: mx_quantize_2way_batched(t, f, f) for n, t, f in (("a", a, FX), ("b", b, FW), ("dy", dy, FG))}
    for n, t, f in (("a", a, FX), ("b", b, FW), ("dy", dy, FG)):
        for got, want in zip(mx_quantize_2way_batched(t.to(DEV), f, f), cpu[n]):
            assert torch.equal(got.cpu(), want), (n, layout)
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = mx_bmm_train(ad, bd, b_layout=layout, a_fmt=FX, b_fmt=FW, grad_fmt=FG)
    da, db = torch.autograd.grad(y, (ad, bd), dy.to(DEV))
    row, col = (lambda p: p[:2]), (lambda p: p[2:])
    b_k, b_n = (col, row) if kn else (row, col)                           # b with blocks along K / along N
    products = [("y", y.detach(), row(cpu["a"]), FX, b_k(cpu["b"]), FW), ("da", da, row(cpu["dy"]), FG, b_n(cpu["b"]), FW),
                ("db", db, col(cpu["a"]), FX, col(cpu["dy"]), FG) if kn else ("db", db, col(cpu["dy"]), FG, col(cpu["a"]), FX)]
    for name, got, pa, fa, pb, fb in products:
        for s in range(Gn):
            check(got[s], (pa[0][s], pa[1][s], pb[0][s], pb[1][s]), fa, fb, None, torch.float32, ("mx_bmm_train " + name, shape, layout, kind, s))


# ---- the convolutions: 3 x 3, stride 2, padding 1, B = 2, 9 x 9 pixels (5 x 5 on the short side), Cout = 20 ---------------------------
CONV_B, CONV_HW, CONV_OHW, CONV_COUT, KS3, GEOM = 2, 9, 5, 20, (3, 3), (2, 1, 1)       # GEOM: stride, padding, dilation


def on_cpu(ops):
    return tuple(t.cpu() for t in ops)


@pytest.mark.parametrize("fx,fw", THREE)
@pytest.mark.parametrize("Cin", [8, 40])
def test_mx_conv2d(Cin, fx, fw):
    """x [2, 9, 9, C] -> y [2, 5, 5, 20]: M = 50, K' = 9 Cp (288 / 576, of which 72 / 360 are no padding)"""
    g = torch.Generator().manual_seed(Cin)
    for kind in KINDS:
        x, w = draw(g, kind, CONV_B, CONV_HW, CONV_HW, Cin), draw(g, kind, CONV_COUT, 3, 3, Cin) / (9 * Cin) ** 0.5
        ops = codes_of(x.to(DEV), fx) + codes_of(w.to(DEV), fw)
        bias = torch.randn(CONV_COUT, generator=g)
        cpu = on_cpu(C.im2col_codes(*ops, 3, 3, *GEOM))
        for dt, b in ((torch.float32, None), (torch.float32, bias), (torch.bfloat16, bias), (torch.float16, None)):
            y = mx_conv2d(ops[0], ops[1], fx, ops[2], ops[3], fw, None if b is None else b.to(DEV), *GEOM, dt)
            assert y.shape == (CONV_B, CONV_OHW, CONV_OHW, CONV_COUT)
            check(y.reshape(-1, CONV_COUT), cpu, fx, fw, b, dt, ("mx_conv2d", Cin, fx, fw, kind, dt, b is not None))


@pytest.mark.parametrize("fx,fw", THREE)
@pytest.mark.parametrize("Cin", [8, 40])
def test_mx_conv_transpose2d(Cin, fx, fw):
    """x [2, 5, 5, C] -> y [2, 9, 9, 20]: M = 162, at most 4 of the 9 taps exist for an output pixel"""
    g = torch.Generator().manual_seed(100 + Cin)
    for kind in KINDS:
        x, w = draw(g, kind, CONV_B, CONV_OHW, CONV_OHW, Cin), draw(g, kind, CONV_COUT, 3, 3, Cin) / (4 * Cin) ** 0.5
        ops = codes_of(x.to(DEV), fx) + codes_of(w.to(DEV), fw)
        bias = torch.randn(CONV_COUT, generator=g)
        cpu = on_cpu(T.gathered_codes(*ops, 2, 1, 0, 1))
        for dt, b in ((torch.float32, None), (torch.float32, bias), (torch.bfloat16, bias), (torch.float16, None)):
            y = mx_conv_transpose2d(ops[0], ops[1], fx, ops[2], ops[3], fw, None if b is None else b.to(DEV), 2, 1, 0, 1, dt)
            assert y.shape == (CONV_B, CONV_HW, CONV_HW, CONV_COUT)
            check(y.reshape(-1, CONV_COUT), cpu, fx, fw, b, dt, ("mx_conv_transpose2d", Cin, fx, fw, kind, dt, b is not None))


def batch_blocked(t, fmt):
    """the column pair of the two-way quantizer on a channels-last t [B, H, W, C] seen as [B, H W C]: codes [H, W, C, B]"""
    B, H, W_, Cn = t.shape
    _, _, cc, cs = mx_quantize_2way(t.reshape(B, -1), None, fmt)
    return cc.view(H, W_, Cn, B), cs.view(H, W_, Cn, -1)


@pytest.mark.parametrize("fg,fx", [("mxfp8_e5m2", "mxfp8_e4m3"), ("mxfp8_e5m2", "mxfp4_e2m1"), ("mxfp6_e3m2", "mxfp8_e5m2")])
@pytest.mark.parametrize("Cin", [8, 40])
def test_conv_weight_grad(Cin, fg, fx):
    """dy [2, 5, 5, 20], x [2, 9, 9, C] -> dW [20, 3, 3, C]: the contraction runs over B OH OW = 50 products (K' = 25 x 32, the
    batch padded to a block with zero codes)"""
    g = torch.Generator().manual_seed(200 + Cin)
    for kind in KINDS:
        x, dy = draw(g, kind, CONV_B, CONV_HW, CONV_HW, Cin), draw(g, kind, CONV_B, CONV_OHW, CONV_OHW, CONV_COUT) / 50 ** 0.5
        ops = batch_blocked(dy.to(DEV), fg) + batch_blocked(x.to(DEV), fx)
        cpu = on_cpu(W.gathered_codes(*ops, KS3, *GEOM))
        for dt, split_k in ((torch.float32, 1), (torch.float32, 2), (torch.bfloat16, "auto")):
            dw = mx_conv2d_weight_grad(ops[0], ops[1], fg, ops[2], ops[3], fx, KS3, *GEOM, dt, split_k)
            assert dw.shape == (CONV_COUT, 3, 3, Cin)
            check(dw.reshape(CONV_COUT, -1), cpu, fg, fx, None, dt, ("conv weight grad", Cin, fg, fx, kind, dt, split_k),
                  slices=_hip.mx_conv_wgrad_last_split)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Cin", [8, 40])
def test_mx_conv2d_train(Cin, kind):
    """y, dx, dW of mx_conv2d_train against the reference on the gathered operands of the public quantizer's bytes taken from the
    CPU path -- Q(x; C), Q(W; C) for y, Q(dy; Cout), Q(W; Cout) for dx, Q(dy; B), Q(x; B) for dW -- which the GPU's are asserted to
    equal here"""
    g = torch.Generator().manual_seed(300 + Cin)
    x, w = draw(g, kind, CONV_B, Cin, CONV_HW, CONV_HW), draw(g, kind, CONV_COUT, Cin, 3, 3) / (9 * Cin) ** 0.5
    bias, dy = torch.randn(CONV_COUT, generator=g), draw(g, kind, CONV_B, CONV_COUT, CONV_OHW, CONV_OHW) / 25
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous()

    def q(t, f, dim):
        """codes and scales of t quantized along `dim`, that axis moved last; the GPU quantizer's must be the same bytes"""
        cpu = tuple(u.movedim(dim, -1).contiguous() for u in quantize_with_mx(t, f, dim, return_codes=True)[1:])
        dev = tuple(u.movedim(dim, -1) for u in quantize_with_mx(t.to(DEV), f, dim, return_codes=True)[1:])
        assert all(torch.equal(a, b.cpu()) for a, b in zip(cpu, dev)), (f, dim)
        return cpu

    xl, wl, dyl = cl(x), cl(w), cl(dy)                                     # [B, H, W, C], [Cout, KH, KW, C], [B, OH, OW, Cout]
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    y = mx_conv2d_train(xd, wd, bd, *GEOM, FX, FW, FG)
    dx, dw = torch.autograd.grad(y, (xd, wd), dy.to(DEV))
    slices = _hip.mx_conv_wgrad_last_split
    check(cl(y.detach()).reshape(-1, CONV_COUT), C.im2col_codes(*q(xl, FX, 3), *q(wl, FW, 3), 3, 3, *GEOM), FX, FW, bias, torch.float32,
          ("mx_conv2d_train y", Cin, kind))
    wt = wl.permute(3, 1, 2, 0).contiguous()                               # [C, KH, KW, Cout]
    check(cl(dx).reshape(-1, Cin), T.gathered_codes(*q(dyl, FG, 3), *q(wt, FW, 3), 2, 1, 0, 1), FG, FW, None, torch.float32,
          ("mx_conv2d_train dx", Cin, kind))
    check(cl(dw).reshape(CONV_COUT, -1), W.gathered_codes(*q(dyl, FG, 0), *q(xl, FX, 0), KS3, *GEOM), FG, FX, None, torch.float32,
          ("mx_conv2d_train dW", Cin, kind), slices=slices)
