"""``mx_bmm_train`` / ``mx_attention_train`` on the GPU.  The codes of every operand are bit-equal to the CPU path's; every product is
bit-equal to the table of public calls on the GPU; and against ``mx_gemm_ref.reference`` the bound is the one tests/test_mx_bmm_gpu.py
uses -- bit equality (``G.same``) on operands whose products sum exactly in float32 in any order, here values from {0, +-0.5, +-1,
+-2}.  On normal deviates every product is held to ``mx_gemm_ref.model_bound``, the bound that follows the instruction's measured
accumulation and holds at every K (tests/test_mx_short_k_gpu.py); the largest |err| / (2 K 2^-23 S + ulp) of
tests/test_mx_gemm_gpu.py's general class is still printed beside it: at K = 40 one element of y (float32, E4M3 x FP4) measured
1.025 of that one, which was derived for K >= 768.  Then graph capture of a stochastic step."""
import pytest
import torch

import mx_gemm_ref as G
from qsparse_amd import mx_attention, mx_attention_train, mx_bmm_train, mx_quantize_2way_batched
from test_mx_bmm_train import composition, exact_operands, float64_autograd, table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMTS = ("mxfp8_e4m3", "mxfp4_e2m1", "mxfp8_e5m2")      # a, b, dy
SHAPE = (3, 45, 33, 40)                                # G, M, N, K


def against_reference(y, a_pair, fa, b_pair, fb, what, exact):
    """y [G, M, N] against the float64 reference on the codes a_pair [G, M, K] / b_pair [G, N, K] (CPU tensors)"""
    K = a_pair[0].shape[-1]
    for s in range(y.shape[0]):
        y_ref, y64, S = G.reference(a_pair[0][s], a_pair[1][s], fa, b_pair[0][s], b_pair[1][s], fb, None, y.dtype)
        if exact:
            assert G.same(y[s], y_ref + 0.0), (what, s)          # (the sum of the definition starts at +0, as test_mx_bmm_gpu.py)
        else:
            print(what, "slice", s, "largest |err| / general-class bound", G.within(y[s], y64, 2 * K * 2.0 ** -23 * S + G.ulp(y64, y.dtype))[1])
            ok, ratio = G.within(y[s], y64, G.model_bound(a_pair[0][s], a_pair[1][s], fa, b_pair[0][s], b_pair[1][s], fb, y64, S, None, y.dtype))
            print(what, "slice", s, "largest |err| / model bound", ratio)
            assert ok, (what, s, ratio)


@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("exact", [True, False])
def test_codes_equal_the_cpu_path_and_products_the_reference(layout, dtype, exact):
    g = torch.Generator().manual_seed(1)
    Gn, M, N, K = SHAPE
    kn = layout == "kn"
    fa, fb, fg = FMTS
    if exact:
        a, b, dy = (t.to(dtype) for t in exact_operands(g, (Gn,), M, N, K, kn))
    else:
        a = torch.randn(Gn, M, K, generator=g).to(dtype)
        b = (torch.randn(Gn, K, N, generator=g) if kn else torch.randn(Gn, N, K, generator=g)).to(dtype)
        dy = torch.randn(Gn, M, N, generator=g).to(dtype)
    cpu = {n: mx_quantize_2way_batched(t, f, f) for n, t, f in (("a", a, fa), ("b", b, fb), ("dy", dy, fg))}
    for n, t, f in (("a", a, fa), ("b", b, fb), ("dy", dy, fg)):
        for got, want in zip(mx_quantize_2way_batched(t.to(DEV), f, f), cpu[n]):
            assert torch.equal(got.cpu(), want), (n, layout)
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = mx_bmm_train(ad, bd, b_layout=layout, a_fmt=fa, b_fmt=fb, grad_fmt=fg)
    da, db = torch.autograd.grad(y, (ad, bd), dy.to(DEV))
    assert y.dtype == da.dtype == db.dtype == dtype and da.shape == a.shape and db.shape == b.shape
    # the table of public calls on the GPU, bit for bit
    want = table(ad.detach(), bd.detach(), None, dy.to(DEV), kn, fa, fb, fg, dtype)
    for name, got, w in zip(("y", "da", "db"), (y.detach(), da, db), want):
        assert G.same(got, w), (name, layout, dtype)
    row, col = (lambda p: p[:2]), (lambda p: p[2:])
    b_k, b_n = (col, row) if kn else (row, col)          # b with blocks along K / along N
    against_reference(y.detach(), row(cpu["a"]), fa, b_k(cpu["b"]), fb, "y", exact)
    against_reference(da, row(cpu["dy"]), fg, b_n(cpu["b"]), fb, "da", exact)
    if kn:
        against_reference(db, col(cpu["a"]), fa, col(cpu["dy"]), fg, "db", exact)
    else:
        against_reference(db, col(cpu["dy"]), fg, col(cpu["a"]), fa, "db", exact)


@pytest.mark.parametrize("layout", ["nk", "kn"])
@pytest.mark.parametrize("fmt", G.FMTS)
def test_exact_operands_are_exact_on_the_gpu(layout, fmt):
    g = torch.Generator().manual_seed(5)
    kn = layout == "kn"
    for lead, M, N, K in (((3,), 45, 33, 40), ((2, 2), 5, 70, 200)):
        a, b, dy = exact_operands(g, lead, M, N, K, kn, DEV)
        a.requires_grad_(True), b.requires_grad_(True)
        y = mx_bmm_train(a, b, b_layout=layout, a_fmt=fmt, b_fmt=fmt, grad_fmt=fmt)
        da, db = torch.autograd.grad(y, (a, b), dy)
        for name, got, want in zip(("y", "da", "db"), (y.detach(), da, db), float64_autograd(a.detach(), b.detach(), dy, kn)):
            assert torch.equal(got.cpu(), want), (name, layout, fmt, lead)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_train_on_strided_heads(dtype):
    """[2, 2, 45, 32] with a causal mask, q / k / v as the strided heads of a packed [B, T, 3 E] projection: the forward is mx_attention
    bit for bit, the backward the composition's, and both agree with the CPU path's codes -- within the products' bound, which
    through the softmax is checked on the exact identity instead: GPU composition == GPU attention, bit for bit"""
    g = torch.Generator().manual_seed(2)
    B, h, T, d = 2, 2, 45, 32
    packed = torch.randn(B, T, 3 * h * d, generator=g).to(dtype).to(DEV).requires_grad_(True)
    q, k, v = (t.view(B, T, h, d).transpose(1, 2) for t in packed.chunk(3, -1))
    assert not q.is_contiguous()
    o = mx_attention_train(q, k, v, is_causal=True)
    with torch.no_grad():
        assert torch.equal(o, mx_attention(q, k, v, is_causal=True, out_dtype=dtype))
        assert torch.equal(o, mx_attention(q.contiguous(), k.contiguous(), v.contiguous(), is_causal=True, out_dtype=dtype))
    do = torch.randn(o.shape, generator=g).to(dtype).to(DEV)
    got, = torch.autograd.grad(o, packed, do)
    causal = torch.zeros(T, T, device=DEV).masked_fill(~torch.ones(T, T, dtype=torch.bool, device=DEV).tril(), float("-inf"))
    want, = torch.autograd.grad(composition(q, k, v, causal, ("mxfp8_e4m3",) * 3), packed, do)
    assert torch.equal(got, want) and bool(got.isfinite().all())
    ref, = torch.autograd.grad(torch.nn.functional.scaled_dot_product_attention(q.float(), k.float(), v.float(), is_causal=True), packed, do.float())
    assert (got.float() - ref.float()).norm() < 0.2 * ref.float().norm()


def test_a_captured_stochastic_step_draws_new_words_on_every_replay():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(3, 45, 40, generator=g).to(DEV).requires_grad_(True)
    b = torch.randn(3, 33, 40, generator=g).to(DEV).requires_grad_(True)
    dy = (torch.randn(3, 45, 33, generator=g) * 0.01).to(DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    kw = dict(grad_fmt="mxfp4_e2m1", grad_rounding="stochastic", seed=5, step=step)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                         # warm-up outside the capture
        torch.autograd.grad(mx_bmm_train(a, b, **kw), (a, b), dy)
    torch.cuda.current_stream().wait_stream(s)
    step.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        da, db = torch.autograd.grad(mx_bmm_train(a, b, **kw), (a, b), dy)
    graph.replay()
    first = da.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert int(step) == 2 and not torch.equal(first, da)
    step.fill_(1)                                      # the second replay ran at step 1: the eager call at that step gives its bits
    eager, _ = torch.autograd.grad(mx_bmm_train(a, b, **kw), (a, b), dy)
    assert torch.equal(eager, da) and int(step) == 2
