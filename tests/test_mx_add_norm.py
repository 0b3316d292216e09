"""The residual add fused into the MX norm family, on the CPU: ``mx_add_norm_quantize`` against the composition ``h = x + residual``
(one float32 addition, rounded once to the stream's dtype) -> ``mx_norm_quantize(h)``, ``mx_norm_backward(dresidual=)`` against the
float32 definition plus ``dresidual`` rounded once, ``mx_add_norm_linear`` against autograd through the composition, the layers, and the
two new descriptors (no GPU needed: everything refused is refused before a launch).  The GPU twins are in ``test_mx_add_norm_gpu.py``;
the checks that run on both are written once, on a device argument, and imported there."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn as nn

import mx_norm_bwd_ref as BR
import mx_norm_ref as NR
import qsparse_amd as qs
import test_mx_norm as T
from mx_norm_ref import DTS, EPS, FMTS, NORMS, WB, same
from qsparse_amd import (MXAddNormLinear, MXLayerNorm, MXLinear, MXRMSNorm, MXTrainAddNormLinear, MXTrainNormLinear, _hip,
                         mx_add_norm_linear, mx_add_norm_quantize, mx_norm_backward, mx_norm_linear, mx_norm_quantize)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = (1, 33, 129), (1, 31, 32, 96, 520)
PAIRS = tuple((xdt, rdt) for xdt in DTS for rdt in DTS)
NAMES = ("h", "codes", "scales", "col_codes", "col_scales", "rstd", "mean")


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def to(dev, ts):
    return [t if t is None else t.to(dev) for t in ts]


def add_inputs(seed, R, C, xdt, rdt, has_w=True, has_b=True):
    """(x, residual, w, b): the stream as mx_norm_ref.inputs draws an x, the branch output a randn of a quarter of the row's scale"""
    res, w, b = NR.inputs(seed, R, C, rdt, has_w, has_b)
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.randn(R, C, generator=g) * res.float().abs().amax(-1, keepdim=True).clamp_min(2.0 ** -8) / 4).to(xdt)
    return x, res, w, b


def composition(x, res, w, b, **kw):
    """what the fused call must equal: h by the issue's expression, then the existing function on h (on the tensors' device)"""
    h = (x.float() + res.float()).to(res.dtype)
    return (h,) + tuple(mx_norm_quantize(h, w, b, **kw))


def agree(got, want, what):
    assert len(got) == len(want), what
    for name, a, r in zip(NAMES, got, want):
        assert (a is None) == (r is None), (name,) + what
        assert a is None or same(a.cpu(), r.cpu()), (name,) + what


# ---- test 1: the fused call is the composition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdt,rdt", PAIRS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_add_norm_quantize_is_the_composition(norm, xdt, rdt):
    """every R x C x (weight, bias); the formats walk as in test_mx_norm.py"""
    i = 0
    for R in ROWS:
        for C in COLS:
            for has_w, has_b in WB:
                x, res, w, b = add_inputs(1000 * R + C, R, C, xdt, rdt, has_w, has_b)
                kw = dict(norm=norm, eps=EPS, fmt=FMTS[i % 5], col_fmt=FMTS[(i + 2) % 5], return_stats=True)
                i += 1
                got = mx_add_norm_quantize(x, res, w, b, **kw)
                assert len(got) == 7 and got[0].dtype == rdt and got[0].shape == (R, C)
                agree(got, composition(x, res, w, b, **kw), (R, C, has_w, has_b, kw["fmt"]))
                assert len(mx_add_norm_quantize(x, res, w, b, norm=norm, eps=EPS, fmt=kw["fmt"])) == 3


def test_leading_dimensions():
    x, res, w, b = add_inputs(3, 6 * 33, 96, torch.bfloat16, torch.float32)
    kw = dict(norm="layer", fmt="mxfp6_e2m3", col_fmt="mxfp8_e5m2", return_stats=True)
    flat = mx_add_norm_quantize(x, res, w, b, **kw)
    lead = mx_add_norm_quantize(x.view(6, 33, 96), res.view(6, 33, 96), w, b, **kw)
    assert lead[0].shape == (6, 33, 96) and lead[0].dtype == torch.float32 and lead[1].shape == (6, 33, 96)
    assert lead[2].shape == (6, 33, 3) and lead[3].shape == (96, 198) and lead[5].shape == lead[6].shape == (6, 33)
    assert all(same(a.reshape(r.shape), r) for a, r in zip(lead, flat))


def rounding_case(R=33, C=96):
    """bf16 x and residual whose float32 sum no bf16 holds: residual in [1, 2) (8 significant bits), x a multiple of 2^-12 below 2^-4
    -- the sum needs up to 13 bits.  A constant offset keeps the sum's rounding error from averaging out of the statistics"""
    g = torch.Generator().manual_seed(11)
    res = (1 + torch.randint(0, 128, (R, C), generator=g) / 128.0).to(torch.bfloat16)
    x = (torch.randint(1, 16, (R, C), generator=g) * 2.0 ** -12 * 17).to(torch.bfloat16)
    return x, res


def check_rounding_shows(dev):
    """the statistics are the ROUNDED h's: those of the unrounded float32 sum differ in at least one row, so a kernel that sums before
    it rounds cannot pass"""
    x, res = rounding_case()
    s32 = x.float() + res.float()
    h = s32.to(torch.bfloat16)
    assert bool((h.float() != s32).any())                                   # the sum is not representable
    for norm in NORMS:
        rounded = mx_norm_quantize(h, norm=norm, eps=EPS, return_stats=True)
        unrounded = mx_norm_quantize(s32, norm=norm, eps=EPS, return_stats=True)
        assert bool((rounded[2] != unrounded[2]).any()), norm               # rstd differs for at least one row
        got = mx_add_norm_quantize(x.to(dev), res.to(dev), norm=norm, eps=EPS, return_stats=True)
        agree(got, (h,) + tuple(rounded), (norm,))


def test_rounding_comes_before_the_sums():
    check_rounding_shows("cpu")


def check_special_values(dev, xdt, rdt, norm):
    """a NaN in x only and an Inf in residual only: the whole row is NaN (0xFF scale bytes, zero codes, NaN rstd) and h holds the NaN /
    the Inf; an all-zero row gives y = b"""
    R, C = 70, 96
    x, res, w, b = add_inputs(17, R, C, xdt, rdt)
    x[5, 40] = float("nan")
    res[37, 70] = float("inf")
    x[10] = 0
    res[10] = 0
    kw = dict(norm=norm, eps=EPS, fmt="mxfp8_e4m3", col_fmt="mxfp6_e3m2", return_stats=True)
    got = [t if t is None else t.cpu() for t in mx_add_norm_quantize(*to(dev, (x, res, w, b)), **kw)]
    agree(got, composition(x, res, w, b, **kw), (xdt, rdt, norm))
    h, codes, scales, cc, cs, rstd, _ = got
    assert bool(h[5, 40].isnan()) and bool(h[37, 70].isinf()) and h[5].isnan().sum() == 1 and h[37].isinf().sum() == 1
    bad = torch.zeros(R, dtype=torch.bool)
    bad[5] = bad[37] = True
    assert bool((scales[bad] == 255).all()) and bool((scales[~bad] != 255).all()) and bool((codes[bad] == 0).all())
    assert bool(rstd[bad].isnan().all()) and bool(rstd[~bad].isfinite().all())
    assert bool((cs[:, :2] == 255).all()) and bool((cs[:, 2] != 255).all())
    assert bool((h[10] == 0).all())
    rc, rs, _, _ = NR.ref_quant(b[None, :].clone(), "mxfp8_e4m3")
    assert torch.equal(codes[10:11], rc) and torch.equal(scales[10:11], rs)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("xdt,rdt", PAIRS, ids=str)
def test_special_values_cpu(xdt, rdt, norm):
    check_special_values("cpu", xdt, rdt, norm)


# ---- test 2: mx_norm_backward(dresidual=) ----------------------------------------------------------------------------------------------
def dres_of(R, C, dtype):
    g = torch.Generator().manual_seed(31 * R + C)
    return torch.randn(R, C, generator=g).to(dtype)


def run_bwd(dev, case, norm, dres, **kw):
    dxhat, x, rstd, mean, w = to(dev, case)
    return to("cpu", mx_norm_backward(dxhat, x, rstd, mean, w, norm=norm, dresidual=None if dres is None else dres.to(dev), **kw))


def want_bwd(key, dres):
    """the definition's float32 dx plus dresidual, rounded once; dweight and dbias as they were"""
    ref = BR.reference(*key)
    return ((ref[0] + dres.float()).to(key[2]), ref[1], ref[2])


@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_backward_with_dresidual_is_the_definition(norm, dtype):
    for R, C in BR.SHAPES[:5]:
        for has_w in (True, False):
            key = (R, C, dtype, norm, has_w)
            dres = dres_of(R, C, dtype)
            got = run_bwd("cpu", BR.case(*key), norm, dres)
            for name, a, r in zip(("dx", "dweight", "dbias"), got, want_bwd(key, dres)):
                assert same(a, r), (name, R, C, has_w)
            plain = run_bwd("cpu", BR.case(*key), norm, None)
            assert all(same(a, r) for a, r in zip(plain, (BR.reference(*key)[0].to(dtype),) + tuple(BR.reference(*key)[1:])))


def check_one_rounding(dev):
    """bf16: dx + dresidual rounded ONCE is not (dx rounded) + dresidual rounded again"""
    key = (129, 96, torch.bfloat16, "layer", True)
    dres = dres_of(129, 96, torch.bfloat16)
    got = run_bwd(dev, BR.case(*key), "layer", dres)[0]
    f32 = BR.reference(*key)[0]
    assert same(got, (f32 + dres.float()).to(torch.bfloat16))
    twice = (f32.to(torch.bfloat16).float() + dres.float()).to(torch.bfloat16)
    assert not same(got, twice)


def test_one_rounding_cpu():
    check_one_rounding("cpu")


def check_needs_with_dresidual(dev, key=(130, 100, torch.float16, "layer")):
    """every subset of needs that has dx: what is not asked for is None, what is asked for does not change with the subset; dweight
    and dbias do not see dresidual"""
    case, dres = BR.case(*key), dres_of(key[0], key[1], key[2])
    full = run_bwd(dev, case, key[3], dres)
    without = run_bwd(dev, case, key[3], None)
    assert same(full[1], without[1]) and same(full[2], without[2]) and not same(full[0], without[0])
    for bits in range(8):
        needs = dict(need_dx=bool(bits & 1), need_dweight=bool(bits & 2), need_dbias=bool(bits & 4))
        if not needs["need_dx"]:
            with pytest.raises(ValueError, match="needs need_dx"):
                run_bwd(dev, case, key[3], dres, **needs)
            got = run_bwd(dev, case, key[3], None, **needs)
            want = without
        else:
            got = run_bwd(dev, case, key[3], dres, **needs)
            want = full
        for need, a, r in zip(needs.values(), got, want):
            assert (a is None) == (not need), bits
            assert a is None or same(a, r), bits


def test_needs_with_dresidual_cpu():
    check_needs_with_dresidual("cpu")
    lead = BR.case(300, 520, torch.bfloat16, "layer")
    dres = dres_of(300, 520, torch.bfloat16)
    flat = mx_norm_backward(*lead, norm="layer", dresidual=dres)[0]
    dxhat, x, rstd, mean, w = lead
    got = mx_norm_backward(dxhat.view(3, 100, 520), x.view(3, 100, 520), rstd.view(3, 100), mean.view(3, 100), w, norm="layer",
                           dresidual=dres.view(3, 100, 520))[0]
    assert got.shape == (3, 100, 520) and same(got.reshape(300, 520), flat)


def test_refusals():
    dxhat, x, rstd, mean, w = BR.case(129, 96, torch.float32, "layer")
    with pytest.raises(ValueError, match="dresidual has shape"):
        mx_norm_backward(dxhat, x, rstd, mean, w, norm="layer", dresidual=x[:, :64])
    with pytest.raises(TypeError, match="dresidual must have x's dtype"):
        mx_norm_backward(dxhat, x, rstd, mean, w, norm="layer", dresidual=x.bfloat16())
    with pytest.raises(TypeError, match="dresidual must be a tensor"):
        mx_norm_backward(dxhat, x, rstd, mean, w, norm="layer", dresidual=1.0)
    with pytest.raises(ValueError, match="x is on cpu but dresidual on meta"):
        mx_norm_backward(dxhat, x, rstd, mean, w, norm="layer", dresidual=x.to("meta"))
    with pytest.raises(ValueError, match="needs need_dx"):
        mx_norm_backward(dxhat, x, rstd, mean, w, norm="layer", dresidual=x, need_dx=False)
    with pytest.raises(ValueError, match="residual has shape"):
        mx_add_norm_quantize(x, x[:, :64])
    with pytest.raises(TypeError, match="residual must be one of"):
        mx_add_norm_quantize(x, x.double())
    with pytest.raises(TypeError, match="residual must be a tensor"):
        mx_add_norm_quantize(x, None)
    with pytest.raises(ValueError, match="x is on cpu but residual on meta"):
        mx_add_norm_quantize(x, x.to("meta"))
    with pytest.raises(ValueError, match="residual has shape"):
        mx_add_norm_linear(x, x[:64], None, None, torch.randn(8, 96))
    with pytest.raises(ValueError, match="unknown norm_backward"):
        mx_add_norm_linear(x, x, None, None, torch.randn(8, 96), norm_backward="aten")
    with pytest.raises(RuntimeError, match="inference layer"):
        MXRMSNorm(96)(x, x.clone().requires_grad_(True))


# ---- test 3: mx_add_norm_linear ----------------------------------------------------------------------------------------------------------
def _leaves(ts, req=None):
    req = [True] * len(ts) if req is None else req
    return [None if t is None else t.clone().requires_grad_(r) for t, r in zip(ts, req)]


def _grads(ts):
    return [None if t is None else t.grad for t in ts]


def check_add_norm_linear_f32(dev, shape, N, norm, mode):
    """float32: y, h and every gradient equal, bit for bit, autograd through h = residual + x; mx_norm_linear(h, norm_backward=mode),
    with a loss that also uses h (its gradient `dh_in` reaches h next to the norm's)"""
    x, nw, nb, W, b, dy = T._train_case(dev, shape, N, norm, 6)
    g = torch.Generator().manual_seed(5)
    res, dh = torch.randn(*shape, generator=g).to(dev) * 2, torch.randn(*shape, generator=g).to(dev)
    kw = dict(norm=norm, eps=EPS, norm_backward=mode)

    a = _leaves((x, res, nw, nb, W, b))
    y, h = mx_add_norm_linear(*a, **kw)
    torch.autograd.backward((y, h), (dy, dh))

    r = _leaves((x, res, nw, nb, W, b))
    h_ref = r[1] + r[0]
    y_ref = mx_norm_linear(h_ref, *r[2:], **kw)
    torch.autograd.backward((y_ref, h_ref), (dy, dh))
    assert same(y, y_ref) and same(h, h_ref)
    for name, p, q in zip(("x", "residual", "norm_weight", "norm_bias", "weight", "bias"), _grads(a), _grads(r)):
        assert (p is None) == (q is None) and (p is None or same(p, q)), (name, mode)

    # dh_in None: nobody used h
    a = _leaves((x, res, nw, nb, W, b))
    mx_add_norm_linear(*a, **kw)[0].backward(dy)
    r = _leaves((x, res, nw, nb, W, b))
    mx_norm_linear(r[1] + r[0], *r[2:], **kw).backward(dy)
    assert all((p is None) == (q is None) and (p is None or same(p, q)) for p, q in zip(_grads(a), _grads(r))), mode
    # only h used: the stream's gradient passes through, the product's are those of a zero dy
    a = _leaves((x, res, nw, nb, W, b))
    mx_add_norm_linear(*a, **kw)[1].backward(dh)
    assert same(a[0].grad, dh) and same(a[1].grad, dh) and bool((a[4].grad == 0).all())


@pytest.mark.parametrize("mode", ("fused", "torch"))
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape,N", [((2, 33, 96), 64), ((129, 128), 32)])
def test_add_norm_linear_f32_cpu(shape, N, norm, mode):
    check_add_norm_linear_f32("cpu", shape, N, norm, mode)


def check_add_norm_linear_mixed(dev, norm, mode, xdt=torch.bfloat16, rdt=torch.bfloat16):
    """bf16 (and a float32 stream with a bf16 branch): the forward bits are mx_norm_linear(h)'s; dh is the norm's float32 input gradient
    plus dh_in, rounded once; the gradient of x is dh in x's dtype; x or residual not requiring grad"""
    shape, N = (129, 96), 64
    x, nw, nb, W, b, dy = T._train_case(dev, shape, N, norm, 9)
    g = torch.Generator().manual_seed(6)
    res, dh_in = (torch.randn(*shape, generator=g) * 2).to(dev).to(rdt), torch.randn(*shape, generator=g).to(dev).to(rdt)
    x, dy = x.to(xdt), dy.to(rdt)
    kw = dict(norm=norm, eps=EPS, norm_backward=mode)
    a = _leaves((x, res, nw, nb, W, b))
    y, h = mx_add_norm_linear(*a, **kw)
    torch.autograd.backward((y, h), (dy, dh_in))
    h_want = (x.float() + res.float()).to(rdt)
    r = _leaves((h_want, nw, nb, W, b))
    y_want = mx_norm_linear(*r, **kw)
    y_want.backward(dy)
    assert y.dtype == rdt and h.dtype == rdt and same(y, y_want) and same(h, h_want)
    assert all((p is None) == (q is None) and (p is None or same(p, q)) for p, q in zip(_grads(a)[2:], _grads(r)[1:]))

    # the float32 definition of dh: the norm's float32 dx from mx_linear's float32 input gradient, + dh_in, one rounding
    K = shape[-1]
    rstd, mean = mx_norm_quantize(h_want, nw, nb, norm=norm, eps=EPS, return_stats=True)[-2:]
    yr = NR.ref_y(h_want.cpu(), nw.cpu(), None if nb is None else nb.cpu(), norm)[0].to(dev).to(rdt).requires_grad_(True)
    qs.mx_linear(yr, W, b).backward(dy)
    dxhat = yr.grad.float()
    if rdt == torch.float32:            # (a two-byte y rounds dxhat once more than the fused path does: compared in float32 only)
        if mode == "fused":
            f32 = BR.ref_backward(dxhat.cpu(), h_want.cpu(), rstd.cpu(), None if mean is None else mean.cpu(), nw.cpu())[0].to(dev)
        else:
            f32 = NR.norm_backward_ref(dxhat, h_want, rstd, mean, nw, norm)[0]
        assert same(a[1].grad, (f32 + dh_in.float()).to(rdt))
    assert a[0].grad.dtype == xdt and a[1].grad.dtype == rdt and same(a[0].grad, a[1].grad.to(xdt))

    for req in ((True, False), (False, True), (False, False)):
        p = _leaves((x, res, nw, nb, W, b), list(req) + [True] * 4)
        y2, h2 = mx_add_norm_linear(*p, **kw)
        torch.autograd.backward((y2, h2) if h2.requires_grad else (y2,), (dy, dh_in) if h2.requires_grad else (dy,))
        for got, want, asked in zip(_grads(p)[:2], _grads(a)[:2], req):
            assert (got is not None) == asked and (got is None or same(got, want)), req
        assert same(p[4].grad, a[4].grad) and same(p[2].grad, a[2].grad)


def bf16_dh_definition(dev, norm):
    """bf16 throughout, fused: dh equals mx_norm_backward's float32 definition on the float32 dxhat the backward product hands out,
    plus dh_in, rounded once -- dxhat taken from the function's own products (float32 out of mx_matmul)"""
    shape, N = (129, 96), 64
    x, nw, nb, W, b, dy = T._train_case(dev, shape, N, norm, 9)
    g = torch.Generator().manual_seed(6)
    res, dh_in = (torch.randn(*shape, generator=g) * 2).to(dev).bfloat16(), torch.randn(*shape, generator=g).to(dev).bfloat16()
    x, dy = x.bfloat16(), dy.bfloat16()
    a = _leaves((x, res, nw, nb, W, b))
    y, h = mx_add_norm_linear(*a, norm=norm, eps=EPS)
    torch.autograd.backward((y, h), (dy, dh_in))
    g_row, g_rs, _, _ = qs.mx_quantize_2way(dy, "mxfp8_e5m2", None)
    _, _, w_col, w_cs = qs.mx_quantize_2way(W, None, "mxfp8_e4m3")
    dxhat = qs.mx_matmul(g_row, g_rs, "mxfp8_e5m2", w_col, w_cs, "mxfp8_e4m3", None, torch.float32)
    hd = h.detach()
    rstd, mean = mx_norm_quantize(hd, nw, nb, norm=norm, eps=EPS, return_stats=True)[-2:]
    f32 = BR.ref_backward(*to("cpu", (dxhat, hd, rstd, mean, nw)))[0]
    assert same(a[1].grad.cpu(), (f32 + dh_in.cpu().float()).to(torch.bfloat16))
    assert same(a[0].grad, a[1].grad)


@pytest.mark.parametrize("mode", ("fused", "torch"))
@pytest.mark.parametrize("norm", NORMS)
def test_add_norm_linear_dtypes_cpu(norm, mode):
    check_add_norm_linear_mixed("cpu", norm, mode)
    check_add_norm_linear_mixed("cpu", norm, mode, torch.bfloat16, torch.float32)
    if mode == "fused":
        bf16_dh_definition("cpu", norm)


# ---- the step on operands whose every sum is exact ----------------------------------------------------------------------------------------
STEP_NAMES = ("y", "h", "dx", "dresidual", "d norm_weight", "d norm_bias", "dW", "db")


def _pick(g, values, *shape):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)]


def exact_step_case(norm, xdt, R=129, K=128, N=64):
    """(x, residual, norm_weight, norm_bias, weight, bias, dy, dh_in) of a float32 stream for which EVERY sum of the step is exact in
    float32, so that its result does not depend on the order of any reduction.  That is what a comparison of a whole step between the
    GPU and the CPU needs: ``mx_matmul`` accumulates by the scaled MFMA on the one and by torch on the other (tests/test_mx_train_gpu.py
    holds the products to a bound against float64 for that reason), and torch's ``mean(-1)`` / ``sum(0)`` -- ``norm_backward="torch"``,
    db -- have an order per device as well; on drawn operands the two devices differ in most elements of y already, for
    ``mx_norm_linear`` as for the new function.  Here:
      * h = +-2^k, k in 0 .. 3 per row, half of a row's signs each: mean = 0, ms = 4^k, eps = 0, rstd = 2^-k, xhat = +-1;
        residual = integers in [-8, 8], x = h - residual (exact in bfloat16 too: |x| <= 16);
      * norm_weight in {1, 1.5, 2, 3}, norm_bias in {-1, 0, 1}: the norm's output is a multiple of 0.5 up to 4, four significant
        bits, exact in mxfp8_e4m3 in a block along either axis; weight in +-{0.5, 1, 1.5}, bias integers; dy in +-{0.5, 1, 1.5, 2, 3},
        three significant bits, exact in mxfp8_e5m2; dh_in integers;
      * so the products are sums of multiples of 0.25 below 2^10; c1 and c2 are such sums over K = 128, a power of two (the division,
        and a multiplication by 1 / K in its place, are exact); dx = rstd (g - xhat c1 - c2) + dh_in is a multiple of 2^-13 below 2^10.
    R = 129: a second row tile and a ragged last block along R; K = 128, N = 64: the VEC route"""
    g = torch.Generator().manual_seed(2024)
    k = torch.randint(0, 4, (R, 1), generator=g)
    signs = torch.cat([torch.ones(R, K // 2), -torch.ones(R, K // 2)], 1)
    signs = torch.gather(signs, 1, torch.rand(R, K, generator=g).argsort(1))
    h = signs * torch.exp2(k.float())
    res = torch.randint(-8, 9, (R, K), generator=g).float()
    x = (h - res).to(xdt)
    nw = _pick(g, (1.0, 1.5, 2.0, 3.0), K)
    nb = _pick(g, (-1.0, 0.0, 1.0), K) if norm == "layer" else None
    W = _pick(g, (-1.5, -1.0, -0.5, 0.5, 1.0, 1.5), N, K)
    b = torch.randint(-2, 3, (N,), generator=g).float()
    dy = _pick(g, (-3.0, -2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0, 3.0), R, N)
    dh = torch.randint(-4, 5, (R, K), generator=g).float()
    assert same(x.float() + res, h)
    return x, res, nw, nb, W, b, dy, dh


def exact_step(dev, norm, mode, xdt, with_dh=True):
    x, res, nw, nb, W, b, dy, dh = to(dev, exact_step_case(norm, xdt))
    leaves = _leaves((x, res, nw, nb, W, b))
    y, h = mx_add_norm_linear(*leaves, norm=norm, eps=0.0, norm_backward=mode)
    torch.autograd.backward((y, h) if with_dh else (y,), (dy, dh) if with_dh else (dy,))
    return [y.detach(), h.detach()] + _grads(leaves)


@pytest.mark.parametrize("xdt", (torch.float32, torch.bfloat16), ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_exact_step_case_is_exact(norm, xdt):
    """the premises of exact_step_case, without a GPU: the float32 y is the float64 one; the two norm backwards, whose sums run in
    different orders, give the same bits; and the case is not trivial -- dh_in changes dx, nothing is constant"""
    x, res, nw, nb, W, b, dy, dh = exact_step_case(norm, xdt)
    fused, torch_ = exact_step("cpu", norm, "fused", xdt), exact_step("cpu", norm, "torch", xdt)
    for name, p, q in zip(STEP_NAMES, fused, torch_):
        assert (p is None) == (q is None) and (p is None or same(p, q)), name
    y, h = fused[:2]
    hat = h.double() / h.abs().double()
    yn = hat * nw.double() + (0 if nb is None else nb.double())
    assert torch.equal(y.double(), yn @ W.double().T + b.double())
    dxhat = dy.double() @ W.double()
    gg = dxhat * nw.double()
    inner = gg - hat * (gg * hat).mean(-1, keepdim=True) - (gg.mean(-1, keepdim=True) if norm == "layer" else 0)
    dres = inner / h.abs().double() + dh.double()
    assert torch.equal(fused[3].double(), dres) and same(fused[2], fused[3].to(xdt))
    assert torch.equal(fused[4].double(), (dxhat * hat).sum(0)) and torch.equal(fused[6].double(), dy.double().T @ yn)
    assert torch.equal(fused[7].double(), dy.double().sum(0)) and (nb is None or torch.equal(fused[5].double(), dxhat.sum(0)))
    assert not same(fused[3], exact_step("cpu", norm, "fused", xdt, with_dh=False)[3])
    assert all(t.unique().numel() > 8 for t in (y, fused[3], fused[4], fused[6]))


# ---- test 4: layers ------------------------------------------------------------------------------------------------------------------------
def check_layers(dev):
    """MXTrainAddNormLinear shares the float modules' parameters, has MXTrainNormLinear's state_dict keys and defaults to the fused
    backward; to_inference() gives the same (y, h) bits; MXRMSNorm / MXLayerNorm with a residual"""
    torch.manual_seed(8)
    for fnorm in (nn.RMSNorm(96, eps=1e-5), nn.LayerNorm(96), nn.LayerNorm(96, bias=False), nn.RMSNorm(96, elementwise_affine=False)):
        fnorm, lin = fnorm.to(dev), nn.Linear(96, 64).to(dev)
        for p in fnorm.parameters():
            nn.init.normal_(p, 1.0, 0.25)
        layer = MXTrainAddNormLinear.from_float(fnorm, lin, x_fmt="mxfp6_e2m3")
        twin = MXTrainNormLinear.from_float(fnorm, lin, x_fmt="mxfp6_e2m3")
        assert isinstance(layer, MXTrainAddNormLinear) and layer.norm_backward == "fused" and twin.norm_backward == "torch"
        assert layer.weight is lin.weight and layer.bias is lin.bias and layer.norm_weight is fnorm.weight
        assert list(layer.state_dict().keys()) == list(twin.state_dict().keys())
        x, res = torch.randn(2, 33, 96).to(dev), torch.randn(2, 33, 96).to(dev)
        y, h = layer(x, res)
        assert same(h, res + x) and same(y, twin(res + x))
        inf = layer.to_inference()
        head = MXRMSNorm if isinstance(fnorm, nn.RMSNorm) else MXLayerNorm
        assert isinstance(inf, MXAddNormLinear) and isinstance(inf.norm, head) and isinstance(inf.linear, MXLinear)
        yi, hi = inf(x, res)
        assert same(yi, y.detach()) and same(hi, h.detach())
        # the norm layers' residual form
        m = head.from_float(fnorm, "mxfp6_e2m3")
        act, hm = m(x, res)
        eps = float(torch.finfo(torch.float32).eps) if fnorm.eps is None else fnorm.eps
        want = mx_add_norm_quantize(x, res, fnorm.weight, getattr(fnorm, "bias", None), norm=m.norm, eps=eps, fmt="mxfp6_e2m3")
        assert isinstance(act, qs.MXActivation) and same(hm, want[0]) and same(act.codes, want[1]) and same(act.scales, want[2])
        assert isinstance(m(x), qs.MXActivation)                            # without a residual: as before
    assert MXTrainAddNormLinear(96, 8, norm="layer").norm_backward == "fused"
    assert MXTrainAddNormLinear(96, 8, norm_backward="torch").norm_backward == "torch"
    layer = MXTrainAddNormLinear(96, 64, norm="layer").to(dev)
    xg, rg = torch.randn(40, 96).to(dev).requires_grad_(True), torch.randn(40, 96).to(dev).requires_grad_(True)
    y, h = layer(xg, rg)
    (y.sum() + (h * h).sum()).backward()
    assert same(xg.grad, rg.grad) and all(p.grad is not None for p in layer.parameters())


def test_layers_cpu():
    check_layers("cpu")


# ---- test 5: the descriptors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct,cname", [(_hip.MxAddNormQuantArgs, "qs_mx_add_norm_quant_args"), (_hip.MxNormBwdResArgs, "qs_mx_norm_bwd_res_args")])
def test_descriptor_struct_has_the_headers_layout(tmp_path, ct, cname):
    """the ctypes mirrors against `sizeof` / `offsetof` of the header itself (gcc: the header is plain C)"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "qsparse_hip.h")}"', 'int main(void) {',
             f'printf("%zu", sizeof({cname}));']
    lines += [f'printf(" %zu", offsetof({cname}, {fname}));' for fname, _ in ct._fields_]
    lines += ['printf("\\n");', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    size, *offsets = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(ct)
    assert [int(o) for o in offsets] == [getattr(ct, f).offset for f, _ in ct._fields_]
    assert ct._fields_[0][0] == "struct_size"


def test_the_old_backward_descriptor_is_a_prefix():
    """qs_mx_norm_bwd_args stays byte-identical: the new descriptor is it plus one pointer"""
    old, new = _hip.MxNormBwdArgs, _hip.MxNormBwdResArgs
    assert ctypes.sizeof(new) == ctypes.sizeof(old) + 8 and new._fields_[:-1] == old._fields_
    assert [getattr(new, f).offset for f, _ in old._fields_] == [getattr(old, f).offset for f, _ in old._fields_]


def add_args(**kw):
    a = _hip.MxAddNormQuantArgs()
    a.struct_size = ctypes.sizeof(a)
    a.mode, a.row_format, a.col_format, a.xdt, a.rdt, a.eps = 1, 0, 1, _hip.F32, _hip.F32, 1e-6
    a.x, a.residual, a.h, a.weight, a.bias = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.row_codes, a.row_scales, a.col_codes, a.col_scales, a.rstd, a.mean = 0x6000, 0x7000, 0x8000, 0x9000, 0xA000, 0xB000
    a.R, a.C = 129, 96
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_add_norm_checks_in_the_documented_order():
    """QS_ERR_ARG (-2) before QS_ERR_DTYPE (-1) before QS_ERR_ALIGN (-3); the route of what is accepted.  Only the route export is
    called on descriptors that would launch: nothing is enqueued here"""
    lib = _hip.load()
    route = lambda a: lib.qs_mx_add_norm_quant_route(ctypes.byref(a))
    VEC, PLAIN = _hip.MX_NORM_ROUTE_VEC, _hip.MX_NORM_ROUTE_PLAIN
    assert lib.qs_mx_add_norm_quant_v(None) == -2 and lib.qs_mx_add_norm_quant_route(None) == -2
    short = add_args(struct_size=2)
    assert lib.qs_mx_add_norm_quant_v(ctypes.byref(short)) == -2 and route(short) == -2
    old_size = add_args(struct_size=ctypes.sizeof(_hip.MxNormQuantArgs))    # a descriptor without residual / h: they read as NULL
    assert route(old_size) == -2
    assert route(add_args()) == VEC
    for bad in (dict(mode=2), dict(x=None), dict(residual=None), dict(h=None), dict(row_codes=None), dict(row_scales=None),
                dict(rstd=None), dict(mean=None), dict(row_format=5), dict(col_format=7), dict(col_codes=None), dict(col_scales=None),
                dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(R=-1), dict(C=-1)):
        a = add_args(xdt=7, rdt=9, weight=0x4002, **bad)                    # later failures as well: the earlier check answers
        assert route(a) == -2 and lib.qs_mx_add_norm_quant_v(ctypes.byref(a)) == -2, bad
    assert route(add_args(mode=0, mean=None)) == VEC                          # rms mode does not look at mean
    assert route(add_args(col_format=-1, col_codes=None, col_scales=None)) == VEC
    for bad in (dict(xdt=7), dict(rdt=-1), dict(rdt=3)):
        a = add_args(x=0x1001, residual=0x2001, **bad)
        assert route(a) == -1 and lib.qs_mx_add_norm_quant_v(ctypes.byref(a)) == -1, bad
    for bad in (dict(x=0x1002), dict(residual=0x2002), dict(h=0x3002), dict(weight=0x4002), dict(bias=0x5001), dict(rstd=0xA002),
                dict(mean=0xB001), dict(xdt=_hip.BF16, x=0x1001), dict(rdt=_hip.F16, residual=0x2001), dict(rdt=_hip.BF16, h=0x3001)):
        a = add_args(**bad)
        assert route(a) == -3 and lib.qs_mx_add_norm_quant_v(ctypes.byref(a)) == -3, bad
    assert route(add_args(R=1 << 40, C=1 << 40)) == -2                        # R * C beyond 64 bits
    for empty in (dict(R=0), dict(C=0)):
        a = add_args(**empty)
        assert route(a) == 0 and lib.qs_mx_add_norm_quant_v(ctypes.byref(a)) == 0
    # the route: VEC needs C % 32 == 0 and x, residual, h, weight, bias at 16 bytes
    for plain in (dict(C=100), dict(x=0x1004), dict(residual=0x2008), dict(h=0x3004), dict(weight=0x4004), dict(bias=0x5008),
                  dict(xdt=_hip.BF16, x=0x1002), dict(rdt=_hip.BF16, residual=0x2002), dict(rdt=_hip.F16, h=0x3002)):
        assert route(add_args(**plain)) == PLAIN, plain
    assert route(add_args(weight=None, bias=None, xdt=_hip.F16, rdt=_hip.BF16)) == VEC
    assert route(add_args(row_codes=0x6001, col_codes=0x8001, row_scales=0x7001)) == VEC     # the outputs' bases do not choose it


def res_args(**kw):
    a = _hip.MxNormBwdResArgs()
    a.struct_size = ctypes.sizeof(a)
    a.mode, a.xdt, a.gdt = 1, _hip.F32, _hip.F32
    a.dxhat, a.x, a.weight, a.rstd, a.mean = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.dx, a.dweight, a.dbias, a.dresidual = 0x6000, 0x7000, 0x8000, 0x9000
    a.workspace, a.workspace_bytes = 0x10000, 1 << 40
    a.R, a.C = 129, 96
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_backward_res_checks_in_the_documented_order():
    """qs_mx_norm_bwd_v's checks in its order, with dresidual's among them"""
    lib = _hip.load()
    route = lambda a: lib.qs_mx_norm_bwd_res_route(ctypes.byref(a))
    VEC, PLAIN = _hip.MX_NORM_BWD_ROUTE_VEC, _hip.MX_NORM_BWD_ROUTE_PLAIN
    assert lib.qs_mx_norm_bwd_res_v(None) == -2 and lib.qs_mx_norm_bwd_res_route(None) == -2
    short = res_args(struct_size=2)
    assert lib.qs_mx_norm_bwd_res_v(ctypes.byref(short)) == -2 and route(short) == -2
    assert route(res_args()) == VEC and route(res_args(dresidual=None)) == VEC
    # the old descriptor's size: dresidual reads as NULL, the call is qs_mx_norm_bwd_v's
    assert route(res_args(struct_size=ctypes.sizeof(_hip.MxNormBwdArgs), dresidual=0x9002)) == VEC
    for bad in (dict(mode=2), dict(dxhat=None), dict(x=None), dict(rstd=None), dict(mean=None), dict(dx=None, dweight=None, dbias=None),
                dict(dx=None), dict(R=-1), dict(C=-1)):
        a = res_args(xdt=7, workspace=None, **bad)
        assert route(a) == -2 and lib.qs_mx_norm_bwd_res_v(ctypes.byref(a)) == -2, bad
    assert route(res_args(dx=None, dresidual=None)) == VEC                    # without dresidual dx stays optional
    for bad in (dict(xdt=7), dict(gdt=-1)):
        a = res_args(dresidual=0x9001, workspace_bytes=0, **bad)
        assert route(a) == -1 and lib.qs_mx_norm_bwd_res_v(ctypes.byref(a)) == -1, bad
    for bad in (dict(dresidual=0x9002), dict(xdt=_hip.BF16, dresidual=0x9001), dict(x=0x2002), dict(dx=0x6002), dict(workspace=0x10008)):
        a = res_args(workspace_bytes=0, **bad)
        assert route(a) == -3 and lib.qs_mx_norm_bwd_res_v(ctypes.byref(a)) == -3, bad
    need = _hip.mx_norm_bwd_plan(129, 96, "layer", True, True)
    for bad in (dict(workspace=None), dict(workspace_bytes=need - 1)):
        a = res_args(**bad)
        assert route(a) == -4 and lib.qs_mx_norm_bwd_res_v(ctypes.byref(a)) == -4, bad
    assert route(res_args(workspace_bytes=need)) == VEC
    assert route(res_args(dresidual=0x9004)) == PLAIN and route(res_args(xdt=_hip.BF16, dresidual=0x9002)) == PLAIN
    assert route(res_args(C=100)) == PLAIN
    for empty in (dict(R=0), dict(C=0)):
        a = res_args(workspace=None, workspace_bytes=0, **empty)
        assert route(a) == 0 and lib.qs_mx_norm_bwd_res_v(ctypes.byref(a)) == 0
