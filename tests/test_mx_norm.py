"""``mx_norm.py`` on the CPU: ``mx_norm_quantize`` against the definition restated in ``mx_norm_ref.py``, the definition's float32 ``y``
against float64, the inference layers, and ``mx_norm_linear`` / ``MXTrainNormLinear`` forward and backward.  The GPU twins are in
``test_mx_norm_gpu.py``; the layer and training checks are written once, on a device argument, and imported there."""
import copy

import pytest
import torch
import torch.nn as nn

import mx_norm_ref as NR
import qsparse_amd as qs
from qsparse_amd import (MXGLULinear, MXLayerNorm, MXLinear, MXRMSNorm, MXTrainNormLinear, mx_linear, mx_matmul, mx_norm_linear,
                         mx_norm_quantize, mx_quantize_2way)
from qsparse_amd.mx_norm import _mx_norm_y
from mx_norm_ref import DTS, EPS, FMTS, NORMS, WB, same

ROWS, COLS = (1, 31, 33, 129), (1, 31, 32, 33, 96, 1000, 1024)


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


# ---- test 1: the CPU path against the definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_cpu_path_is_the_definition(norm, dtype):
    """every R x C x (weight, bias); the row format walks through all five, the col format two behind it, so each (format, mode,
    dtype) is met some twenty times"""
    i = 0
    for R in ROWS:
        for C in COLS:
            for has_w, has_b in WB:
                x, w, b = NR.inputs(1000 * R + C, R, C, dtype, has_w, has_b)
                fmt, col_fmt = FMTS[i % 5], FMTS[(i + 2) % 5]
                i += 1
                y, rstd, mean = NR.ref_y(x, w, b, norm)
                want = NR.ref_quant(y, fmt, col_fmt)
                got = mx_norm_quantize(x, w, b, norm=norm, eps=EPS, fmt=fmt, col_fmt=col_fmt, return_stats=True)
                assert len(got) == 6
                for name, a, r in zip(("codes", "scales", "col_codes", "col_scales", "rstd"), got, want + (rstd,)):
                    assert same(a, r), (name, R, C, has_w, has_b, fmt, col_fmt)
                assert (got[5] is None) == (norm == "rms") and (mean is None or same(got[5], mean))
                assert len(mx_norm_quantize(x, w, b, norm=norm, eps=EPS, fmt=fmt)) == 2


def test_leading_dimensions_and_return_forms():
    x, w, b = NR.inputs(3, 6 * 33, 96, torch.bfloat16)
    flat = mx_norm_quantize(x, w, b, norm="layer", fmt="mxfp6_e2m3", col_fmt="mxfp8_e5m2", return_stats=True)
    lead = mx_norm_quantize(x.view(6, 33, 96), w, b, norm="layer", fmt="mxfp6_e2m3", col_fmt="mxfp8_e5m2", return_stats=True)
    assert lead[0].shape == (6, 33, 96) and lead[1].shape == (6, 33, 3) and lead[2].shape == (96, 198) and lead[3].shape == (96, 7)
    assert lead[4].shape == lead[5].shape == (6, 33)
    for a, r in zip(lead, flat):
        assert same(a.reshape(r.shape), r)
    # the order of the sums does not depend on the rows around a row
    one = mx_norm_quantize(x[77:78], w, b, norm="layer", fmt="mxfp6_e2m3")
    assert same(one[0], flat[0][77:78]) and same(one[1], flat[1][77:78])


# ---- test 2: the float32 y of the CPU path against float64 -------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
def test_float32_y_against_float64(norm):
    """|y - y64| <= 2^-20 ((|x_i| + |mean|) rstd |w_i| + |b_i|): sixteen float32 roundings' worth.  The worst ratio to the
    bound over these inputs is printed (0.23 in rms mode, 0.30 in layer mode)"""
    worst = 0.0
    for seed, (R, C) in enumerate(((129, 1000), (33, 1024), (257, 96), (31, 33), (64, 4104))):
        x, w, b = NR.inputs(seed, R, C, torch.float32)
        y = _mx_norm_y(x, w, b, norm, EPS)[0]
        assert same(y, NR.ref_y(x, w, b, norm)[0])
        y64, rstd, mean = NR.y_float64(x, w, b, norm)
        bound = 2.0 ** -20 * ((x.double().abs() + mean.abs()) * rstd * w.double().abs() + b.double().abs())
        err = (y.double() - y64).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (R, C, float((err / bound).max()))
    print(f"{norm}: worst |y - y64| / bound = {worst:.3f}")


# ---- test 5: inference layers --------------------------------------------------------------------------------------------------------
def check_inference_layers(dev):
    torch.manual_seed(5)
    K, N = 96, 64
    x = torch.randn(2, 33, K).to(dev)
    lin = nn.Linear(K, N).to(dev)
    wc, ws, _, _ = mx_quantize_2way(lin.weight.detach(), "mxfp8_e4m3", None)
    floats = [nn.RMSNorm(K, eps=1e-5), nn.RMSNorm(K), nn.RMSNorm(K, elementwise_affine=False), nn.LayerNorm(K),
              nn.LayerNorm(K, bias=False), nn.LayerNorm(K, elementwise_affine=False)]
    for f in floats:
        f = f.to(dev)
        for p in f.parameters():
            nn.init.normal_(p, 1.0, 0.25)
        rms = isinstance(f, nn.RMSNorm)
        m = (MXRMSNorm if rms else MXLayerNorm).from_float(f, "mxfp6_e3m2")
        assert list(m.state_dict().keys()) == list(f.state_dict().keys())
        eps = f.eps if f.eps is not None else float(torch.finfo(torch.float32).eps)
        codes, scales = mx_norm_quantize(x, f.weight, getattr(f, "bias", None), norm="rms" if rms else "layer", eps=eps, fmt="mxfp6_e3m2")
        act = m(x)
        assert isinstance(act, qs.MXActivation) and act.fmt == "mxfp6_e3m2" and same(act.codes, codes) and same(act.scales, scales)
        head = MXLinear(wc, ws, "mxfp8_e4m3", lin.bias.detach())
        assert same(nn.Sequential(m, head)(x), mx_matmul(codes, scales, "mxfp6_e3m2", wc, ws, "mxfp8_e4m3", lin.bias.detach()))
        glu = MXGLULinear.from_float(torch.randn(N, K).to(dev) / 8, torch.randn(N, K).to(dev) / 8)
        assert same(nn.Sequential(m, glu)(x), qs.mx_glu_matmul(codes, scales, "mxfp6_e3m2", glu.weight_codes, glu.weight_scales,
                                                                 glu.weight_fmt, glu.bias, act="silu"))
        # the state_dict goes back into a fresh float module
        fresh = copy.deepcopy(f)
        for p in fresh.parameters():
            nn.init.zeros_(p)
        fresh.load_state_dict(m.state_dict())
        for a, r in zip(fresh.parameters(), f.parameters()):
            assert torch.equal(a, r)


def test_inference_layers_cpu():
    check_inference_layers("cpu")


def test_refusals():
    x = torch.randn(4, 32)
    with pytest.raises(ValueError, match="last dimension only"):
        MXLayerNorm.from_float(nn.LayerNorm((4, 32)))
    with pytest.raises(ValueError, match="last dimension only"):
        MXRMSNorm((4, 32))
    with pytest.raises(ValueError, match="unknown norm"):
        mx_norm_quantize(x, norm="batch")
    with pytest.raises(ValueError, match="unknown norm"):
        mx_norm_linear(x, None, None, torch.randn(8, 32), norm="group")
    with pytest.raises(ValueError, match="x is on cpu but weight on meta"):
        mx_norm_quantize(x, torch.ones(32, device="meta"))
    with pytest.raises(TypeError, match="x must be one of"):
        mx_norm_quantize(torch.ones(4, 32, dtype=torch.int32))
    with pytest.raises(TypeError, match="x must be one of"):
        MXRMSNorm(32, eps=1e-6)(torch.ones(4, 32, dtype=torch.int64))
    with pytest.raises(ValueError, match="unknown MX format"):
        mx_norm_quantize(x, fmt="fp8")
    with pytest.raises(ValueError, match="expected \\(32,\\)"):
        mx_norm_quantize(x, torch.ones(31))
    with pytest.raises(TypeError, match="needs an nn.RMSNorm"):
        MXRMSNorm.from_float(nn.LayerNorm(32))
    with pytest.raises(RuntimeError, match="inference layer"):
        MXRMSNorm(32)(x.clone().requires_grad_(True))


# ---- test 6: mx_norm_linear forward and backward ---------------------------------------------------------------------------------
def _train_case(dev, shape, N, norm, seed):
    g = torch.Generator().manual_seed(seed)
    K = shape[-1]
    x = (torch.randn(*shape, generator=g) * 3 + 0.5).to(dev)
    nw = (torch.rand(K, generator=g) + 0.5).to(dev)
    nb = torch.randn(K, generator=g).to(dev) if norm == "layer" else None
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    dy = torch.randn(*shape[:-1], N, generator=g).to(dev)
    return x, nw, nb, W, b, dy


def check_norm_linear(dev, shape, N, norm):
    """forward, dW and db against mx_linear on the definition's y; dx, d norm_weight and d norm_bias against the docstring's formulas
    in float32 (bit for bit) and in float64 (within the margins of DESIGN.md 3r, derived from the count of roundings)"""
    x, nw, nb, W, b, dy = _train_case(dev, shape, N, norm, 6)
    K = shape[-1]
    leaves = [t.clone().requires_grad_(True) for t in (x, nw, W, b)] + [None if nb is None else nb.clone().requires_grad_(True)]
    xg, nwg, Wg, bg, nbg = leaves
    out = mx_norm_linear(xg, nwg, nbg, Wg, bg, norm=norm, eps=EPS)
    out.backward(dy)

    # the definition is evaluated on the CPU, as everywhere in these tests
    y, rstd, mean = [t if t is None else t.to(dev) for t in NR.ref_y(x.reshape(-1, K).cpu(), nw.cpu(), None if nb is None else nb.cpu(), norm)]
    yr = y.reshape(shape).requires_grad_(True)
    Wr, br = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = mx_linear(yr, Wr, br)
    ref.backward(dy)
    assert same(out, ref) and same(Wg.grad, Wr.grad) and same(bg.grad, br.grad)

    dxhat = yr.grad.reshape(-1, K)                                        # mx_linear's input gradient, float32
    dx, dw, db = NR.norm_backward_ref(dxhat, x.reshape(-1, K), rstd, mean, nw, norm)
    assert same(xg.grad, dx.reshape(shape)) and same(nwg.grad, dw) and (nb is None or same(nbg.grad, db))
    dx64, dw64, db64 = NR.norm_backward_ref(dxhat, x.reshape(-1, K), rstd, mean, nw, norm, torch.float64)
    m_dx, m_dw, m_db = NR.norm_backward_margins(dxhat, x.reshape(-1, K), rstd, mean, nw, norm)
    for name, got, want, margin in (("dx", dx, dx64, m_dx), ("dw", dw, dw64, m_dw), ("db", db, db64, m_db)):
        err = (got.double() - want).abs()
        print(f"{norm} {shape}: {name} worst error / margin = {float((err / margin.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= margin).all()), name


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape,N", [((2, 33, 96), 64), ((129, 128), 32)])
def test_norm_linear_cpu(shape, N, norm):
    check_norm_linear("cpu", shape, N, norm)


def check_unasked_gradients(dev, monkeypatch):
    """gradients nobody asks for are not computed; without grad the col pair is not produced"""
    import qsparse_amd.mx_norm as M
    x, nw, nb, W, b, dy = _train_case(dev, (40, 64), 32, "layer", 7)
    calls = []
    real = M.mx_norm_quantize
    monkeypatch.setattr(M, "mx_norm_quantize", lambda *a, **k: calls.append(k.get("col_fmt")) or real(*a, **k))
    with torch.no_grad():
        mx_norm_linear(x, nw, nb, W.requires_grad_(True), b, norm="layer")
    mx_norm_linear(x, nw, nb, W.detach(), b, norm="layer")
    mx_norm_linear(x, nw, nb, W.detach().requires_grad_(True), b, norm="layer")
    assert calls == [None, None, "mxfp8_e4m3"]
    # only x asks: no weight gradient product, no parameter gradients
    products = []
    real_mm = M.mx_matmul
    monkeypatch.setattr(M, "mx_matmul", lambda *a, **k: products.append(a[0].shape) or real_mm(*a, **k))
    xg = x.clone().requires_grad_(True)
    mx_norm_linear(xg, nw, nb, W.detach(), b, norm="layer").backward(dy)
    assert products == [(40, 64), (40, 32)] and xg.grad is not None
    del products[:]
    Wg = W.detach().clone().requires_grad_(True)
    mx_norm_linear(x, nw, nb, Wg, b, norm="layer").backward(dy)
    assert products == [(40, 64), (32, 40)] and Wg.grad is not None


def test_unasked_gradients_cpu(monkeypatch):
    check_unasked_gradients("cpu", monkeypatch)


def check_layer(dev):
    """MXTrainNormLinear shares the float modules' parameters; to_inference() is its forward bit for bit; a stochastic backward differs
    between steps and repeats with the same step"""
    torch.manual_seed(8)
    for fnorm in (nn.RMSNorm(96, eps=1e-5), nn.LayerNorm(96), nn.LayerNorm(96, bias=False), nn.RMSNorm(96, elementwise_affine=False)):
        fnorm, lin = fnorm.to(dev), nn.Linear(96, 64).to(dev)
        layer = MXTrainNormLinear.from_float(fnorm, lin, x_fmt="mxfp6_e2m3")
        assert layer.weight is lin.weight and layer.bias is lin.bias and layer.norm_weight is fnorm.weight
        x = torch.randn(2, 33, 96).to(dev)
        y = layer(x)
        inf = layer.to_inference()
        assert isinstance(inf[0], MXRMSNorm if isinstance(fnorm, nn.RMSNorm) else MXLayerNorm) and isinstance(inf[1], MXLinear)
        assert same(inf(x), y.detach())
    fnorm, lin = nn.RMSNorm(96, eps=1e-5).to(dev), nn.Linear(96, 64).to(dev)
    layer = MXTrainNormLinear.from_float(fnorm, lin, grad_fmt="mxfp4_e2m1", grad_rounding="stochastic", seed=3)
    assert layer.sr_step.device == lin.weight.device
    x, dy = torch.randn(66, 96).to(dev), torch.randn(66, 64).to(dev)

    def grads(step):
        layer.sr_step.fill_(step)
        xg = x.clone().requires_grad_(True)
        for p in layer.parameters():
            p.grad = None
        layer(xg).backward(dy)
        return xg.grad, lin.weight.grad.clone(), fnorm.weight.grad.clone()

    a, b, c = grads(0), grads(1), grads(0)
    assert int(layer.sr_step) == 1
    assert all(same(p, q) for p, q in zip(a, c)) and not same(a[0], b[0]) and not same(a[1], b[1])


def test_layer_cpu():
    check_layer("cpu")
