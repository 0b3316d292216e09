"""Training through grouped MX products on the CPU path: ``mx_grouped_weight_grad`` against its definition built by hand from
``mx_matmul`` calls on masked slices, ``mx_grouped_linear`` against the table of public calls and -- where every boundary is a multiple
of 128, so that the blocks along the tokens coincide -- against ``mx_linear`` group by group, the layers ``MXTrainGroupedLinear`` and
``MXTrainMoEFeedForward``, every argument refusal, and the C ABI's descriptor and status order, which need no GPU."""
import pytest
import torch

import qsparse_amd as qs
from qsparse_amd import (MXGroupedLinear, MXMoEFeedForward, MXTrainGroupedLinear, MXTrainMoEFeedForward, mx_grouped_linear,
                         mx_grouped_matmul, mx_grouped_weight_grad, mx_linear, mx_matmul, mx_quantize_2way, quantize_with_mx)
from test_mx_grouped import clamped, moe_weights

FMTS = ["mxfp8_e4m3", "mxfp8_e5m2", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp4_e2m1"]
E4, E5, FP4 = "mxfp8_e4m3", "mxfp8_e5m2", "mxfp4_e2m1"
# the smallest shapes where the kernel can go wrong (the GPU tests' too): T no multiple of 32, N and K past one tile and no multiples
# of 16; an empty first group, one inside a block, an empty middle one, one ending on a step, one spanning steps, a 10-token tail
T_PLAIN, N_PLAIN, K_PLAIN, OFFS_PLAIN = 300, 136, 72, [0, 37, 45, 45, 128, 290]
T_VEC, N_VEC, K_VEC, OFFS_VEC = 256, 128, 128, [0, 37, 45, 45, 128, 250]


def codes_of(x, fmt):
    return tuple(quantize_with_mx(x, fmt, -1, return_codes=True)[1:])


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def same(a, b):
    """bit-for-bit equality with all NaNs alike"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a.isnan() & b.isnan()) | ((a == b) & (torch.signbit(a) == torch.signbit(b)))).all())


def bounds_of(offs, T):
    """[(lo, hi)] of the header's clamped boundaries"""
    c = clamped(offs, T)
    return list(zip([0] + c, c))


def masked(codes, scales, lo, hi):
    """the issue's G_e / GS_e (X_e / XS_e) of one operand [rows, T], element by element: the columns [s0, s1), a code outside [lo, hi)
    byte 0, the scale byte of a block that does not intersect [lo, hi) 127"""
    T = codes.shape[1]
    s0, s1 = 128 * (lo // 128), min(T, 128 * -(-hi // 128))
    t = torch.arange(s0, s1, device=codes.device)
    c = torch.where((t >= lo) & (t < hi), codes[:, s0:s1], torch.zeros((), dtype=torch.uint8, device=codes.device))
    b = torch.arange(s0 // 32, -(-s1 // 32), device=codes.device)
    s = torch.where((32 * b < hi) & (32 * b + 32 > lo), scales[:, s0 // 32:-(-s1 // 32)], torch.full((), 127, dtype=torch.uint8, device=codes.device))
    return c, s


def definition(gt, gs, fg, xt, xs, fx, offs, dt=torch.float32):
    """dw [E, N, K] of the normative definition: mx_matmul on the masked slices, +0 for an empty group.  `offs`: Python integers"""
    N, T = gt.shape
    out = torch.zeros(len(offs), N, xt.shape[0], dtype=dt, device=gt.device)
    for e, (lo, hi) in enumerate(bounds_of(offs, T)):
        if hi > lo:
            out[e] = mx_matmul(*masked(gt, gs, lo, hi), fg, *masked(xt, xs, lo, hi), fx, None, dt)
    return out


def col_pairs(g, T, N, K, fg, fx, device="cpu"):
    """(gt_codes [N, T], gt_scales, xt_codes [K, T], xt_scales) of normal deviates under a per-token spread"""
    spread = torch.exp(torch.randn(T, 1, generator=g))
    dy, x = torch.randn(T, N, generator=g) * spread, torch.randn(T, K, generator=g) * spread
    return mx_quantize_2way(dy.to(device), None, fg)[2:] + mx_quantize_2way(x.to(device), None, fx)[2:]


def table(x, w, bias, offs, dy, fx, fw, fg, out_dtype):
    """y, dx, dW of mx_grouped_linear's table from public calls: quantize_with_mx for every Q"""
    T = lambda t: t.transpose(-1, -2).contiguous()
    b32 = None if bias is None else bias.float()
    y = mx_grouped_matmul(*codes_of(x, fx), fx, *codes_of(w, fw), fw, offs, b32, out_dtype)
    dx = mx_grouped_matmul(*codes_of(dy, fg), fg, *codes_of(T(w), fw), fw, offs, None, x.dtype)
    dw = mx_grouped_weight_grad(*codes_of(T(dy), fg), fg, *codes_of(T(x), fx), fx, offs, w.dtype)
    return y, dx, dw


def dbias_within(dbias, dy, offs):
    """dbias[e] against the float64 sum of dy over the rows of group e: within n_e 2^-24 sum |dy|, the worst case of any float32
    summation order (dbias float32)"""
    dy64 = dy.detach().cpu().double()
    for e, (lo, hi) in enumerate(bounds_of(offs, dy.shape[0])):
        err = (dbias[e].detach().cpu().double() - dy64[lo:hi].sum(0)).abs()
        if not bool((err <= (hi - lo) * 2.0 ** -24 * dy64[lo:hi].abs().sum(0)).all()):
            return False
    return True


# ---- mx_grouped_weight_grad -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fg,fx", [(E5, E4), (FP4, "mxfp6_e2m3"), ("mxfp6_e3m2", FP4)])
def test_cpu_weight_grad_is_the_definition_built_by_hand(fg, fx):
    g = torch.Generator().manual_seed(FMTS.index(fg) * 5 + FMTS.index(fx))
    for T, N, K, rows in ((T_PLAIN, 9, 7, [OFFS_PLAIN, [300], [0, 0, 0], [129, 129, 257]]), (64, 3, 40, [[5, 64], [0, 31, 32, 33]])):
        ops = col_pairs(g, T, N, K, fg, fx)
        for row in rows:
            for offs in (torch.tensor(row, dtype=torch.int64), torch.tensor(row, dtype=torch.int32)):
                for dt in (torch.float32, torch.bfloat16, torch.float16):
                    dw = mx_grouped_weight_grad(*ops[:2], fg, *ops[2:], fx, offs, dt)
                    assert dw.shape == (len(row), N, K) and dw.dtype == dt
                    assert bits(dw, definition(*ops[:2], fg, *ops[2:], fx, row, dt)), (T, row, dt)
                    for e, (lo, hi) in enumerate(bounds_of(row, T)):
                        if hi == lo:
                            assert (dw[e] == 0).all() and not torch.signbit(dw[e]).any()          # +0


def test_cpu_weight_grad_poison_stays_inside_the_blocks_that_hold_it():
    g = torch.Generator().manual_seed(2)
    gt, gs, xt, xs = col_pairs(g, T_PLAIN, 9, 7, E5, E4)
    clean = mx_grouped_weight_grad(gt, gs, E5, xt, xs, E4, torch.tensor(OFFS_PLAIN))
    assert not clean.isnan().any()
    # the block [192, 224) lies wholly inside group 5 = [128, 290): 0xFF there, and NaN codes, reach no other group
    gs2, gt2 = gs.clone(), gt.clone()
    gs2[:, 6], gt2[:, 192:224] = 255, 0x7F
    dw = mx_grouped_weight_grad(gt2, gs2, E5, xt, xs, E4, torch.tensor(OFFS_PLAIN))
    assert bits(dw[:5], clean[:5]) and dw[5].isnan().all()
    # the block [32, 64) holds all of group 2 = [37, 45) and straddles its boundaries with 1 = [0, 37) and 4 = [45, 128): the shared
    # byte is NaN in all three, by the definition; the empty groups stay +0 and group 5 is untouched
    xs2 = xs.clone()
    xs2[:, 1] = 255
    dw = mx_grouped_weight_grad(gt, gs, E5, xt, xs2, E4, torch.tensor(OFFS_PLAIN))
    assert all(dw[e].isnan().all() for e in (1, 2, 4)) and bits(dw[[0, 3, 5]], clean[[0, 3, 5]])
    assert same(dw, definition(gt, gs, E5, xt, xs2, E4, OFFS_PLAIN))


def test_weight_grad_refusals():
    g = torch.Generator().manual_seed(4)
    gt, gs, xt, xs = col_pairs(g, 64, 5, 6, E5, E4)
    offs = torch.tensor([10, 10, 64])
    ok = lambda **kw: mx_grouped_weight_grad(kw.pop("gt", gt), kw.pop("gs", gs), kw.pop("fg", E5), kw.pop("xt", xt), kw.pop("xs", xs),
                                             kw.pop("fx", E4), kw.pop("offs", offs), **kw)
    assert ok().shape == (3, 5, 6)
    with pytest.raises(ValueError, match=r"gt_codes needs 2 dimensions \[N, T\]"):
        ok(gt=gt[None], gs=gs[None])
    with pytest.raises(ValueError, match=r"xt_codes needs 2 dimensions \[K, T\]"):
        ok(xt=xt[0], xs=xs[0])
    with pytest.raises(ValueError, match="gt_scales has shape"):
        ok(gs=gs[:, :1])
    with pytest.raises(TypeError, match="xt_codes must be uint8"):
        ok(xt=xt.float())
    with pytest.raises(ValueError, match="disagree on T"):
        ok(xt=xt[:, :32], xs=xs[:, :1])
    with pytest.raises(ValueError, match="unknown MX format|mxfp9"):
        ok(fg="mxfp9")
    with pytest.raises(TypeError, match="offs must be a tensor"):
        ok(offs=[10, 10, 64])
    with pytest.raises(TypeError, match="offs must be an int32 or int64 tensor"):
        ok(offs=offs.float())
    with pytest.raises(ValueError, match=r"offs has shape \(1, 3\)"):
        ok(offs=offs[None])
    with pytest.raises(ValueError, match="gt_codes is on cpu but offs on meta"):
        ok(offs=offs.to("meta"))
    with pytest.raises(ValueError, match="gt_codes is on cpu but xt_codes on meta"):
        ok(xt=xt.to("meta"), xs=xs.to("meta"))
    for bad in ([11, 10, 64], [10, 10, 65], [-1, 10, 64]):
        with pytest.raises(ValueError, match=r"offs must be nondecreasing within \[0, 64\]"):
            ok(offs=torch.tensor(bad))
    with pytest.raises(TypeError, match="out_dtype must be one of"):
        ok(out_dtype=torch.float64)
    assert ok(offs=offs[:0]).shape == (0, 5, 6)
    assert qs.mx_grouped_weight_grad is mx_grouped_weight_grad and qs.mx_grouped_linear is mx_grouped_linear
    assert qs.MXTrainGroupedLinear is MXTrainGroupedLinear and qs.MXTrainMoEFeedForward is MXTrainMoEFeedForward


# ---- mx_grouped_linear ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx,fw,fg", [(E4, E4, E5), ("mxfp6_e2m3", FP4, "mxfp6_e3m2")])
def test_grouped_linear_is_the_table_of_public_calls(fx, fw, fg):
    g = torch.Generator().manual_seed(3)
    for T, N, K, row, dt, out_dtype, with_bias in ((T_PLAIN, 9, 40, OFFS_PLAIN, torch.float32, None, True),
                                                   (70, 36, 19, [0, 33, 64], torch.bfloat16, torch.float32, False),
                                                   (50, 4, 33, [50], torch.float16, None, True)):
        E = len(row)
        offs = torch.tensor(row)
        x = torch.randn(T, K, generator=g).to(dt).requires_grad_(True)
        w = torch.randn(E, N, K, generator=g).to(dt).requires_grad_(True)
        bias = torch.randn(E, N, generator=g).to(dt).requires_grad_(True) if with_bias else None
        y = mx_grouped_linear(x, w, offs, bias, x_fmt=fx, w_fmt=fw, grad_fmt=fg, out_dtype=out_dtype)
        dy = torch.randn(T, N, generator=g).to(y.dtype)
        grads = torch.autograd.grad(y, (x, w) + ((bias,) if with_bias else ()), dy)
        want = table(x.detach(), w.detach(), None if bias is None else bias.detach(), offs, dy, fx, fw, fg, out_dtype or dt)
        for name, got, wnt in zip(("y", "dx", "dW"), (y.detach(), grads[0], grads[1]), want):
            assert bits(got, wnt), (name, T, dt)
        assert y.dtype == (out_dtype or dt) and grads[0].dtype == dt and grads[1].dtype == dt
        tail = row[-1]
        assert (grads[0][tail:] == 0).all() and not torch.signbit(grads[0][tail:]).any()          # the tail rows of dx: +0
        if with_bias:
            assert grads[2].dtype == dt and grads[2].shape == (E, N)
            if dt is torch.float32:
                assert dbias_within(grads[2], dy, row)
            # the tail rows of dy reach nothing
            dy2 = dy.clone()
            dy2[tail:] = 1e4
            again = torch.autograd.grad(mx_grouped_linear(x, w, offs, bias, x_fmt=fx, w_fmt=fw, grad_fmt=fg, out_dtype=out_dtype),
                                        (x, w, bias), dy2)
            assert bits(again[0], grads[0]) and bits(again[2], grads[2])
            live = [e for e, (lo, hi) in enumerate(bounds_of(row, T)) if hi <= 32 * (tail // 32)]        # groups that share no block with the tail
            assert bits(again[1][live], grads[1][live])


def test_gradients_nobody_asks_for_are_not_computed_and_nothing_is_kept_without_grad():
    g = torch.Generator().manual_seed(5)
    x, w, offs = torch.randn(40, 32, generator=g), torch.randn(2, 8, 32, generator=g), torch.tensor([10, 40])
    y = mx_grouped_linear(x, w, offs)
    assert not y.requires_grad and bits(y, table(x, w, None, offs, y, E4, E4, E5, torch.float32)[0])
    xg = x.clone().requires_grad_(True)
    y = mx_grouped_linear(xg, w, offs)
    assert [t is None for t in y.grad_fn.saved_tensors[:4]] == [True, True, False, False]          # only the col pair of W
    wg = w.clone().requires_grad_(True)
    y = mx_grouped_linear(x, wg, offs)
    assert [t is None for t in y.grad_fn.saved_tensors[:4]] == [False, False, True, True]          # only the col pair of x
    assert all(t is None or t.dtype in (torch.uint8, torch.int64) for t in y.grad_fn.saved_tensors)      # codes and offs, no float tensor
    with torch.no_grad():
        assert not mx_grouped_linear(xg, wg, offs).requires_grad


def test_grouped_linear_refusals():
    x, w, offs = torch.randn(6, 32), torch.randn(3, 5, 32), torch.tensor([2, 2, 6])
    assert mx_grouped_linear(x, w, offs).shape == (6, 5)
    with pytest.raises(ValueError, match=r"x needs \[T, K\] and weight \[E, N, K\].*is mx_linear"):
        mx_grouped_linear(x, w[0], offs)
    with pytest.raises(ValueError, match="disagree on K"):
        mx_grouped_linear(x[:, :16], w, offs)
    with pytest.raises(ValueError, match=r"bias has shape \(5,\), expected \(3, 5\)"):
        mx_grouped_linear(x, w, offs, torch.zeros(5))
    with pytest.raises(ValueError, match=r"offs has shape \(2,\), expected \(3,\)"):
        mx_grouped_linear(x, w, offs[:2])
    with pytest.raises(TypeError, match="offs must be an int32 or int64 tensor"):
        mx_grouped_linear(x, w, offs.float())
    with pytest.raises(ValueError, match="x is on cpu but offs on meta"):
        mx_grouped_linear(x, w, offs.to("meta"))
    with pytest.raises(ValueError, match="x is on cpu but weight on meta"):
        mx_grouped_linear(x, w.to("meta"), offs)
    with pytest.raises(TypeError, match="x must be one of"):
        mx_grouped_linear(x.double(), w, offs)
    with pytest.raises(ValueError, match="unknown MX format|mxfp9"):
        mx_grouped_linear(x, w, offs, grad_fmt="mxfp9")
    with pytest.raises(ValueError, match="unknown rounding"):
        mx_grouped_linear(x, w, offs, grad_rounding="up")
    with pytest.raises(TypeError, match="step must be a one-element int64 tensor"):
        mx_grouped_linear(x, w, offs, grad_rounding="stochastic", step=torch.zeros(1))
    with pytest.raises(ValueError, match=r"offs must be nondecreasing within \[0, 6\]"):
        mx_grouped_linear(x, w, torch.tensor([3, 2, 6]))


def test_every_group_is_mx_linear_when_the_boundaries_are_multiples_of_128():
    """the blocks along the tokens then coincide with those of the group's own rows, so y, dx and dW of group e are mx_linear's on
    x[lo:hi] with the weight and bias of e, bit for bit (wgrad_split_k=1: the unsplit product)"""
    g = torch.Generator().manual_seed(6)
    row, T, N, K = [128, 128, 384], 394, 24, 40
    x = torch.randn(T, K, generator=g).requires_grad_(True)
    w = torch.randn(3, N, K, generator=g).requires_grad_(True)
    bias = torch.randn(3, N, generator=g).requires_grad_(True)
    dy = torch.randn(T, N, generator=g)
    fmts = dict(x_fmt="mxfp6_e2m3", w_fmt=FP4, grad_fmt=E5)
    y = mx_grouped_linear(x, w, torch.tensor(row), bias, **fmts)
    dx, dw, db = torch.autograd.grad(y, (x, w, bias), dy)
    for e, (lo, hi) in enumerate(bounds_of(row, T)):
        if hi == lo:
            assert not dw[e].any() and not db[e].any()
            continue
        xe, we, be = x[lo:hi].detach().requires_grad_(True), w[e].detach().requires_grad_(True), bias[e].detach().requires_grad_(True)
        ye = mx_linear(xe, we, be, **fmts, wgrad_split_k=1)
        dxe, dwe, dbe = torch.autograd.grad(ye, (xe, we, be), dy[lo:hi])
        assert bits(y[lo:hi].detach(), ye.detach()) and bits(dx[lo:hi], dxe) and bits(dw[e], dwe), e
        assert torch.allclose(db[e], dbe, rtol=0, atol=float((hi - lo) * 2.0 ** -23 * dy[lo:hi].abs().sum(0).max()))
    assert not y[384:].any() and not dx[384:].any()


def test_stochastic_rounding_touches_dy_alone_and_advances_the_step():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(70, 32, generator=g).requires_grad_(True)
    w = torch.randn(2, 8, 32, generator=g).requires_grad_(True)
    offs, dy = torch.tensor([33, 64]), torch.randn(70, 8, generator=g) * 0.01
    step = torch.tensor([3])
    kw = dict(grad_fmt=FP4, grad_rounding="stochastic", seed=11, step=step)
    y = mx_grouped_linear(x, w, offs, **kw)
    assert bits(y.detach(), mx_grouped_linear(x, w, offs, grad_fmt=FP4).detach()) and int(step) == 3
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    assert int(step) == 4
    g_row, g_rs, g_col, g_cs = mx_quantize_2way(dy, FP4, FP4, "stochastic", 11, torch.tensor([3]))
    wt = w.detach().transpose(1, 2).contiguous()
    assert bits(dx, mx_grouped_matmul(g_row, g_rs, FP4, *codes_of(wt, E4), E4, offs))
    assert bits(dw, mx_grouped_weight_grad(g_col, g_cs, FP4, *codes_of(x.detach().t().contiguous(), E4), E4, offs))
    dx2, _ = torch.autograd.grad(mx_grouped_linear(x, w, offs, **kw), (x, w), dy)
    assert int(step) == 5 and not torch.equal(dx, dx2)


# ---- the layers -----------------------------------------------------------------------------------------------------------------------
def test_train_grouped_linear_layer_and_its_round_trip_to_inference():
    g = torch.Generator().manual_seed(8)
    w, b = torch.randn(3, 10, 40, generator=g), torch.randn(3, 10, generator=g)
    layer = MXTrainGroupedLinear.from_float(w, b, x_fmt="mxfp6_e2m3", w_fmt=FP4)
    assert layer.weight.data_ptr() == w.data_ptr() and layer.bias.data_ptr() == b.data_ptr()           # shared, not copied
    assert isinstance(layer.weight, torch.nn.Parameter) and set(layer.state_dict()) == {"weight", "bias"}
    assert (layer.num_groups, layer.out_features, layer.in_features) == (3, 10, 40) and "num_groups=3" in repr(layer)
    p = torch.nn.Parameter(w.clone())
    assert MXTrainGroupedLinear.from_float(p).weight is p and set(MXTrainGroupedLinear.from_float(p).state_dict()) == {"weight"}
    x, offs = torch.randn(9, 40, generator=g), torch.tensor([4, 4, 7])
    y = layer(x, offs)
    assert y.requires_grad and bits(y.detach(), mx_grouped_linear(x, w, offs, b, x_fmt="mxfp6_e2m3", w_fmt=FP4))
    inf = layer.to_inference()
    assert isinstance(inf, MXGroupedLinear) and inf.weight_fmt == FP4 and inf.act_fmt == "mxfp6_e2m3"
    assert torch.equal(inf.weight_codes, codes_of(w, FP4)[0]) and torch.equal(inf.weight_scales, codes_of(w, FP4)[1])
    assert bits(inf(x, offs), y.detach())
    again = MXTrainGroupedLinear.from_float(w, b, x_fmt="mxfp6_e2m3", w_fmt=FP4).to_inference()
    assert torch.equal(again.weight_codes, inf.weight_codes) and torch.equal(again.bias, inf.bias)
    fresh = MXTrainGroupedLinear(3, 40, 10, grad_rounding="stochastic", seed=5)
    assert fresh.weight.shape == (3, 10, 40) and fresh.bias.shape == (3, 10) and float(fresh.weight.detach().abs().max()) <= 40 ** -0.5
    assert fresh.sr_seed == 5 and int(fresh.sr_step) == 0 and "sr_step" not in fresh.state_dict()
    fresh(x, offs).sum().backward()
    assert int(fresh.sr_step) == 1 and fresh.weight.grad.shape == (3, 10, 40) and fresh.bias.grad.shape == (3, 10)
    with pytest.raises(ValueError, match=r"needs a weight tensor \[E, N, K\]"):
        MXTrainGroupedLinear.from_float(w[0])
    with pytest.raises(ValueError, match=r"expected \(3, 10\)"):
        MXTrainGroupedLinear.from_float(w, b[0])


def test_train_moe_forward_is_the_inference_blocks_and_its_gradients_repeat():
    g = torch.Generator().manual_seed(9)
    E, k, D, H, T = 4, 2, 64, 96, 37
    router, up, down = moe_weights(g, E, D, H)
    for hidden_fmt in (E4, FP4):
        moe = MXTrainMoEFeedForward.from_float(router, *up, *down, k, hidden_fmt=hidden_fmt)
        ref = MXMoEFeedForward.from_float(router, *up, *down, k, hidden_fmt=hidden_fmt)
        assert isinstance(moe.router, torch.nn.Parameter) and moe.up.weight.data_ptr() == up[0].data_ptr()
        assert set(moe.state_dict()) == {"router", "up.weight", "up.bias", "down.weight", "down.bias"}
        x = torch.randn(T, D, generator=g)
        with torch.no_grad():
            want = ref(x)
        y = moe(x)
        assert y.requires_grad and bits(y.detach(), want)
        inf = moe.to_inference()
        assert isinstance(inf, MXMoEFeedForward) and inf.up.out_fmt == hidden_fmt and inf.up.act == "relu"
        with torch.no_grad():
            assert bits(inf(x), want)
        assert torch.equal(inf.up.weight_codes, ref.up.weight_codes) and torch.equal(inf.down.weight_scales, ref.down.weight_scales)
        runs = []
        for _ in range(2):
            xg = x.clone().requires_grad_(True)
            params = [moe.router, moe.up.weight, moe.up.bias, moe.down.weight, moe.down.bias]
            runs.append(torch.autograd.grad(moe(xg), [xg] + params, torch.ones(T, D)))
        assert all(bits(a, b) for a, b in zip(*runs)) and all(bool(t.isfinite().all()) and bool(t.any()) for t in runs[0])
    with pytest.raises(TypeError, match="must be MXTrainGroupedLinear"):
        MXTrainMoEFeedForward(router, moe.up, torch.nn.Linear(4, 4), 1)
    with pytest.raises(ValueError, match=r"top_k must be an int in \[1, 4\]"):
        MXTrainMoEFeedForward(router, moe.up, moe.down, 5)
    with pytest.raises(ValueError, match=r"needs up \[E, H, D\] and down \[E, D, H\]"):
        MXTrainMoEFeedForward(router[:3], moe.up, moe.down, 1)
    with pytest.raises(ValueError, match=r"x must be \[T, D\]"):
        moe(x[:, :32])


# ---- the C ABI without a GPU: layout of the descriptor, and the checks that come before anything is enqueued ---------------------
def test_descriptor_has_the_headers_layout(tmp_path):
    import ctypes
    import os
    import subprocess
    from qsparse_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cname, ct = "qs_mx_grouped_wgrad_args", _hip.MxGroupedWgradArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(root, "include", "qsparse_hip.h")}"', 'int main(void) {',
             f'printf("%zu", sizeof({cname}));'] + [f'printf(" %zu", offsetof({cname}, {fname}));' for fname, _ in ct._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ['return 0; }']))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    size, *offsets = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(ct) and [int(o) for o in offsets] == [getattr(ct, f).offset for f, _ in ct._fields_]
    assert "qs_mx_grouped_wgrad_v" in _hip.SIGNATURES and "qs_mx_grouped_wgrad_route" in _hip.SIGNATURES


def test_entry_points_validate_without_a_gpu():
    import ctypes
    from qsparse_amd import _hip
    lib = _hip.load()
    ARG, DTYPE, ALIGN = -2, -1, -3
    VEC, PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN
    assert lib.qs_mx_grouped_wgrad_v(None) == ARG and lib.qs_mx_grouped_wgrad_route(None) == ARG

    def desc(**kw):
        a = _hip.MxGroupedWgradArgs()
        a.struct_size = ctypes.sizeof(a)
        a.gt_codes, a.gt_scales, a.xt_codes, a.xt_scales, a.offs, a.dw = 1024, 2048, 4096, 8192, 512, 1 << 30
        a.T, a.E, a.N, a.K = 64, 3, 8, 15
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    route = lib.qs_mx_grouped_wgrad_route
    for fn in (route, lib.qs_mx_grouped_wgrad_v):                 # the refusals of the launching call: nothing is enqueued
        for name in ("gt_codes", "gt_scales", "xt_codes", "xt_scales", "offs", "dw"):
            assert fn(desc(**{name: None})) == ARG, name
        assert fn(desc(g_format=5)) == ARG and fn(desc(x_format=-1)) == ARG
        for name in ("T", "E", "N", "K"):
            assert fn(desc(**{name: -1})) == ARG, name
        assert fn(desc(E=4097)) == ARG
        assert fn(desc(ydt=7)) == DTYPE and fn(desc(ydt=7, E=-1)) == ARG          # the arguments come before the dtype
        assert fn(desc(dw=(1 << 30) + 2)) == ALIGN and fn(desc(offs=514)) == ALIGN
        assert fn(desc(ydt=7, dw=(1 << 30) + 2)) == DTYPE                           # ... the dtype before the alignment
        for empty in ("E", "N", "K"):
            assert fn(desc(**{empty: 0})) == 0
        assert fn(desc(N=1 << 40, T=1 << 24)) == ARG and fn(desc(K=1 << 40, T=1 << 24)) == ARG       # N T, K T beyond INT64_MAX
        assert fn(desc(E=4096, N=1 << 26, K=1 << 26)) == ARG                        # E N K beyond INT64_MAX
        assert fn(desc(E=4096, N=1 << 20, K=1 << 20, T=1)) == ARG                   # more work-groups than a grid holds
    assert route(desc()) == VEC and route(desc(E=4096)) == VEC
    assert route(desc(T=40)) == PLAIN                                               # T % 16 != 0
    assert route(desc(gt_codes=1025)) == PLAIN and route(desc(xt_codes=4097)) == PLAIN       # a base off the 16-byte grid
    assert route(desc(ydt=_hip._DT[torch.bfloat16], dw=(1 << 30) + 2)) == VEC
    assert route(desc(T=0, gt_codes=None, gt_scales=None, xt_codes=None, xt_scales=None)) == VEC       # no token: every group is empty
    assert route(desc(E=2047, N=128 << 10, K=128 << 10, T=16)) == VEC and route(desc(E=2048, N=128 << 10, K=128 << 10, T=16)) == ARG       # 2^31 - 2^20, 2^31
