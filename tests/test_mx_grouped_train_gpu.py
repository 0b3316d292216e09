"""``mx_grouped_weight_grad`` / ``mx_grouped_linear`` / ``MXTrainMoEFeedForward`` on the GPU.  The weight gradient is held to its
normative definition -- ``mx_matmul`` on the masked, 128-aligned slices of the two operands, group by group, under ``G.same`` (bit for
bit, the sign of zero included, all NaNs alike) -- on quantizer codes and on raw bytes, for hostile ``offs``, poisoned blocks and an
output carved out of guard bytes; to the float64 reference within ``mx_gemm_ref.model_bound`` and bit for bit on exact operands, as
tests/test_mx_bmm_train_gpu.py; then the autograd function against the table of public calls, a captured step replayed on other
boundaries, and the mixture-of-experts block.

Shapes (tests/test_mx_grouped_train.py): T = 300, N = 136, K = 72 with offs = [0, 37, 45, 45, 128, 290] -- T no multiple of 32, N and K
past one tile and no multiples of 16 (the PLAIN route), an empty first group, one inside a block, an empty middle one, one ending on a
step of 128, one spanning steps, a 10-token tail -- and T = 256, N = K = 128 for the VEC route."""
import pytest
import torch

import mx_gemm_ref as G
from mx_guard import PAD, PATTERN, guarded, intact
from qsparse_amd import (MXMoEFeedForward, MXTrainMoEFeedForward, _hip, mx_grouped_linear, mx_grouped_weight_grad, mx_quantize_2way)
from test_mx_bmm_train import EXACT_VALUES
from test_mx_grouped import moe_weights
from test_mx_grouped_train import (K_PLAIN, K_VEC, N_PLAIN, N_VEC, OFFS_PLAIN, OFFS_VEC, T_PLAIN, T_VEC, bounds_of, col_pairs, dbias_within,
                                   definition, masked, table)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E4, E5, FP4 = "mxfp8_e4m3", "mxfp8_e5m2", "mxfp4_e2m1"
PAIRS = [(fg, fx) for fg in G.FMTS for fx in G.FMTS]
DIAGONAL = [(G.FMTS[i], G.FMTS[(i + 1) % 5]) for i in range(5)]
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
VEC, PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN


def raw_pairs(g, T, N, K):
    """code bytes uniform over 0 .. 255 -- NaN and Inf encodings and the bits above the format's width included -- and scale bytes
    uniform over 100 .. 150 with 0 and 254 planted inside groups and in a straddling block"""
    ntb = -(-T // 32)
    gt, xt = (torch.randint(0, 256, (r, T), generator=g).to(torch.uint8) for r in (N, K))
    gs, xs = (torch.randint(100, 151, (r, ntb), generator=g).to(torch.uint8) for r in (N, K))
    gs[0, 0], gs[1, 1], gs[2, ntb - 1], xs[0, 1], xs[3, 4], xs[K - 1, ntb - 1] = 0, 254, 0, 254, 0, 254
    return tuple(t.to(DEV) for t in (gt, gs, xt, xs))


def check_definition(ops, fg, fx, row, T, dt, route, offs_dtype=torch.int32):
    dw = mx_grouped_weight_grad(*ops[:2], fg, *ops[2:], fx, torch.tensor(row, dtype=offs_dtype, device=DEV), dt)
    assert _hip.mx_grouped_wgrad_last_route == route
    want = definition(*ops[:2], fg, *ops[2:], fx, row, dt)
    assert dw.shape == want.shape and dw.dtype == dt
    for e in range(len(row)):
        assert G.same(dw[e], want[e]), (fg, fx, row, e, dt)
    return dw


@pytest.mark.parametrize("fg,fx", PAIRS)
def test_weight_grad_is_mx_matmul_on_the_masked_slices_on_the_vec_route(fg, fx):
    p = PAIRS.index((fg, fx))
    g = torch.Generator().manual_seed(p)
    check_definition(col_pairs(g, T_VEC, N_VEC, K_VEC, fg, fx, DEV), fg, fx, OFFS_VEC, T_VEC, DTYPES[p % 3], VEC)
    check_definition(raw_pairs(g, T_VEC, N_VEC, K_VEC), fg, fx, OFFS_VEC, T_VEC, DTYPES[(p + 1) % 3], VEC)


@pytest.mark.parametrize("fg,fx", DIAGONAL)
def test_weight_grad_is_mx_matmul_on_the_masked_slices_on_the_plain_route(fg, fx):
    g = torch.Generator().manual_seed(100 + G.FMTS.index(fg))
    ops, raw = col_pairs(g, T_PLAIN, N_PLAIN, K_PLAIN, fg, fx, DEV), raw_pairs(g, T_PLAIN, N_PLAIN, K_PLAIN)
    for dt in DTYPES:
        check_definition(ops, fg, fx, OFFS_PLAIN, T_PLAIN, dt, PLAIN)
        check_definition(raw, fg, fx, OFFS_PLAIN, T_PLAIN, dt, PLAIN)
    # an operand base off the 16-byte grid sends an aligned shape down the PLAIN route, with the same bits
    ops = col_pairs(g, T_VEC, N_VEC, K_VEC, fg, fx, DEV)
    off = torch.empty(ops[0].numel() + 1, dtype=torch.uint8, device=DEV)[1:].view_as(ops[0]).copy_(ops[0])
    check_definition((off,) + ops[1:], fg, fx, OFFS_VEC, T_VEC, torch.float32, PLAIN)


HOSTILE = [[100, 37, 290, 45, 128, 300],                     # not monotone: the running maximum
           [-5, -1, 40, -300, 129, 129],                     # negative entries
           [0, 37, 500, 45, 10 ** 6, 290],                   # beyond T: the clamp
           [300], [0], [200], [129],                         # one group: everything, nothing, a tail, one token past a step
           [0, 0, 0], [-7, -7], [300, 300, 300],             # all groups empty / all but the first
           [127, 128, 129, 255, 256, 257, 300]]              # boundaries around the steps
HOSTILE_64 = [[2 ** 31 + 5, 0, 0], [100, 2 ** 32 + 5, 150, 2 ** 40, 300], [-2 ** 31 - 1, 50, -2 ** 63, 2 ** 63 - 1, 0], [2 ** 40], [-2 ** 40]]


def test_hostile_offs_give_the_result_of_the_clamped_boundaries():
    g = torch.Generator().manual_seed(7)
    ops = col_pairs(g, T_PLAIN, N_PLAIN, K_PLAIN, E5, E4, DEV)
    for row in HOSTILE:
        for offs_dtype in (torch.int32, torch.int64):
            check_definition(ops, E5, E4, row, T_PLAIN, torch.float32, PLAIN, offs_dtype)
    for row in HOSTILE_64:
        check_definition(ops, E5, E4, row, T_PLAIN, torch.float32, PLAIN, torch.int64)
    ops = col_pairs(g, T_VEC, N_VEC, K_VEC, FP4, "mxfp6_e2m3", DEV)
    for row in ([200, 100, 256, 7], [0, 0], [2 ** 31 - 1], [-2 ** 31, 256]):
        check_definition(ops, FP4, "mxfp6_e2m3", row, T_VEC, torch.bfloat16, VEC)
    assert mx_grouped_weight_grad(*ops[:2], FP4, *ops[2:], "mxfp6_e2m3", torch.zeros(0, dtype=torch.int32, device=DEV)).shape == (0, N_VEC, K_VEC)


@pytest.mark.parametrize("shape", ["plain", "vec"])
def test_poison_stays_inside_the_blocks_that_hold_it(shape):
    T, N, K, row, route = (T_PLAIN, N_PLAIN, K_PLAIN, OFFS_PLAIN, PLAIN) if shape == "plain" else (T_VEC, N_VEC, K_VEC, OFFS_VEC, VEC)
    g = torch.Generator().manual_seed(8)
    gt, gs, xt, xs = col_pairs(g, T, N, K, E5, E4, DEV)
    clean = check_definition((gt, gs, xt, xs), E5, E4, row, T, torch.float32, route)
    assert not clean.isnan().any()
    # the block [192, 224) lies wholly inside the last group: a 0xFF byte and NaN-coded rows there reach no other group
    gs2, gt2, xt2 = gs.clone(), gt.clone(), xt.clone()
    gs2[:, 6], gt2[:, 192:224], xt2[:, 192:224] = 255, 0x7F, 0x7F
    dw = check_definition((gt2, gs2, xt2, xs), E5, E4, row, T, torch.float32, route)
    assert G.same(dw[:5], clean[:5]) and bool(dw[5].isnan().all())
    # ... in one row only: that row of dw[5] and nothing else
    gs2 = gs.clone()
    gs2[3, 6] = 255
    dw = check_definition((gt, gs2, xt, xs), E5, E4, row, T, torch.float32, route)
    bad = torch.zeros_like(clean, dtype=torch.bool)
    bad[5, 3] = True
    assert torch.equal(dw.isnan(), bad) and G.same(dw[~bad], clean[~bad])
    # the block [32, 64) holds group 2 = [37, 45) and straddles its boundaries with 1 = [0, 37) and 4 = [45, 128): both sides follow
    # the definition -- the shared byte is NaN in all three, the empty groups stay +0, the last group is untouched
    xs2 = xs.clone()
    xs2[:, 1] = 255
    dw = check_definition((gt, gs, xt, xs2), E5, E4, row, T, torch.float32, route)
    assert all(bool(dw[e].isnan().all()) for e in (1, 2, 4)) and G.same(dw[[0, 3, 5]], clean[[0, 3, 5]])


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_margins_survive_and_every_element_is_stored(dt, tail):
    """dw carved out of a pattern-filled allocation (tests/mx_guard.py), the pattern in the body too: an element that no work-group
    stored -- an empty group's +0 included -- still holds it.  `tail`: the body ends at the allocation's last byte"""
    for T, N, K, row, route, fg, fx in ((T_PLAIN, N_PLAIN, K_PLAIN, OFFS_PLAIN, PLAIN, E5, "mxfp6_e2m3"), (T_VEC, N_VEC, K_VEC, OFFS_VEC, VEC, FP4, E4),
                                       (T_PLAIN, 133, 129, [0, 0, 300], PLAIN, E5, E4)):
        ops = col_pairs(torch.Generator().manual_seed(T + K), T, N, K, fg, fx, DEV)
        nbytes = len(row) * N * K * torch.empty(0, dtype=dt).element_size()
        if tail:
            raw = torch.full((PAD + nbytes,), PATTERN, dtype=torch.uint8, device=DEV)
            body, ok = raw[PAD:], lambda: bool((raw[:PAD] == PATTERN).all())
        else:
            raw, body = guarded(nbytes)
            ok = lambda: intact(raw, nbytes)
        dw = _hip.mx_grouped_wgrad(*ops[:2], fg, *ops[2:], fx, torch.tensor(row, dtype=torch.int32, device=DEV), dt, out=body.view(dt))
        torch.cuda.synchronize()
        assert dw.data_ptr() == body.data_ptr() and dw.shape == (len(row), N, K) and _hip.mx_grouped_wgrad_last_route == route
        assert ok(), ("dw margins", T, dt, tail)
        assert G.same(dw, definition(*ops[:2], fg, *ops[2:], fx, row, dt)), (T, dt, tail)


# ---- against the CPU path and the float64 reference -------------------------------------------------------------------------------
def against_reference(dw, cpu_ops, fg, fx, row, exact):
    """dw [E, N, K] against the float64 reference on the definition's masked operands (CPU tensors), group by group"""
    gt, gs, xt, xs = cpu_ops
    for e, (lo, hi) in enumerate(bounds_of(row, gt.shape[1])):
        if hi == lo:
            assert not dw[e].any() and not torch.signbit(dw[e]).any()
            continue
        a, b = masked(gt, gs, lo, hi), masked(xt, xs, lo, hi)
        y_ref, y64, S = G.reference(*a, fg, *b, fx, None, dw.dtype)
        if exact:
            assert G.same(dw[e], y_ref + 0.0), e                     # (the sum of the definition starts at +0)
        else:
            ok, ratio = G.within(dw[e], y64, G.model_bound(*a, fg, *b, fx, y64, S, None, dw.dtype))
            print("dw group", e, "largest |err| / model bound", ratio)
            assert ok, (e, ratio)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_codes_equal_the_cpu_path_and_the_products_hold_the_model_bound(dt):
    g = torch.Generator().manual_seed(11)
    fg, fx = E5, FP4
    dy, x = torch.randn(T_PLAIN, N_PLAIN, generator=g), torch.randn(T_PLAIN, K_PLAIN, generator=g)
    cpu = mx_quantize_2way(dy, None, fg)[2:] + mx_quantize_2way(x, None, fx)[2:]
    gpu = mx_quantize_2way(dy.to(DEV), None, fg)[2:] + mx_quantize_2way(x.to(DEV), None, fx)[2:]
    for got, want in zip(gpu, cpu):
        assert torch.equal(got.cpu(), want)
    offs = torch.tensor(OFFS_PLAIN)
    dw = mx_grouped_weight_grad(*gpu[:2], fg, *gpu[2:], fx, offs.to(DEV), dt)
    against_reference(dw.cpu(), cpu, fg, fx, OFFS_PLAIN, False)
    # the CPU path rounds the float64 sum once: it lies inside the same bound, so the two paths agree within twice that
    cpu_dw = mx_grouped_weight_grad(*cpu[:2], fg, *cpu[2:], fx, offs, dt)
    against_reference(cpu_dw, cpu, fg, fx, OFFS_PLAIN, False)


@pytest.mark.parametrize("fmt", G.FMTS)
def test_exact_operands_are_exact_on_the_gpu(fmt):
    """values from {0, +-0.5, +-1, +-2}: every format holds them exactly, products are multiples of 1/4 up to 4 and sums of at most 300
    of them stay far below 2^24 / 4 -- exact in float32 in any order, so dw IS the float64 dy_e^T x_e"""
    g = torch.Generator().manual_seed(12)
    vals = torch.tensor(EXACT_VALUES)
    for T, N, K, row in ((T_PLAIN, N_PLAIN, K_PLAIN, OFFS_PLAIN), (T_VEC, N_VEC, K_VEC, OFFS_VEC)):
        dy, x = (vals[torch.randint(0, len(vals), (T, n), generator=g)] for n in (N, K))
        ops = mx_quantize_2way(dy.to(DEV), None, fmt)[2:] + mx_quantize_2way(x.to(DEV), None, fmt)[2:]
        dw = mx_grouped_weight_grad(*ops[:2], fmt, *ops[2:], fmt, torch.tensor(row, device=DEV)).cpu()
        for e, (lo, hi) in enumerate(bounds_of(row, T)):
            assert torch.equal(dw[e], (dy[lo:hi].double().t() @ x[lo:hi].double()).float()), (fmt, T, e)
        against_reference(dw, tuple(t.cpu() for t in ops), fmt, fmt, row, True)


# ---- mx_grouped_linear ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fx,fw,fg", [(E4, E4, E5), ("mxfp6_e2m3", FP4, "mxfp6_e3m2")])
def test_grouped_linear_is_the_table_of_public_calls(fx, fw, fg, dtype):
    g = torch.Generator().manual_seed(13)
    for T, N, K, row, offs_dtype in ((T_PLAIN, N_PLAIN, K_PLAIN, OFFS_PLAIN, torch.int32), (T_VEC, N_VEC, K_VEC, [100, 37, 256, 0], torch.int64)):
        E = len(row)
        offs = torch.tensor(row, dtype=offs_dtype, device=DEV)
        x = torch.randn(T, K, generator=g).to(dtype).to(DEV).requires_grad_(True)
        w = torch.randn(E, N, K, generator=g).to(dtype).to(DEV).requires_grad_(True)
        bias = torch.randn(E, N, generator=g).to(DEV).requires_grad_(True)          # float32 parameters next to a bfloat16 x are fine
        dy = torch.randn(T, N, generator=g).to(dtype).to(DEV)
        y = mx_grouped_linear(x, w, offs, bias, x_fmt=fx, w_fmt=fw, grad_fmt=fg)
        dx, dw, db = torch.autograd.grad(y, (x, w, bias), dy)
        want = table(x.detach(), w.detach(), bias.detach(), offs, dy, fx, fw, fg, dtype)
        for name, got, wnt in zip(("y", "dx", "dW"), (y.detach(), dx, dw), want):
            assert got.dtype == dtype and G.same(got, wnt), (name, T, dtype)
        tail = bounds_of(row, T)[-1][1]
        assert not dx[tail:].any() and not torch.signbit(dx[tail:]).any() and not y[tail:].any()
        assert db.dtype == torch.float32 and db.shape == (E, N) and dbias_within(db, dy, row), (T, dtype)


def step_of(x, w, bias, offs, dy, **kw):
    return torch.autograd.grad(mx_grouped_linear(x, w, offs, bias, **kw), (x, w, bias), dy)


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
def test_a_captured_step_replays_on_other_boundaries(rounding):
    g = torch.Generator().manual_seed(14)
    T, N, K, E = T_PLAIN, N_PLAIN, K_PLAIN, len(OFFS_PLAIN)
    x = torch.randn(T, K, generator=g).to(DEV).requires_grad_(True)
    w = torch.randn(E, N, K, generator=g).to(DEV).requires_grad_(True)
    bias = torch.randn(E, N, generator=g).to(DEV).requires_grad_(True)
    dy = (torch.randn(T, N, generator=g) * 0.01).to(DEV)
    offs = torch.tensor(OFFS_PLAIN, dtype=torch.int32, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    kw = dict(grad_fmt=FP4, grad_rounding="stochastic", seed=5, step=step) if rounding == "stochastic" else {}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                         # warm-up outside the capture
        step_of(x, w, bias, offs, dy, **kw)
    torch.cuda.current_stream().wait_stream(s)
    step.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = mx_grouped_linear(x, w, offs, bias, **kw)
        grads = torch.autograd.grad(y, (x, w, bias), dy)
    graph.replay()
    first = [t.clone() for t in grads]
    other = torch.tensor([10, 10, 150, 129, 260, 300], dtype=torch.int32, device=DEV)
    offs.copy_(other)                                  # other boundaries in the SAME tensor
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(first[1], grads[1])
    if rounding == "stochastic":
        assert int(step) == 2
        step.fill_(1)                                  # the second replay ran at step 1
    eager_y = mx_grouped_linear(x, w, other.clone(), bias, **kw)
    eager = torch.autograd.grad(eager_y, (x, w, bias), dy)
    assert G.same(y, eager_y) and all(G.same(a, b) for a, b in zip(grads, eager))
    if rounding == "stochastic":
        assert int(step) == 2
        offs.copy_(torch.tensor(OFFS_PLAIN, dtype=torch.int32, device=DEV))
        graph.replay()                                 # the first boundaries again, at step 2: other words than at step 0
        torch.cuda.synchronize()
        assert int(step) == 3 and not torch.equal(first[0], grads[0])


# ---- the mixture-of-experts block -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden_fmt", [E4, FP4])
def test_train_moe_forward_is_the_inference_blocks_and_its_gradients_repeat(hidden_fmt):
    g = torch.Generator().manual_seed(15)
    T, D, H, E, k = 96, 64, 96, 4, 2
    router, up, down = moe_weights(g, E, D, H)
    to = lambda t: t.to(DEV)
    moe = MXTrainMoEFeedForward.from_float(to(router), to(up[0]), to(up[1]), to(down[0]), to(down[1]), k, hidden_fmt=hidden_fmt)
    ref = MXMoEFeedForward.from_float(router, *up, *down, k, hidden_fmt=hidden_fmt).to(DEV)
    x = torch.randn(T, D, generator=g).to(DEV)
    with torch.no_grad():
        want = ref(x)
    y = moe(x)
    assert y.requires_grad and G.same(y.detach(), want)
    with torch.no_grad():
        assert G.same(moe.to_inference()(x), want)
    dy = torch.randn(T, D, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        xg = x.clone().requires_grad_(True)
        runs.append(torch.autograd.grad(moe(xg), [xg, moe.router, moe.up.weight, moe.up.bias, moe.down.weight, moe.down.bias], dy))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(bool(t.isfinite().all()) and bool(t.any()) for t in runs[0])
