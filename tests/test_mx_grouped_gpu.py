"""Grouped (ragged) matrix products on MX codes on the GPU (qs_mx_grouped_matmul_v, qs_mx_grouped_matmul_q_v).  The main property is
the group identity: the rows of group e of ``mx_grouped_matmul`` are bit for bit ``mx_matmul`` of those rows with the weight of e, for
all 25 format pairs, with the route of every launch asserted, and the rows past the last group are +0.  The operands are from the
exact class of tests/mx_gemm_ref.py with a different scale base per group in both operands, so a kernel that reads the wrong expert's
weight, or strides the scales by the code stride, cannot pass; the same operands are checked against the float64 reference too,
which guards against a bug shared with ``mx_matmul``.  The group boundaries stay on the device: a captured call replays with other
boundaries written into the same tensor."""
import pytest
import torch

import mx_gemm_ref as G
import qsparse_amd as qs
from qsparse_amd import MXActivation, MXGroupedLinear, MXMoEFeedForward, _hip, mx_bmm, mx_grouped_matmul, mx_matmul, quantize_with_mx
from test_mx_grouped import codes_of, moe_composition, moe_weights, per_group_linear

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
VEC, PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN
# empty groups first, last and consecutive; a group of one row; groups one under, at and one over a tile; a group spanning three tiles
SIZES, TAIL = (0, 1, 127, 0, 0, 129, 128, 257, 0), 5
SHAPES = [(16, 129), (129, 32), (300, 256), (132, 1)]          # (N, K)
PER_PAIR = 4          # shapes per pair; see shapes_of


def shapes_of(fa, fb):
    """PER_PAIR of the 4 shapes for the pair, walking the list by the pair's index: every pair meets every shape, and the draw's index
    i, which picks the dtype of offs and the output dtypes, differs from pair to pair"""
    p = G.FMTS.index(fa) * 5 + G.FMTS.index(fb)
    return [(i, SHAPES[i % len(SHAPES)]) for i in range(PER_PAIR * p, PER_PAIR * p + PER_PAIR)]


def test_every_shape_meets_every_width():
    for width in ("fp8", "fp6", "fp4"):
        seen = {s for fa, fb in PAIRS if width in fa or width in fb for _, s in shapes_of(fa, fb)}
        assert seen == set(SHAPES), width


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def ends_of(sizes):
    return torch.tensor(sizes, dtype=torch.int64).cumsum(0).tolist()


def grouped_case(g, sizes, tail, N, K, fa, fb):
    """exact-class operands on the CPU: the rows of group e under the scale base 120 + 3 (e % 9), weight e under 134 - 3 (e % 9), the
    tail rows under 127 -- neighbouring groups differ in both operands' scales, and the products stay near 2^0, where acc + bias is
    exact in float32 as well.  (a_codes [T, K], a_scales, b_codes [E, N, K], b_scales)"""
    ra, rb = G.scale_windows(K, fa, fb)
    G.assert_exact_class(K, fa, fb, ra, rb)
    a = [G.exact_operand(g, n, K, fa, ra, 120 + 3 * (e % 9)) for e, n in enumerate(sizes)] + [G.exact_operand(g, tail, K, fa, ra, 127)]
    b = [G.exact_operand(g, N, K, fb, rb, 134 - 3 * (e % 9)) for e in range(len(sizes))]
    nkb = -(-K // 32)
    stack = lambda ts, shape: torch.stack(ts) if ts else torch.zeros(shape, dtype=torch.uint8)
    return (torch.cat([c for c, _ in a]), torch.cat([s for _, s in a]), stack([c for c, _ in b], (0, N, K)), stack([s for _, s in b], (0, N, nkb)))


def group_bias(bias, e):
    return None if bias is None else (bias if bias.dim() == 1 else bias[e])


def per_group(ops, fa, fb, ends, bias=None, dt=torch.float32, **kw):
    """mx_matmul over the groups that have rows: [(lo, hi, result)]"""
    out = []
    for e, (lo, hi) in enumerate(zip([0] + ends, ends)):
        if hi > lo:
            out.append((lo, hi, mx_matmul(ops[0][lo:hi], ops[1][lo:hi], fa, ops[2][e], ops[3][e], fb, group_bias(bias, e), dt, **kw)))
    return out


def reference64(cpu, fa, fb, ends):
    """the float64 definition without a bias, [T, N]: the groups' products, zeros in the tail"""
    T, N = cpu[0].shape[0], cpu[2].shape[1]
    y = torch.zeros(T, N, dtype=torch.float64)
    for e, (lo, hi) in enumerate(zip([0] + ends, ends)):
        if hi > lo:
            y[lo:hi] = G.reference(cpu[0][lo:hi], cpu[1][lo:hi], fa, cpu[2][e], cpu[3][e], fb)[1]
    return y


def rounded(y64, ends, bias, dt):
    """the reference with the groups' bias, rounded once to `dt`.  The sum of the definition starts at +0 (a -0 product sums to +0),
    which a float64 matmul over K = 1 does not do by itself: hence the `+ 0.0`.  The tail takes no bias"""
    y = y64.clone()
    for e, (lo, hi) in enumerate(zip([0] + ends, ends)):
        if bias is not None:
            y[lo:hi] += group_bias(bias, e).double()
    return (y + 0.0).to(dt)


def positive_zero(t):
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_group_identity_float64_reference_and_the_tail(fa, fb):
    g = torch.Generator().manual_seed(700 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    ends, E = ends_of(SIZES), len(SIZES)
    for i, (N, K) in shapes_of(fa, fb):
        cpu = grouped_case(g, SIZES, TAIL, N, K, fa, fb)
        dev = tuple(t.to(DEV) for t in cpu)
        offs = torch.tensor(ends, dtype=torch.int32 if i % 2 else torch.int64, device=DEV)
        y64 = reference64(cpu, fa, fb, ends)
        route = VEC if K % 16 == 0 else PLAIN
        for bias in (None, torch.randint(-64, 64, (N,), generator=g).float(), torch.randint(-64, 64, (E, N), generator=g).float()):
            bdev = None if bias is None else bias.to(DEV)
            for dt in (torch.float32,) + ((torch.bfloat16, torch.float16) if i % 3 == 0 else ()):
                what = (fa, fb, N, K, None if bias is None else tuple(bias.shape), dt)
                y = mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, offs, bdev, dt)
                assert _hip.mx_grouped_last_route == route, (_hip.mx_grouped_last_route, what)
                assert y.is_cuda and y.dtype == dt and y.shape == (ends[-1] + TAIL, N)
                for lo, hi, want in per_group(dev, fa, fb, ends, bdev, dt):
                    assert G.same(y[lo:hi], want), ("group identity", lo, hi, what)
                assert G.same(y, rounded(y64, ends, bias, dt)), ("float64 reference", what)
                assert positive_zero(y[ends[-1]:]), ("tail", what)


def test_no_store_across_a_group_boundary():
    """300 groups of one row: every tile holds 127 rows that belong to later groups, and a kernel that stored them would race 127
    wrong writers against each right one.  One launch of mx_bmm on [300, 1, K] is the per-row mx_matmul by its own definition"""
    g = torch.Generator().manual_seed(41)
    E, N, K, fa, fb = 300, 129, 32, "mxfp8_e4m3", "mxfp6_e2m3"
    cpu = grouped_case(g, (1,) * E, 0, N, K, fa, fb)
    dev = tuple(t.to(DEV) for t in cpu)
    bias = torch.randint(-64, 64, (E, N), generator=g).float()
    offs = torch.arange(1, E + 1, dtype=torch.int32, device=DEV)
    y = mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, offs, bias.to(DEV))
    assert _hip.mx_grouped_last_route == VEC
    assert G.same(y, mx_bmm(dev[0][:, None], dev[1][:, None], fa, dev[2], dev[3], fb, bias.to(DEV)).reshape(E, N))
    want = torch.einsum("ek,enk->en", G.values(cpu[0], cpu[1], fa), G.values(cpu[2], cpu[3], fb)) + bias.double()
    assert G.same(y, (want + 0.0).float())


def offset_by_one(t):
    """the same bytes on the device at a base one byte past a 16-byte boundary (a slice of a larger allocation)"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    return view


def test_degenerate_cases():
    g = torch.Generator().manual_seed(42)
    fa, fb, N, K = "mxfp6_e3m2", "mxfp4_e2m1", 132, 64
    cpu = grouped_case(g, (130, 0, 70), 3, N, K, fa, fb)
    dev = tuple(t.to(DEV) for t in cpu)
    T = 203
    bias = torch.randint(-64, 64, (N,), generator=g).float().to(DEV)
    offs = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    # one group that holds every row: mx_matmul on the whole matrix
    y = mx_grouped_matmul(dev[0], dev[1], fa, dev[2][:1], dev[3][:1], fb, offs(T), bias)
    assert _hip.mx_grouped_last_route == VEC and G.same(y, mx_matmul(dev[0], dev[1], fa, dev[2][0], dev[3][0], fb, bias))
    # every group empty, and no group at all: zeros, no bias
    for y in (mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, offs(0, 0, 0), bias),
              mx_grouped_matmul(dev[0], dev[1], fa, dev[2][:0], dev[3][:0], fb, offs(), bias, torch.bfloat16)):
        assert _hip.mx_grouped_last_route == VEC and y.shape == (T, N) and positive_zero(y)
    codes, scales = mx_grouped_matmul(dev[0], dev[1], fa, dev[2][:0], dev[3][:0], fb, offs(), bias, out_fmt="mxfp8_e4m3", act="relu")
    assert codes.shape == (T, N) and scales.shape == (T, 5) and not codes.any() and not scales.any()
    # no rows: nothing is enqueued
    y = mx_grouped_matmul(dev[0][:0], dev[1][:0], fa, dev[2], dev[3], fb, offs(0, 0, 0))
    assert y.shape == (0, N) and _hip.mx_grouped_last_route is None
    codes, scales = mx_grouped_matmul(dev[0][:0], dev[1][:0], fa, dev[2], dev[3], fb, offs(0, 0, 0), out_fmt="mxfp4_e2m1")
    assert codes.shape == (0, N) and scales.shape == (0, 5) and _hip.mx_grouped_q_last_route is None
    # a code base off by one byte: the byte loads, the same bits
    y = mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, offs(130, 130, 200), bias)
    assert _hip.mx_grouped_last_route == VEC
    for shifted in ((0,), (2,), (0, 1, 2, 3)):
        ops = tuple(offset_by_one(t) if j in shifted else t for j, t in enumerate(dev))
        z = mx_grouped_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, offs(130, 130, 200), bias)
        assert _hip.mx_grouped_last_route == PLAIN and G.same(z, y), shifted
    assert G.same(y, rounded(reference64(cpu, fa, fb, [130, 130, 200]), [130, 130, 200], bias.cpu(), torch.float32))


def test_boundaries_are_clamped_on_the_device():
    """[5, 3, 10] is within range but not monotone: the running maximum makes it [5, 5, 10]"""
    g = torch.Generator().manual_seed(43)
    fa, fb = "mxfp8_e5m2", "mxfp8_e4m3"
    cpu = grouped_case(g, (5, 0, 5), 0, 40, 96, fa, fb)
    dev = tuple(t.to(DEV) for t in cpu)
    bias = torch.randint(-64, 64, (3, 40), generator=g).float().to(DEV)
    got = mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, torch.tensor([5, 3, 10], device=DEV), bias)
    want = mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, torch.tensor([5, 5, 10], device=DEV), bias)
    assert G.same(got, want)
    assert G.same(want, rounded(reference64(cpu, fa, fb, [5, 5, 10]), [5, 5, 10], bias.cpu(), torch.float32))


def relu(y):
    return torch.where(y > 0, y, torch.where(y != y, y, torch.zeros_like(y)))


@pytest.mark.parametrize("fa,fb,out_fmt,N,K", [("mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e4m3", 64, 96), ("mxfp4_e2m1", "mxfp6_e2m3", "mxfp8_e5m2", 100, 96),
                                               ("mxfp8_e5m2", "mxfp4_e2m1", "mxfp6_e2m3", 33, 100), ("mxfp6_e3m2", "mxfp8_e4m3", "mxfp6_e3m2", 132, 64),
                                               ("mxfp6_e2m3", "mxfp4_e2m1", "mxfp4_e2m1", 161, 40)])
def test_codes_out_is_the_quantizer_of_the_float_result(fa, fb, out_fmt, N, K):
    g = torch.Generator().manual_seed(44 + N)
    ends, E = ends_of(SIZES), len(SIZES)
    T = ends[-1] + TAIL
    route = VEC if K % 16 == 0 else PLAIN
    w = torch.randn(E, N, K, generator=g) / K ** 0.5 * torch.pow(2.0, torch.arange(E) % 5.0).view(-1, 1, 1)     # every expert its own scale
    dev = codes_of((torch.randn(T, K, generator=g) * 2).to(DEV), fa) + codes_of(w.to(DEV), fb)
    offs = torch.tensor(ends, dtype=torch.int32, device=DEV)
    biases = (None, torch.randn(N, generator=g).to(DEV), torch.randn(E, N, generator=g).to(DEV))
    for j, act in enumerate((None, "relu", None, "relu")):
        bias = biases[j % 3]
        codes, scales = mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, offs, bias, out_fmt=out_fmt, act=act)
        assert _hip.mx_grouped_q_last_route == route
        assert codes.shape == (T, N) and scales.shape == (T, -(-N // 32)) and codes.dtype == scales.dtype == torch.uint8
        y32 = mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, offs, bias)
        want = codes_of(relu(y32) if act else y32, out_fmt)
        assert torch.equal(codes, want[0]) and torch.equal(scales, want[1]), (out_fmt, act)
        for lo, hi, (c, s) in per_group(dev, fa, fb, ends, bias, out_fmt=out_fmt, act=act):
            assert torch.equal(codes[lo:hi], c) and torch.equal(scales[lo:hi], s), (lo, hi, out_fmt, act)
        assert not codes[ends[-1]:].any() and not scales[ends[-1]:].any()


def captured(step, *warm):
    """`step` captured on one stream after a warm-up on a side stream: (graph, its static result)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*warm)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(*warm)
    return graph, out


def test_graph_capture_replays_with_other_boundaries():
    g = torch.Generator().manual_seed(45)
    fa, fb, N, K, T = "mxfp8_e4m3", "mxfp4_e2m1", 200, 160, 400
    cpu = grouped_case(g, (100, 100, 100, 100), 0, N, K, fa, fb)
    dev = tuple(t.to(DEV) for t in cpu)
    bias = torch.randint(-64, 64, (4, N), generator=g).float().to(DEV)
    step = lambda o: mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, o, bias)
    contents = [torch.tensor(v, dtype=torch.int32, device=DEV) for v in ((0, 129, 129, 390), (400, 400, 400, 400), (1, 2, 3, 4))]
    eager = [step(o).clone() for o in contents]
    assert not G.same(eager[0], eager[1]) and not G.same(eager[0], eager[2])
    static_offs = torch.tensor((100, 200, 300, 400), dtype=torch.int32, device=DEV)
    graph, static_y = captured(step, static_offs)
    for o, want in zip(contents, eager):
        static_offs.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        assert G.same(static_y, want), o.tolist()


def test_graph_capture_of_the_moe_block_replays_bit_for_bit():
    g = torch.Generator().manual_seed(46)
    E, k, D, H, T = 4, 2, 64, 96, 37
    router, up, down = moe_weights(g, E, D, H)
    moe = MXMoEFeedForward.from_float(router, *up, *down, k).to(DEV)
    xs = [torch.randn(T, D, generator=g).to(DEV) for _ in range(3)]
    eager = [moe(x).clone() for x in xs]
    assert not G.same(eager[0], eager[1])
    static_x = xs[2].clone()
    graph, static_y = captured(moe, static_x)
    for x, want in zip(xs, eager):
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert G.same(static_y, want)


def test_grouped_linear_is_the_per_group_loop_of_linear():
    g = torch.Generator().manual_seed(47)
    E, N, K, sizes = 5, 130, 72, (3, 0, 140, 128, 1)
    w, b = torch.randn(E, N, K, generator=g) * torch.pow(2.0, torch.arange(E).float()).view(-1, 1, 1), torch.randn(E, N, generator=g)
    x = torch.randn(sum(sizes) + 4, K, generator=g).to(DEV)
    ends = ends_of(sizes)
    offs = torch.tensor(ends, device=DEV)
    wc, ws = codes_of(w.to(DEV), "mxfp6_e2m3")
    layer = MXGroupedLinear.from_float(w, b, "mxfp6_e2m3", "mxfp8_e5m2").to(DEV)
    y = layer(x, offs)
    assert y.is_cuda and y.shape == (x.shape[0], N) and positive_zero(y[ends[-1]:])
    for (lo, hi), piece in zip(zip([0] + ends, ends), per_group_linear(x, offs, wc, ws, "mxfp6_e2m3", b.to(DEV), "mxfp8_e5m2")):
        assert piece is None and hi == lo or G.same(y[lo:hi], piece), (lo, hi)
    chained = MXGroupedLinear(wc, ws, "mxfp6_e2m3", b, "mxfp8_e5m2", out_fmt="mxfp4_e2m1", act="relu").to(DEV)
    act = chained(x, offs)
    assert isinstance(act, MXActivation) and act.fmt == "mxfp4_e2m1"
    for (lo, hi), piece in zip(zip([0] + ends, ends), per_group_linear(x, offs, wc, ws, "mxfp6_e2m3", b.to(DEV), "mxfp8_e5m2", out_fmt="mxfp4_e2m1",
                                                                      act="relu")):
        assert piece is None and hi == lo or torch.equal(act.codes[lo:hi], piece.codes) and torch.equal(act.scales[lo:hi], piece.scales)
    assert G.same(layer(MXActivation(*codes_of(x, "mxfp8_e5m2"), "mxfp8_e5m2"), offs), y)


def test_moe_feed_forward_is_its_composition():
    g = torch.Generator().manual_seed(48)
    E, k, D, H, T = 4, 2, 64, 96, 37
    router, up, down = moe_weights(g, E, D, H)
    moe = MXMoEFeedForward.from_float(router, *up, *down, k).to(DEV)
    assert set(moe.state_dict()) == {"router", "up.weight_codes", "up.weight_scales", "up.bias", "down.weight_codes", "down.weight_scales",
                                     "down.bias"}
    to_dev = lambda pair: tuple(t.to(DEV) for t in pair)
    x = torch.randn(T, D, generator=g).to(DEV)
    y = moe(x)
    assert y.is_cuda and y.shape == (T, D) and y.dtype == torch.float32 and not y.isnan().any()
    assert G.same(y, moe_composition(x, router.to(DEV), to_dev(up), to_dev(down), k))
    assert G.same(moe(x), y)                                        # no atomic combine: the same bits on every run
    xa = MXActivation(*codes_of(x, "mxfp6_e2m3"), "mxfp6_e2m3")
    assert G.same(moe(xa), moe_composition(xa, router.to(DEV), to_dev(up), to_dev(down), k))
