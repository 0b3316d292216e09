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
from qsparse_amd.mx_grouped import _offs_int32
from test_mx_grouped import clamped, codes_of, moe_composition, moe_routing_cases, moe_weights, per_group_linear, routed, routing_of

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


def into_poison(dev, fa, fb, offs, bias=None, dt=torch.float32, **kw):
    """the public call's launch with its output in a pattern-filled body instead of a fresh ``torch.empty`` (which is often the block a
    correct call has just freed): a row that is not stored shows as the pattern.  ``offs`` passes through the wrapper's narrowing"""
    T, N = dev[0].shape[0], dev[2].shape[1]
    fill = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
    o32 = _offs_int32(offs, T)
    if kw:
        return _hip.mx_grouped_matmul_q(dev[0], dev[1], fa, dev[2], dev[3], fb, o32, bias, kw["out_fmt"], kw.get("act"),
                                        out=(fill(T * N).view(T, N), fill(T * (-(-N // 32))).view(T, -1)))
    return _hip.mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, o32, bias, dt, out=fill(T * N * torch.empty(0, dtype=dt).element_size()).view(dt))


I32MIN, I32MAX = -2 ** 31, 2 ** 31 - 1
# offs, its dtype, the boundaries c_e = min(max(offs[e], c_{e-1}), 300) worked out by hand
HOSTILE = [([-7, 100, 99, 1000, 200], torch.int32, [0, 100, 100, 300, 300]),
           ([I32MAX] * 5, torch.int32, [300] * 5),
           ([I32MIN, 0, I32MIN, 300, I32MAX], torch.int32, [0, 0, 0, 300, 300]),
           ([301, 0, 0, 0, 0], torch.int32, [300] * 5),
           ([2 ** 31, 0, 0, 0, 0], torch.int64, [300] * 5),                               # narrowing alone: -2^31, group 0 empty
           ([100, 2 ** 32 + 5, 150, 2 ** 40, 300], torch.int64, [100, 300, 300, 300, 300]),      # ... 5 and 0
           ([-2 ** 31 - 1, 50, -2 ** 63, 2 ** 63 - 1, 0], torch.int64, [0, 50, 50, 300, 300])]   # ... 2^31 - 1: group 0 takes every row


@pytest.fixture(scope="module")
def hostile_case():
    """one set of exact-class operands for every row of HOSTILE: T = 300, E = 5, N = 40, K = 96, and their float64 products with
    every weight, [E, T, N] -- any partition's reference is a selection from it"""
    g = torch.Generator().manual_seed(49)
    fa, fb = "mxfp8_e5m2", "mxfp8_e4m3"
    cpu = grouped_case(g, (60,) * 5, 0, 40, 96, fa, fb)
    bias = torch.randint(-64, 64, (5, 40), generator=g).float()
    full = torch.stack([G.reference(cpu[0], cpu[1], fa, cpu[2][e], cpu[3][e], fb)[1] for e in range(5)])
    return fa, fb, cpu, tuple(t.to(DEV) for t in cpu), bias, full


def selected(full, ends):
    y = torch.zeros(full.shape[1:], dtype=torch.float64)
    for e, (lo, hi) in enumerate(zip([0] + ends, ends)):
        y[lo:hi] = full[e, lo:hi]
    return y


@pytest.mark.parametrize("row,dtype,ends", HOSTILE, ids=[str(i) for i in range(len(HOSTILE))])
def test_hostile_offs_give_the_clamped_boundaries(hostile_case, row, dtype, ends):
    """entries above T, negative ones, INT32_MIN / INT32_MAX and int64 ones beyond int32: inside the contract (any content of offs
    gives the result of the clamped boundaries).  MxgmBlock bounds every boundary to [c, cap] with 0 <= c <= cap = min(T, INT32_MAX)
    before it forms an address (qs_mx_gmm.h: `ce = max(v, c)`, `ce = min(ce, cap)`), and every load of offs is at an index below E"""
    fa, fb, cpu, dev, bias, full = hostile_case
    T = 300
    assert clamped(row, T) == ends
    offs, hand = torch.tensor(row, dtype=dtype, device=DEV), torch.tensor(ends, dtype=torch.int32, device=DEV)
    bdev = bias.to(DEV)
    want64 = rounded(selected(full, ends), ends, bias, torch.float32)
    want = into_poison(dev, fa, fb, hand, bdev)
    assert G.same(want, want64) and positive_zero(want[ends[-1]:])
    for got in (mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, offs, bdev), into_poison(dev, fa, fb, offs, bdev)):
        assert G.same(got, want), ("the clamped boundaries", row)
        assert G.same(got, want64), ("float64 reference", row)
    kw = dict(out_fmt="mxfp6_e2m3", act="relu")
    cwant = into_poison(dev, fa, fb, hand, bdev, **kw)
    assert all(torch.equal(a, b) for a, b in zip(cwant, codes_of(relu(want), kw["out_fmt"])))       # the quantizer of the float result
    pieces = per_group(dev, fa, fb, ends, bdev, **kw)
    for lo, hi, (c, s) in pieces:
        assert torch.equal(cwant[0][lo:hi], c) and torch.equal(cwant[1][lo:hi], s), (lo, hi, row)
    assert not cwant[0][ends[-1]:].any() and not cwant[1][ends[-1]:].any()
    for got in (mx_grouped_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, offs, bdev, **kw), into_poison(dev, fa, fb, offs, bdev, **kw)):
        assert torch.equal(got[0], cwant[0]) and torch.equal(got[1], cwant[1]), ("codes out", row)


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
    # an int64 offs: the clamp and the narrowing are captured with the launch, and contents beyond int32 replay as their clamped
    # boundaries ([0, 129, 129, 400], [400] * 4 and [0, 0, 3, 400] by hand)
    wide = [(-5, 129, -2 ** 40, 2 ** 31), (2 ** 32 + 1, 0, 0, 0), (-2 ** 31 - 1, -2 ** 63, 3, 2 ** 63 - 1)]
    hand = [torch.tensor(v, dtype=torch.int32, device=DEV) for v in ((0, 129, 129, 400), (400, 400, 400, 400), (0, 0, 3, 400))]
    static_offs = torch.tensor((100, 200, 300, 400), dtype=torch.int64, device=DEV)
    graph, static_y = captured(step, static_offs)
    graph.replay()
    torch.cuda.synchronize()
    assert G.same(static_y, step(torch.tensor((100, 200, 300, 400), dtype=torch.int32, device=DEV)))
    for v, h in zip(wide, hand):
        static_offs.copy_(torch.tensor(v, dtype=torch.int64))
        graph.replay()
        torch.cuda.synchronize()
        assert G.same(static_y, step(h)), v


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


# ---- the decode's chunks of eight entries of offs -----------------------------------------------------------------------------------
CHUNK_EDGES = (0, 7, 8, 15, 16)        # the first and the last lane of a chunk, for the first three chunks


def chunk_patterns(E):
    """size patterns [E] whose only non-empty groups sit at the CHUNK_EDGES that E has; one of them holds 130 rows (two tiles), the
    others 3: each edge alone, all of them with the two-tile group at each in turn, each pair of neighbours across a chunk boundary
    (the last lane of one chunk, then the first lane of the next), and everything past the first eight groups (a whole chunk of empty
    groups in front).  For E = 9 and 17 the last chunk holds ONE real entry, index 8 / 16, and seven re-reads of it"""
    at = sorted({e for e in CHUNK_EDGES if e < E} | {E - 1})       # (E - 1: the entry that the lanes past it re-read; new for E = 7 alone)
    sets = [(e,) for e in at] + [tuple(at)[i:] + tuple(at)[:i] for i in range(len(at))]
    sets += [(a, b) for a, b in ((7, 8), (8, 7), (15, 16), (16, 15)) if max(a, b) < E]
    if E > 8:
        sets.append(tuple(e for e in at if e >= 8))
    out = []
    for big, *small in sets:
        sizes = [0] * E
        sizes[big] = 130
        for e in small:
            sizes[e] = 3
        out.append(tuple(sizes))
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("E", [7, 8, 9, 16, 17])
def test_the_decode_at_the_edges_of_its_chunks(E):
    """a per-group bias and a per-group scale base in both operands: a group index that is off by one shows in every row"""
    g = torch.Generator().manual_seed(50 + E)
    fa, fb, N, K, tail = "mxfp8_e4m3", "mxfp4_e2m1", 16, 32, 2
    patterns = chunk_patterns(E)
    assert any(not any(p[:8]) for p in patterns) == (E > 8)         # a whole chunk of empty groups in front
    if E in (9, 17):
        assert any(p[E - 1] and p[E - 2] for p in patterns) and any(p[E - 1] and not any(p[:E - 1]) for p in patterns)
    for sizes in patterns:
        assert all(e in CHUNK_EDGES + (E - 1,) for e, n in enumerate(sizes) if n) and 130 in sizes
        cpu = grouped_case(g, sizes, tail, N, K, fa, fb)
        dev = tuple(t.to(DEV) for t in cpu)
        bias = torch.randint(-64, 64, (E, N), generator=g).float()
        ends = ends_of(sizes)
        y = into_poison(dev, fa, fb, torch.tensor(ends, dtype=torch.int32, device=DEV), bias.to(DEV))
        assert _hip.mx_grouped_last_route == VEC and y.shape == (ends[-1] + tail, N)
        for lo, hi, want in per_group(dev, fa, fb, ends, bias.to(DEV)):
            assert G.same(y[lo:hi], want), ("group identity", lo, hi, sizes)
        assert G.same(y, rounded(reference64(cpu, fa, fb, ends), ends, bias, torch.float32)), ("float64 reference", sizes)
        assert positive_zero(y[ends[-1]:]), ("tail", sizes)


def test_the_largest_number_of_groups():
    """E = QS_MX_GROUPED_MAX_GROUPS = 4096, T = 4096 + 3: one row a group, groups 1000 .. 1009 empty, 11 rows in the last one, a tail
    of 3.  The one-row groups against ONE mx_bmm over [G, 1, K] (the per-row mx_matmul by its own definition), the last group against
    mx_matmul, everything against float64"""
    g = torch.Generator().manual_seed(51)
    E, N, K, fa, fb, tail = 4096, 16, 32, "mxfp8_e4m3", "mxfp4_e2m1", 3
    sizes = torch.ones(E, dtype=torch.int64)
    sizes[1000:1010], sizes[E - 1] = 0, 11
    ends = sizes.cumsum(0)
    T = int(ends[-1]) + tail
    assert T == 4096 + 3
    ra, rb = G.scale_windows(K, fa, fb)
    G.assert_exact_class(K, fa, fb, ra, rb)
    owner = torch.cat([torch.repeat_interleave(torch.arange(E), sizes), torch.full((tail,), E)])             # [T]: the group; E: the tail
    suba, subb = G.exact_subset(fa), G.exact_subset(fb)
    ac = suba[torch.randint(0, len(suba), (T, K), generator=g)].to(torch.uint8)
    bc = subb[torch.randint(0, len(subb), (E, N, K), generator=g)].to(torch.uint8)
    asc = (torch.where(owner < E, 120 + 3 * (owner % 9), 127).view(T, 1) + torch.randint(0, ra, (T, 1), generator=g)).to(torch.uint8)
    bsc = ((134 - 3 * (torch.arange(E) % 9)).view(E, 1, 1) + torch.randint(0, rb, (E, N, 1), generator=g)).to(torch.uint8)
    bias = torch.randint(-64, 64, (E, N), generator=g).float()
    dev = tuple(t.to(DEV) for t in (ac, asc, bc, bsc))
    bdev = bias.to(DEV)
    y = into_poison(dev, fa, fb, ends.to(DEV), bdev)
    assert _hip.mx_grouped_last_route == VEC and y.shape == (T, N)
    rows = (owner < E - 1).nonzero().reshape(-1).to(DEV)           # the rows of the one-row groups, and their groups
    of = owner.to(DEV)[rows]
    one = mx_bmm(dev[0][rows, None], dev[1][rows, None], fa, dev[2][of], dev[3][of], fb, bdev[of]).reshape(-1, N)
    assert len(rows) == E - 11 and G.same(y[rows], one)
    lo, hi = int(ends[-2]), int(ends[-1])
    assert hi - lo == 11 and G.same(y[lo:hi], mx_matmul(dev[0][lo:hi], dev[1][lo:hi], fa, dev[2][E - 1], dev[3][E - 1], fb, bdev[E - 1]))
    grouped = owner[:hi]
    want = torch.einsum("tk,tnk->tn", G.values(ac[:hi], asc[:hi], fa), G.values(bc, bsc, fb)[grouped]) + bias[grouped].double()
    assert G.same(y[:hi], (want + 0.0).float()) and positive_zero(y[hi:])


# ---- raw codes: every byte value in both operands, NaN and Inf encodings and the bits above the format's width included -----------
RAW_SIZES, RAW_TAIL = (3, 0, 130, 1), 2
RAW_SHAPES = [(33, 100), (40, 96), (129, 32)]          # (N, K), one per pair


def raw_operand(g, rows, K):
    """code bytes uniform over 0 .. 255 and scale bytes uniform over 100 .. 150, of any leading shape `rows`"""
    return (torch.randint(0, 256, rows + (K,), generator=g).to(torch.uint8),
            torch.randint(100, 151, rows + (-(-K // 32),), generator=g).to(torch.uint8))


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_group_identity_on_raw_codes_and_ff_scale_bytes(fa, fb):
    """the bit-for-bit claim is about ARBITRARY codes: what mx_matmul gives for bytes that the quantizer never writes is left open
    per row, but the grouped product gives the same.  Compared under G.same, which takes all NaNs alike and everything else -- Inf and
    the sign of zero too -- bit for bit.  A raw code may be a NaN by itself, so the 0xFF scale bytes are asserted as a difference: the
    NaNs after planting them are the NaNs before plus exactly the planted row and the planted column of group 2, and no other output
    changes"""
    p = G.FMTS.index(fa) * 5 + G.FMTS.index(fb)
    g = torch.Generator().manual_seed(800 + p)
    N, K = RAW_SHAPES[p % len(RAW_SHAPES)]
    ends, E = ends_of(RAW_SIZES), len(RAW_SIZES)
    T, nkb = ends[-1] + RAW_TAIL, -(-K // 32)
    (ac, asc), (bc, bsc) = raw_operand(g, (T,), K), raw_operand(g, (E, N), K)
    asc[1, 0], asc[70, nkb - 1], asc[T - 1, 0], bsc[0, 2, 0], bsc[2, 5, nkb - 1], bsc[3, N - 1, 0] = 0, 0, 0, 0, 0, 0
    asc[2, nkb - 1], bsc[3, 0, 0] = 255, 255                       # 0xFF in group 0's last row and in the weight of the one-row group
    offs = torch.tensor(ends, dtype=torch.int32, device=DEV)
    route = VEC if K % 16 == 0 else PLAIN
    outs = []
    row, col = 3 + 64, N - 2                                        # a row of group 2 (rows 3 .. 132); a column of its weight
    for planted in (False, True):
        if planted:
            asc[row, 0], bsc[2, col, nkb - 1] = 255, 255
        dev = tuple(t.to(DEV) for t in (ac, asc, bc, bsc))
        for dt in (torch.float32,) + ((torch.bfloat16,) if p % 2 else ()):
            y = into_poison(dev, fa, fb, offs, None, dt)
            assert _hip.mx_grouped_last_route == route
            for lo, hi, want in per_group(dev, fa, fb, ends, None, dt):
                assert G.same(y[lo:hi], want), ("group identity", lo, hi, fa, fb, N, K, dt, planted)
            assert positive_zero(y[ends[-1]:]), ("tail", fa, fb, dt, planted)
            if dt == torch.float32:
                outs.append(y.cpu())
    before, after = outs
    added = torch.zeros(T, N, dtype=torch.bool)
    added[row, :] = True
    added[ends[1]:ends[2], col] = True
    assert bool(after[added].isnan().all())
    assert torch.equal(after.isnan(), before.isnan() | added)
    assert bool(before[2].isnan().all()) and bool(before[ends[2]:ends[3], 0].isnan().all())      # the 0xFF bytes of the first draw
    keep = ~added
    assert G.same(after[keep], before[keep])


@pytest.mark.parametrize("name,logits,dead,k,counts", moe_routing_cases(), ids=[c[0] for c in moe_routing_cases()])
def test_moe_routing_edges_are_the_composition(name, logits, dead, k, counts):
    """routing outcomes that a random router at T = 37 does not produce: an expert that gets no token (an empty group between
    others), top_k == E (the same expert gets every token), T = 1, and one expert with 190 rows (a group of two tiles).  Against the
    per-expert loop of MXLinear pairs, which does not use the grouped kernel; the routing itself is asserted, with its gap"""
    g = torch.Generator().manual_seed(13)
    E, D, H = logits.shape[1], 64, 96
    _, up, down = moe_weights(g, E, D, H)
    router, x = routed(g, logits, D, dead)
    router, x = router.to(DEV), x.to(DEV)
    routing_of(x, router, k, counts)
    moe = MXMoEFeedForward.from_float(router, *up, *down, k).to(DEV)
    to_dev = lambda pair: tuple(t.to(DEV) for t in pair)
    y = moe(x)
    assert y.is_cuda and y.shape == x.shape and not y.isnan().any()
    assert G.same(y, moe_composition(x, router, to_dev(up), to_dev(down), k)), name
    xa = MXActivation(*codes_of(x, "mxfp6_e2m3"), "mxfp6_e2m3")
    routing_of(xa.dequantize(), router, k, counts)
    assert G.same(moe(xa), moe_composition(xa, router, to_dev(up), to_dev(down), k)), name
