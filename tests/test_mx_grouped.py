"""Grouped (ragged) matrix products on MX codes on the CPU: ``mx_grouped_matmul`` against ``mx_matmul`` group by group (bit for bit,
codes out included) and its tail rows, every argument refusal with its message, the constructors of ``MXGroupedLinear`` and
``MXMoEFeedForward`` and their compositions, and the C ABI's descriptors and status order, which need no GPU."""
import pytest
import torch

import qsparse_amd as qs
from qsparse_amd import MXActivation, MXGroupedLinear, MXMoEFeedForward, mx_grouped_matmul, mx_matmul, quantize_with_mx
from qsparse_amd.mx_gemm import MXLinear

FMTS = ["mxfp8_e4m3", "mxfp8_e5m2", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp4_e2m1"]
E4, FP4 = "mxfp8_e4m3", "mxfp4_e2m1"


def codes_of(x, fmt):
    return tuple(quantize_with_mx(x, fmt, -1, return_codes=True)[1:])


def operands(g, T, E, N, K, fa, fb):
    """(a_codes [T, K], a_scales, b_codes [E, N, K], b_scales); weight e is scaled by 2^e, so no two experts agree"""
    w = torch.randn(E, N, K, generator=g) * torch.pow(2.0, torch.arange(E, dtype=torch.float32)).view(-1, 1, 1)
    return codes_of(torch.randn(T, K, generator=g) * 3, fa) + codes_of(w, fb)


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def ends_of(sizes):
    return torch.tensor(sizes, dtype=torch.int64).cumsum(0)


def bias_of(bias, e):
    return None if bias is None else (bias if bias.dim() == 1 else bias[e])


@pytest.mark.parametrize("fa,fb", [(E4, E4), (FP4, "mxfp6_e2m3"), ("mxfp8_e5m2", FP4), ("mxfp6_e3m2", E4)])
def test_cpu_path_is_matmul_group_by_group_and_the_tail_is_zero(fa, fb):
    g = torch.Generator().manual_seed(FMTS.index(fa) * 5 + FMTS.index(fb))
    for sizes, tail, N, K in (((0, 1, 5, 0, 0, 3, 0), 2, 7, 40), ((4,), 0, 33, 64), ((2, 2), 3, 1, 1)):
        E, T = len(sizes), sum(sizes) + tail
        ops = operands(g, T, E, N, K, fa, fb)
        args = (*ops[:2], fa, *ops[2:], fb)
        ends = ends_of(sizes).tolist()
        for offs in (ends_of(sizes), ends_of(sizes).to(torch.int32)):
            for bias in (None, torch.randn(N, generator=g), torch.randn(E, N, generator=g)):
                for dt in (torch.float32, torch.bfloat16, torch.float16):
                    y = mx_grouped_matmul(*args, offs, bias, dt)
                    assert y.shape == (T, N) and y.dtype == dt
                    for e, (lo, hi) in enumerate(zip([0] + ends, ends)):
                        assert bits(y[lo:hi], mx_matmul(ops[0][lo:hi], ops[1][lo:hi], fa, ops[2][e], ops[3][e], fb, bias_of(bias, e), dt))
                    assert (y[ends[-1]:] == 0).all() and not torch.signbit(y[ends[-1]:]).any()        # +0, no bias
                for out_fmt in (E4, FP4):
                    for act in (None, "relu"):
                        codes, scales = mx_grouped_matmul(*args, offs, bias, out_fmt=out_fmt, act=act)
                        assert codes.shape == (T, N) and scales.shape == (T, -(-N // 32)) and codes.dtype == scales.dtype == torch.uint8
                        for e, (lo, hi) in enumerate(zip([0] + ends, ends)):
                            if hi > lo:
                                want = mx_matmul(ops[0][lo:hi], ops[1][lo:hi], fa, ops[2][e], ops[3][e], fb, bias_of(bias, e), out_fmt=out_fmt,
                                                 act=act)
                                assert torch.equal(codes[lo:hi], want[0]) and torch.equal(scales[lo:hi], want[1])
                        assert not codes[ends[-1]:].any() and not scales[ends[-1]:].any()


def test_cpu_path_without_groups_or_rows():
    g = torch.Generator().manual_seed(3)
    ops = operands(g, 4, 2, 5, 32, E4, FP4)
    none = (ops[2][:0], ops[3][:0])
    y = mx_grouped_matmul(ops[0], ops[1], E4, *none, FP4, torch.zeros(0, dtype=torch.int32), torch.ones(5))
    assert y.shape == (4, 5) and (y == 0).all() and not torch.signbit(y).any()           # E == 0: every row is a tail row
    codes, scales = mx_grouped_matmul(ops[0], ops[1], E4, *none, FP4, torch.zeros(0, dtype=torch.int32), out_fmt=E4, act="relu")
    assert codes.shape == (4, 5) and scales.shape == (4, 1) and not codes.any() and not scales.any()
    y = mx_grouped_matmul(ops[0][:0], ops[1][:0], E4, ops[2], ops[3], FP4, torch.zeros(2, dtype=torch.int64))
    assert y.shape == (0, 5)
    codes, scales = mx_grouped_matmul(ops[0][:0], ops[1][:0], E4, ops[2], ops[3], FP4, torch.zeros(2, dtype=torch.int64), out_fmt=FP4)
    assert codes.shape == (0, 5) and scales.shape == (0, 1)


def test_argument_refusals():
    g = torch.Generator().manual_seed(4)
    ac, asc, bc, bsc = operands(g, 6, 3, 5, 64, E4, FP4)
    offs = torch.tensor([2, 2, 6])
    ok = lambda **kw: mx_grouped_matmul(kw.pop("ac", ac), kw.pop("asc", asc), kw.pop("fa", E4), kw.pop("bc", bc), kw.pop("bsc", bsc),
                                        kw.pop("fb", FP4), kw.pop("offs", offs), **kw)
    assert ok().shape == (6, 5)
    with pytest.raises(ValueError, match=r"a_codes needs 2 dimensions \[T, K\]"):
        ok(ac=ac[None], asc=asc[None])
    with pytest.raises(ValueError, match=r"b_codes needs 3 dimensions \[E, N, K\]"):
        ok(bc=bc[None], bsc=bsc[None])
    with pytest.raises(ValueError, match="one weight .* shared by every row of a is mx_matmul"):
        ok(bc=bc[0], bsc=bsc[0])
    with pytest.raises(ValueError, match="a_scales has shape"):
        ok(asc=asc[:, :1])
    with pytest.raises(TypeError, match="a_codes must be uint8"):
        ok(ac=ac.float())
    with pytest.raises(ValueError, match="disagree on K"):
        ok(bc=bc[..., :32], bsc=bsc[..., :1])
    with pytest.raises(ValueError, match="unknown MX format|mxfp9"):
        ok(fa="mxfp9")
    with pytest.raises(TypeError, match="offs must be a tensor"):
        ok(offs=[2, 2, 6])
    with pytest.raises(TypeError, match="offs must be an int32 or int64 tensor"):
        ok(offs=offs.float())
    with pytest.raises(ValueError, match=r"offs has shape \(2,\), expected \(3,\)"):
        ok(offs=offs[:2])
    with pytest.raises(ValueError, match=r"offs has shape \(1, 3\)"):
        ok(offs=offs[None])
    with pytest.raises(ValueError, match="a_codes is on cpu but offs on meta"):
        ok(offs=offs.to("meta"))
    with pytest.raises(ValueError, match=r"offs must be nondecreasing within \[0, 6\]"):
        ok(offs=torch.tensor([3, 2, 6]))
    with pytest.raises(ValueError, match=r"offs must be nondecreasing within \[0, 6\]"):
        ok(offs=torch.tensor([2, 2, 7]))
    with pytest.raises(ValueError, match=r"offs must be nondecreasing within \[0, 6\]"):
        ok(offs=torch.tensor([-1, 2, 6]))
    with pytest.raises(ValueError, match="act='relu' needs out_fmt"):
        ok(act="relu")
    with pytest.raises(ValueError, match="cannot be combined with out_fmt"):
        ok(out_dtype=torch.bfloat16, out_fmt=E4)
    with pytest.raises(TypeError, match="out_dtype must be one of"):
        ok(out_dtype=torch.float64)
    with pytest.raises(TypeError, match="bias must be a float32 tensor"):
        ok(bias=torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"bias has shape \(3,\), expected \(5,\) or \(3, 5\)"):
        ok(bias=torch.zeros(3))
    assert qs.mx_grouped_matmul is mx_grouped_matmul and qs.MXGroupedLinear is MXGroupedLinear and qs.MXMoEFeedForward is MXMoEFeedForward


# ---- the boundaries of the definition, the grid's bound on the M-tiles and the wrapper's narrowing of an int64 offs ---------------
TILE = 128
INT32_MIN, INT32_MAX, INT64_MIN, INT64_MAX = -2 ** 31, 2 ** 31 - 1, -2 ** 63, 2 ** 63 - 1
TIGHT = ((1, 129, 1, 257), 1)          # sizes and tail that all leave 1 row modulo 128: the bound on the M-tiles is reached


def clamped(offs, T):
    """the header's boundaries in Python integers: c_-1 = 0, c_e = min(max(offs[e], c_{e-1}), T)"""
    out, c = [], 0
    for v in offs:
        c = min(max(int(v), c), T)
        out.append(c)
    return out


def m_tiles(offs, T):
    """the M-tiles the kernel has work for: group-relative ones of every group, then the tail's"""
    c = clamped(offs, T)
    return sum(-(-(hi - lo) // TILE) for lo, hi in zip([0] + c, c)) + -(-(T - (c[-1] if c else 0)) // TILE)


def mt_max(T, E):
    """the grid's bound (qs_mx_gmm.h, mx_gmm_mt_max)"""
    return (T + (TILE - 1) * (E + 1)) // TILE


def test_the_grid_bound_holds_for_any_offs_and_the_tight_family_reaches_it():
    g = torch.Generator().manual_seed(11)
    cases = []
    for _ in range(300):                                                  # random sizes with a random tail
        E = int(torch.randint(0, 20, (1,), generator=g))
        sizes = torch.randint(0, 300, (E,), generator=g).tolist()
        cases.append((sum(sizes) + int(torch.randint(0, 200, (1,), generator=g)), ends_of(sizes).tolist() if E else []))
    for _ in range(300):                                                  # any content, not sorted and out of range
        E, T = int(torch.randint(1, 20, (1,), generator=g)), int(torch.randint(0, 1000, (1,), generator=g))
        cases.append((T, torch.randint(-200, 1400, (E,), generator=g).tolist()))
    for T in (0, 1, 127, 128, 129, 900):
        for E in (0, 1, 7, 8, 9, 4096):
            cases += [(T, [0] * E), (T, [T] * E), (T, [T] + [0] * (E - 1) if E else []), (T, [0] * (E - 1) + [T] if E else [])]
    for E in range(0, 12):                                                # every group and the tail 1 modulo 128
        for tail in (0, 1, 129):
            sizes = [1 + TILE * int(v) for v in torch.randint(0, 3, (E,), generator=g)]
            cases.append((sum(sizes) + tail, ends_of(sizes).tolist() if E else []))
    cases += [(300, v) for v in ([-7, 100, 99, 1000, 200], [INT32_MAX] * 5, [INT32_MIN, 0, INT32_MIN, 300, INT32_MAX], [301, 0, 0, 0, 0],
                                 [2 ** 31, 0, 0, 0, 0], [100, 2 ** 32 + 5, 150, 2 ** 40, 300], [INT64_MIN, INT64_MAX, 0], [INT64_MAX, INT64_MIN])]
    for T, offs in cases:
        c = clamped(offs, T)
        assert all(0 <= lo <= hi <= T for lo, hi in zip([0] + c, c + [T])), (T, offs)          # a partition of [0, c_{E-1}) and the tail
        assert m_tiles(offs, T) <= mt_max(T, len(offs)), (T, offs)
    for sizes, tail in (TIGHT, (TIGHT[0], 0), ((), 129), ((1,) * 40, 1), ((129,) * 7, 257)):
        T, offs = sum(sizes) + tail, ends_of(sizes).tolist() if sizes else []
        assert m_tiles(offs, T) == mt_max(T, len(offs)), (sizes, tail)     # reached: an empty tail wastes nothing either
    sizes = (0, 1, 127, 0, 0, 129, 128, 257, 0)                           # the GPU tests' main case is far from it
    assert (m_tiles(ends_of(sizes).tolist(), sum(sizes) + 5), mt_max(sum(sizes) + 5, len(sizes))) == (9, 14)


def test_the_int64_offs_is_clamped_before_it_is_narrowed():
    """what the kernel is handed for an int64 ``offs`` gives the boundaries of the int64 definition; a plain ``.to(torch.int32)`` wraps
    (2^31 -> -2^31, 2^32 + 5 -> 5, -2^31 - 1 -> 2^31 - 1, 2^40 -> 0)"""
    from qsparse_amd.mx_grouped import _offs_int32
    rows = [[2 ** 31, 0, 0, 0, 0], [100, 2 ** 32 + 5, 150, 2 ** 40, 300], [-2 ** 31 - 1, 50, INT64_MIN, INT64_MAX, 0], [2 ** 32 + 5], [2 ** 40],
            [-2 ** 31 - 1], [2 ** 31], [INT64_MAX], [INT64_MIN], [INT64_MIN, INT64_MAX], [INT64_MAX, INT64_MIN], [-1, 5, 3, 299, 300, 301],
            [INT32_MAX, INT32_MIN], []]
    for T in (1, 300, INT32_MAX, 2 ** 31, 2 ** 33):
        for row in rows:
            wide = torch.tensor(row, dtype=torch.int64)
            narrow = _offs_int32(wide, T)
            assert narrow.dtype == torch.int32 and narrow.shape == wide.shape and narrow.is_contiguous()
            assert clamped(narrow.tolist(), T) == [min(c, INT32_MAX) for c in clamped(row, T)], (T, row)      # (the kernel's cap)
    for row in ([-7, 100, 99, 1000, 200], [INT32_MAX] * 5, [INT32_MIN, 0, INT32_MIN, 300, INT32_MAX]):
        narrow = torch.tensor(row, dtype=torch.int32)
        assert _offs_int32(narrow, 300).tolist() == row                    # an int32 one is the kernel's to clamp: handed on as it is
    assert _offs_int32(torch.tensor([3, 0, 9, 0])[::2], 5).tolist() == [3, 5]          # (strided in: contiguous out)


def per_group_linear(x, offs, wc, ws, w_fmt, bias, act_fmt, **kw):
    """one MXLinear per group on the group's rows; the pieces, in order"""
    out, lo = [], 0
    for e, hi in enumerate(offs.tolist()):
        lin = MXLinear(wc[e], ws[e], w_fmt, None if bias is None else bias[e], act_fmt, **kw)
        out.append(lin(MXActivation(x.codes[lo:hi], x.scales[lo:hi], x.fmt) if isinstance(x, MXActivation) else x[lo:hi]) if hi > lo else None)
        lo = hi
    return out


def test_grouped_linear_constructors_and_the_per_group_loop():
    g = torch.Generator().manual_seed(5)
    E, N, K, sizes = 3, 10, 40, (4, 0, 3)
    w, b, x = torch.randn(E, N, K, generator=g), torch.randn(E, N, generator=g), torch.randn(9, K, generator=g)
    offs = ends_of(sizes)
    layer = MXGroupedLinear.from_float(w, b, FP4, "mxfp6_e2m3")
    assert (layer.num_groups, layer.out_features, layer.in_features) == (E, N, K) and layer.weight_fmt == FP4
    assert set(layer.state_dict()) == {"weight_codes", "weight_scales", "bias"}
    assert set(MXGroupedLinear.from_float(w).state_dict()) == {"weight_codes", "weight_scales"}
    wc, ws = codes_of(w, FP4)
    assert torch.equal(layer.weight_codes, wc) and torch.equal(layer.weight_scales, ws) and "num_groups=3" in repr(layer)
    y = layer(x, offs)
    assert y.shape == (9, N) and y.dtype == torch.float32 and not y.requires_grad
    pieces = per_group_linear(x, offs, wc, ws, FP4, b, "mxfp6_e2m3")
    assert bits(y[:4], pieces[0]) and pieces[1] is None and bits(y[4:7], pieces[2]) and (y[7:] == 0).all()
    # codes out, and an MXActivation in
    chained = MXGroupedLinear(wc, ws, FP4, b, "mxfp6_e2m3", out_fmt=E4, act="relu")
    act = chained(x, offs)
    assert isinstance(act, MXActivation) and act.fmt == E4 and act.codes.shape == (9, N) and act.scales.shape == (9, 1)
    pieces = per_group_linear(x, offs, wc, ws, FP4, b, "mxfp6_e2m3", out_fmt=E4, act="relu")
    assert torch.equal(act.codes[:4], pieces[0].codes) and torch.equal(act.scales[4:7], pieces[2].scales)
    xa = MXActivation(*codes_of(x, "mxfp6_e2m3"), "mxfp6_e2m3")
    assert bits(layer(xa, offs), y)
    # from_exported
    qt = qs.QuantizedTensor(kind="mx", bits=4, channel_index=-1, codes=wc, values=w, block_scale=ws, fmt=FP4, block_dim=-1)
    assert bits(MXGroupedLinear.from_exported(qt, b, "mxfp6_e2m3")(x, offs), y)
    qt.block_dim = 1
    with pytest.raises(ValueError, match="blocks run along dim 1, not along K"):
        MXGroupedLinear.from_exported(qt)
    qt.kind = "int"
    with pytest.raises(ValueError, match="needs an MX weight"):
        MXGroupedLinear.from_exported(qt)
    with pytest.raises(ValueError, match=r"needs a weight tensor \[E, N, K\]"):
        MXGroupedLinear.from_float(w[0])
    with pytest.raises(ValueError, match=r"bias has shape \(10,\), expected \(3, 10\)"):
        MXGroupedLinear(wc, ws, FP4, b[0])
    with pytest.raises(ValueError, match="act='relu' needs out_fmt"):
        MXGroupedLinear(wc, ws, FP4, act="relu")
    with pytest.raises(RuntimeError, match="inference layer"):
        layer(x.clone().requires_grad_(True), offs)


def moe_composition(x, router, up, down, k, act_fmt=E4, hidden_fmt=E4, w_fmt=E4):
    """the block written out with one MXLinear pair per expert: expert e takes, in token order, the (token, slot) pairs routed to it"""
    x32 = x.dequantize() if isinstance(x, MXActivation) else x
    top, experts = torch.topk(x32 @ router.t(), k, -1)
    gates = torch.softmax(top, -1)
    y = torch.zeros(x32.shape[0], k, router.shape[1], device=x32.device)
    for e in range(router.shape[0]):
        tok, slot = (experts == e).nonzero(as_tuple=True)
        if len(tok):
            first = MXLinear(*codes_of(up[0][e], w_fmt), w_fmt, up[1][e], act_fmt, out_fmt=hidden_fmt, act="relu").to(x32.device)
            second = MXLinear(*codes_of(down[0][e], w_fmt), w_fmt, down[1][e], hidden_fmt).to(x32.device)
            rows = MXActivation(x.codes[tok], x.scales[tok], x.fmt) if isinstance(x, MXActivation) else x[tok]
            y[tok, slot] = second(first(rows))
    return (y * gates.unsqueeze(-1)).sum(1)


def moe_weights(g, E, D, H):
    return (torch.randn(E, D, generator=g), (torch.randn(E, H, D, generator=g) / D ** 0.5, torch.randn(E, H, generator=g)),
            (torch.randn(E, D, H, generator=g) / H ** 0.5, torch.randn(E, D, generator=g)))


def test_moe_feed_forward_is_its_composition_and_its_constructors():
    g = torch.Generator().manual_seed(6)
    E, k, D, H, T = 4, 2, 64, 96, 37
    router, up, down = moe_weights(g, E, D, H)
    moe = MXMoEFeedForward.from_float(router, *up, *down, k)
    assert set(moe.state_dict()) == {"router", "up.weight_codes", "up.weight_scales", "up.bias", "down.weight_codes", "down.weight_scales",
                                     "down.bias"}
    assert moe.up.out_fmt == E4 and moe.up.act == "relu" and moe.down.out_fmt is None and "top_k=2" in repr(moe)
    x = torch.randn(T, D, generator=g)
    y = moe(x)
    assert y.shape == (T, D) and y.dtype == torch.float32 and bits(y, moe_composition(x, router, up, down, k))
    assert bits(moe(x), y)
    xa = MXActivation(*codes_of(x, E4), E4)
    assert bits(moe(xa), moe_composition(xa, router, up, down, k))
    with pytest.raises(ValueError, match=r"top_k must be an int in \[1, 4\]"):
        MXMoEFeedForward(router, moe.up, moe.down, 5)
    with pytest.raises(TypeError, match="must be MXGroupedLinear"):
        MXMoEFeedForward(router, moe.up, torch.nn.Linear(4, 4), 1)
    with pytest.raises(ValueError, match="up must hand out MX codes"):
        MXMoEFeedForward(router, MXGroupedLinear.from_float(up[0]), moe.down, 1)
    with pytest.raises(ValueError, match="down must return float32"):
        MXMoEFeedForward(router, moe.up, MXGroupedLinear.from_float(down[0], None, E4, E4, out_fmt=E4), 1)
    with pytest.raises(ValueError, match=r"needs up \[E, H, D\] and down \[E, D, H\]"):
        MXMoEFeedForward(router[:3], moe.up, moe.down, 1)
    with pytest.raises(ValueError, match=r"x must be \[T, D\]"):
        moe(x[:, :32])


# ---- routing outcomes at the edges: an expert without a token, top_k == E, one token, an expert whose group spans two tiles ------
ROUTING_GAP = 0.5


def routed(g, logits, D, dead=()):
    """(router [E, D], x [T, D]) in float32 with ``x @ router.t() == logits`` up to float32 rounding, the rows `dead` of the router all
    zero (their logits are exactly 0): x is the minimum-norm solution plus noise from the router's null space, so its rows are not of
    rank E"""
    T, E = logits.shape
    live = [e for e in range(E) if e not in dead]
    router = torch.zeros(E, D, dtype=torch.float64)
    router[live] = torch.randn(len(live), D, generator=g, dtype=torch.float64)
    pinv = torch.linalg.pinv(router[live])                                     # [D, live]
    noise = torch.randn(T, D, generator=g, dtype=torch.float64) / 8       # (small: an MX-quantized x keeps the gap as well)
    x = logits[:, live].double() @ pinv.t() + noise - noise @ (pinv @ router[live])
    return router.float(), x.float()


def moe_routing_cases():
    """[(name, logits [T, E], dead router rows, k, {expert: the (token, slot) pairs it must get})].  The logits of a token are distinct
    integers, so the top-k order has a gap of 1 (``routing_of`` asserts more than ROUTING_GAP of it on the device that routes)"""
    g = torch.Generator().manual_seed(12)
    T = 37
    starved = torch.zeros(T, 4)
    starved[:, [0, 1, 3]] = torch.stack([torch.tensor([1.0, 2.0, 3.0])[torch.randperm(3, generator=g)] for _ in range(T)])
    two_tiles = torch.tensor([[2.0, 1.0]] * 190 + [[1.0, 2.0]] * 10)[torch.randperm(200, generator=g)]
    return [("an expert without a token", starved, (2,), 2, {2: 0}),           # its logit 0 is below the other three, 1 2 3
            ("top_k == E", starved, (2,), 4, {e: T for e in range(4)}),
            ("one token", torch.tensor([[3.0, 1.0, 2.0, 0.0]]), (), 2, {0: 1, 1: 0, 2: 1, 3: 0}),
            ("a group of two tiles", two_tiles, (), 1, {0: 190, 1: 10})]


def routing_of(x, router, k, counts):
    """asserts the gap between consecutive logits down to the first one left out, and the `counts`, as ``x`` routes on its device"""
    ordered = torch.sort(x @ router.t(), -1, descending=True)[0]
    gaps = (ordered[:, :-1] - ordered[:, 1:])[:, :k]
    assert gaps.numel() == 0 or float(gaps.min()) > ROUTING_GAP, float(gaps.min())
    experts = torch.topk(x @ router.t(), k, -1)[1]
    assert {e: int((experts == e).sum()) for e in counts} == counts


@pytest.mark.parametrize("name,logits,dead,k,counts", moe_routing_cases(), ids=[c[0] for c in moe_routing_cases()])
def test_moe_routing_edges_are_the_composition(name, logits, dead, k, counts):
    g = torch.Generator().manual_seed(13)
    E, D, H = logits.shape[1], 64, 96
    _, up, down = moe_weights(g, E, D, H)
    router, x = routed(g, logits, D, dead)
    assert all(not router[e].any() for e in dead)
    routing_of(x, router, k, counts)
    moe = MXMoEFeedForward.from_float(router, *up, *down, k)
    y = moe(x)
    assert y.shape == x.shape and not y.isnan().any() and bits(y, moe_composition(x, router, up, down, k))
    xa = MXActivation(*codes_of(x, "mxfp6_e2m3"), "mxfp6_e2m3")
    routing_of(xa.dequantize(), router, k, counts)
    assert bits(moe(xa), moe_composition(xa, router, up, down, k))


# ---- the C ABI without a GPU: layout of the descriptors, and the checks that come before anything is enqueued --------------------
def test_descriptors_have_the_headers_layout(tmp_path):
    import ctypes
    import os
    import subprocess
    from qsparse_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = {"qs_mx_grouped_matmul_args": _hip.MxGroupedMatmulArgs, "qs_mx_grouped_matmul_q_args": _hip.MxGroupedMatmulQArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(root, "include", "qsparse_hip.h")}"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append(f'printf("{cname} %zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {fname}));' for fname, _ in ct._fields_]
        lines.append('printf("\\n");')
    (tmp_path / "layout.c").write_text("\n".join(lines + ['return 0; }']))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    for line, (cname, ct) in zip(out, pairs.items()):
        name, size, *offsets = line.split()
        assert name == cname and int(size) == ctypes.sizeof(ct)
        assert [int(o) for o in offsets] == [getattr(ct, f).offset for f, _ in ct._fields_], cname


def test_entry_points_validate_in_bmms_order_without_a_gpu():
    import ctypes
    from qsparse_amd import _hip
    lib = _hip.load()
    ARG, DTYPE, ALIGN = -2, -1, -3
    VEC, PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN
    for fn in (lib.qs_mx_grouped_matmul_v, lib.qs_mx_grouped_matmul_route, lib.qs_mx_grouped_matmul_q_v, lib.qs_mx_grouped_matmul_q_route):
        assert fn(None) == ARG

    def desc(cls, **kw):
        a = cls()
        a.struct_size = ctypes.sizeof(a)
        a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.offs = 1024, 2048, 4096, 8192, 512
        a.T, a.E, a.N, a.K = 15, 3, 8, 64
        if cls is _hip.MxGroupedMatmulArgs:
            a.y = 1 << 30
        else:
            a.out_codes, a.out_scales = 1 << 30, 1 << 31
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    for cls, route in ((_hip.MxGroupedMatmulArgs, lib.qs_mx_grouped_matmul_route), (_hip.MxGroupedMatmulQArgs, lib.qs_mx_grouped_matmul_q_route)):
        assert route(desc(cls)) == VEC
        assert route(desc(cls, K=40)) == PLAIN                                          # K % 16 != 0
        assert route(desc(cls, b_codes=4097)) == PLAIN and route(desc(cls, a_codes=1025)) == PLAIN      # a base off the 16-byte grid
        assert route(desc(cls, bias=64, bias_batch_stride=8)) == VEC
        assert route(desc(cls, bias=64, bias_batch_stride=4)) == ARG                    # neither 0 nor N
        assert route(desc(cls, a_scales=None)) == ARG and route(desc(cls, b_format=5)) == ARG and route(desc(cls, E=-1)) == ARG
        assert route(desc(cls, b_codes=None)) == ARG and route(desc(cls, offs=None)) == ARG
        assert route(desc(cls, E=0, b_codes=None, b_scales=None, offs=None)) == VEC     # no groups: every row is a tail row
        assert route(desc(cls, E=1024)) == VEC and route(desc(cls, E=4096)) == VEC and route(desc(cls, E=4097)) == ARG
        assert route(desc(cls, bias=66)) == ALIGN and route(desc(cls, offs=514)) == ALIGN
        assert route(desc(cls, offs=514, E=-1)) == ARG                                  # the arguments come before the alignment
        for empty in ("T", "N"):
            assert route(desc(cls, **{empty: 0})) == 0
        assert route(desc(cls, K=0)) == ARG and route(desc(cls, K=0, T=0)) == 0
        assert route(desc(cls, T=1 << 40, K=1 << 24)) == ARG                            # T K beyond INT64_MAX
        assert route(desc(cls, E=4096, N=1 << 26, K=1 << 26)) == ARG                    # E N K beyond INT64_MAX
        assert route(desc(cls, T=1 << 40, N=1 << 24, K=1)) == ARG                       # T N beyond INT64_MAX
        assert route(desc(cls, T=1 << 38, N=1, K=1)) == ARG                             # more work-groups than a grid holds
        assert route(desc(cls, T=(1 << 38) - 127 * 4096, E=4095, N=1, K=1)) == ARG      # ... the E + 1 spare tiles count: 2^31
        if cls is _hip.MxGroupedMatmulArgs:             # (the codes-out form refuses these addresses: 2^38 rows from 1024 on overlap)
            assert route(desc(cls, T=(1 << 38) - 127 * 4096 - 128, E=4095, N=1, K=1)) == PLAIN     # 2^31 - 1 work-groups
    f = _hip.MxGroupedMatmulArgs
    assert lib.qs_mx_grouped_matmul_route(desc(f, y=None)) == ARG
    assert lib.qs_mx_grouped_matmul_route(desc(f, ydt=7, y=(1 << 20) + 1, E=-1)) == ARG         # the arguments come before the dtype
    assert lib.qs_mx_grouped_matmul_route(desc(f, ydt=7, y=(1 << 20) + 1)) == DTYPE             # ... the dtype before the alignment
    assert lib.qs_mx_grouped_matmul_route(desc(f, y=(1 << 20) + 2)) == ALIGN
    assert lib.qs_mx_grouped_matmul_route(desc(f, ydt=_hip._DT[torch.bfloat16], y=(1 << 20) + 2)) == VEC
    q, qroute = _hip.MxGroupedMatmulQArgs, lib.qs_mx_grouped_matmul_q_route
    assert qroute(desc(q, out_scales=None)) == ARG and qroute(desc(q, out_format=9)) == ARG and qroute(desc(q, act=2)) == ARG
    # out_codes [15, 8] = 120 bytes may not share a byte with a_codes [15, 64] = 960 bytes at 1024 or b_codes [3, 8, 64] at 4096
    assert qroute(desc(q, out_codes=1024 + 959)) == ARG and qroute(desc(q, out_codes=1024 + 960)) > 0
    assert qroute(desc(q, out_codes=4096 - 120)) > 0 and qroute(desc(q, out_codes=4096 - 119)) == ARG
    assert qroute(desc(q, out_codes=4096 + 3 * 8 * 64 - 1)) == ARG                      # the LAST weight of b_codes counts
    assert qroute(desc(q, out_codes=4096 + 8, E=0, b_codes=None, b_scales=None, offs=None)) > 0        # no weight to overlap
