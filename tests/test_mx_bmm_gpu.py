"""Batched matrix products on MX codes on the GPU (qs_mx_bmm_v, qs_mx_bmm_q_v).  The main property is the slice identity: slice g of
``mx_bmm`` is bit for bit ``mx_matmul`` of slice g, for all 25 format pairs, with the route of every launch asserted.  The operands
are from the exact class of tests/mx_gemm_ref.py with a different scale base per slice, so a kernel that reads slice 0 for every g, or
strides the scales by the code stride, cannot pass; the same operands are checked against the float64 reference too, which guards
against a bug shared with ``mx_matmul``."""
import pytest
import torch
import torch.nn as nn

import mx_gemm_ref as G
import qsparse_amd as qs
from qsparse_amd import MXMultiheadAttention, _hip, mx_attention, mx_bmm, mx_matmul, quantize_with_mx
from qsparse_amd.mx_gemm import MXLinear

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
VEC, PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN
SHAPES = [(1, 300, 128), (15, 17, 129), (127, 129, 33), (129, 16, 127), (128, 127, 32), (17, 15, 1), (197, 64, 64), (197, 64, 197),
          (130, 132, 256)]
GS = (1, 2, 3, 5)
PER_PAIR = 4          # shapes per pair; see shapes_of


def shapes_of(fa, fb):
    """PER_PAIR of the 9 shapes for the pair, walking the list by the pair's index.  The pairs whose A is one FP8 format have indices
    5 ia .. 5 ia + 4: 20 consecutive draws, which cover every shape twice -- and so for FP6 and FP4 (asserted below)"""
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


def batched_case(g, Gn, M, N, K, fa, fb):
    """exact-class operands [Gn, ., K] on the CPU, slice s with the scale bases 120 + 3 s (A) and 134 - 3 s (B): every slice differs
    from every other in both operands' scales, and the products stay near 2^0, where acc + bias is exact in float32 as well"""
    ra, rb = G.scale_windows(K, fa, fb)
    G.assert_exact_class(K, fa, fb, ra, rb)
    a = [G.exact_operand(g, M, K, fa, ra, 120 + 3 * s) for s in range(Gn)]
    b = [G.exact_operand(g, N, K, fb, rb, 134 - 3 * s) for s in range(Gn)]
    return (torch.stack([c for c, _ in a]), torch.stack([s for _, s in a]), torch.stack([c for c, _ in b]), torch.stack([s for _, s in b]))


def slice_bias(bias, s):
    return None if bias is None else (bias if bias.dim() == 1 else bias[s])


def stacked(ops, fa, fb, bias=None, dt=torch.float32, route=None, **kw):
    """torch.stack of mx_matmul over the slices (a tuple of stacks with out_fmt), each launch on `route`"""
    outs = []
    for s in range(ops[0].shape[0]):
        outs.append(mx_matmul(ops[0][s], ops[1][s], fa, ops[2][s], ops[3][s], fb, slice_bias(bias, s), dt, **kw))
        if route is not None:
            last = _hip.mx_gemm_last_route if kw.get("out_fmt") is None else _hip.mx_gemm_q_last_route
            assert last == route, (last, route)
    return torch.stack(outs) if kw.get("out_fmt") is None else tuple(torch.stack([o[j] for o in outs]) for j in range(2))


def reference(cpu, fa, fb, bias, dt):
    """the float64 definition per slice, rounded once to `dt`.  The sum of the definition starts at +0 (include/qsparse_hip.h, "MX
    matrix product": a -0 product sums to +0), which a float64 matmul over K = 1 does not do by itself: hence the `+ 0.0`"""
    return torch.stack([(G.reference(cpu[0][s], cpu[1][s], fa, cpu[2][s], cpu[3][s], fb, slice_bias(bias, s), dt)[1] + 0.0).to(dt)
                        for s in range(cpu[0].shape[0])])


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_slice_identity_and_float64_reference(fa, fb):
    g = torch.Generator().manual_seed(500 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    for i, (M, N, K) in shapes_of(fa, fb):
        Gn = GS[i % len(GS)]
        cpu = batched_case(g, Gn, M, N, K, fa, fb)
        dev = tuple(t.to(DEV) for t in cpu)
        route = VEC if K % 16 == 0 else PLAIN
        for bias in (None, torch.randint(-64, 64, (N,), generator=g).float(), torch.randint(-64, 64, (Gn, N), generator=g).float()):
            bdev = None if bias is None else bias.to(DEV)
            for dt in (torch.float32,) + ((torch.bfloat16, torch.float16) if i % 3 == 0 else ()):
                what = (fa, fb, Gn, M, N, K, None if bias is None else tuple(bias.shape), dt)
                y = mx_bmm(dev[0], dev[1], fa, dev[2], dev[3], fb, bdev, dt)
                assert _hip.mx_bmm_last_route == route, (_hip.mx_bmm_last_route, what)
                assert y.is_cuda and y.dtype == dt and y.shape == (Gn, M, N)
                assert G.same(y, stacked(dev, fa, fb, bdev, dt, route)), ("slice identity", what)
                assert G.same(y, reference(cpu, fa, fb, bias, dt)), ("float64 reference", what)


def offset_by_one(t):
    """the same bytes on the device at a base one byte past a 16-byte boundary (a slice of a larger allocation)"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    return view


@pytest.mark.parametrize("fa,fb", [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp8_e5m2")])
def test_offset_bases_take_the_byte_loads_with_the_same_bits(fa, fb):
    g = torch.Generator().manual_seed(21)
    cpu = batched_case(g, 3, 129, 130, 256, fa, fb)
    aligned = tuple(t.to(DEV) for t in cpu)
    y = mx_bmm(aligned[0], aligned[1], fa, aligned[2], aligned[3], fb)
    assert _hip.mx_bmm_last_route == VEC
    for shifted in ((0,), (2,), (0, 1, 2, 3)):                     # either code base alone, then all four operands
        ops = tuple(offset_by_one(t) if j in shifted else t for j, t in enumerate(aligned))
        z = mx_bmm(ops[0], ops[1], fa, ops[2], ops[3], fb)
        assert _hip.mx_bmm_last_route == PLAIN and G.same(z, y), shifted
    assert G.same(y, reference(cpu, fa, fb, None, torch.float32))


@pytest.mark.parametrize("fa,fb", [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e3m2", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp4_e2m1")])
def test_ff_scale_byte_gives_nan_in_its_row_of_its_slice_only(fa, fb):
    g = torch.Generator().manual_seed(22)
    for M, N, K, route in ((140, 70, 256, VEC), (33, 130, 100, PLAIN)):
        base = batched_case(g, 3, M, N, K, fa, fb)
        for side in ("a", "b"):
            ac, asc, bc, bsc = (t.clone() for t in base)
            nan = torch.zeros(3, M, N, dtype=torch.bool)
            if side == "a":
                asc[1, M - 1, asc.shape[-1] - 1] = 255
                nan[1, M - 1, :] = True
            else:
                bsc[2, 3, 0] = 255
                bc[2, 3, :32] = 0                                   # (as the quantizer writes such a block)
                nan[2, :, 3] = True
            cpu = (ac, asc, bc, bsc)
            dev = tuple(t.to(DEV) for t in cpu)
            y = mx_bmm(dev[0], dev[1], fa, dev[2], dev[3], fb)
            assert _hip.mx_bmm_last_route == route
            assert torch.equal(y.isnan().cpu(), nan), (side, M, N, K)
            assert G.same(y, stacked(dev, fa, fb)) and G.same(y, reference(cpu, fa, fb, None, torch.float32))


@pytest.mark.parametrize("fa,fb", [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp6_e2m3"), ("mxfp8_e5m2", "mxfp4_e2m1")])
@pytest.mark.parametrize("N", [64, 100, 33])
def test_codes_out_is_the_stacked_codes_out_matmul(fa, fb, N):
    g = torch.Generator().manual_seed(23 + N)
    Gn, M, K = 3, 130, 96 if N != 33 else 100
    route = VEC if K % 16 == 0 else PLAIN
    x, w = torch.randn(Gn, M, K, generator=g) * 2, torch.randn(Gn, N, K, generator=g) / K ** 0.5
    dev = tuple(quantize_with_mx(x.to(DEV), fa, -1, return_codes=True)[1:]) + tuple(quantize_with_mx(w.to(DEV), fb, -1, return_codes=True)[1:])
    biases = (None, torch.randn(N, generator=g).to(DEV), torch.randn(Gn, N, generator=g).to(DEV))
    for j, out_fmt in enumerate(G.FMTS):
        for act in (None, "relu"):
            bias = biases[(j + (act is not None)) % 3]
            codes, scales = mx_bmm(dev[0], dev[1], fa, dev[2], dev[3], fb, bias, out_fmt=out_fmt, act=act)
            assert _hip.mx_bmm_q_last_route == route
            assert codes.shape == (Gn, M, N) and scales.shape == (Gn, M, -(-N // 32)) and codes.dtype == scales.dtype == torch.uint8
            want = stacked(dev, fa, fb, bias, route=route, out_fmt=out_fmt, act=act)
            assert torch.equal(codes, want[0]) and torch.equal(scales, want[1]), (out_fmt, act)


def test_empty_products_enqueue_nothing():
    dev = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=DEV)
    for Gn, M, N in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
        y = mx_bmm(dev(Gn, M, 32), dev(Gn, M, 1), "mxfp8_e4m3", dev(Gn, N, 32), dev(Gn, N, 1), "mxfp4_e2m1")
        assert y.shape == (Gn, M, N) and _hip.mx_bmm_last_route is None
        c, s = mx_bmm(dev(Gn, M, 32), dev(Gn, M, 1), "mxfp8_e4m3", dev(Gn, N, 32), dev(Gn, N, 1), "mxfp4_e2m1", out_fmt="mxfp8_e4m3")
        assert c.shape == (Gn, M, N) and s.shape == (Gn, M, -(-N // 32)) and _hip.mx_bmm_q_last_route is None


# ---- attention and the layer: the composition run through per-slice mx_matmul ------------------------------------------------------
def codes_of(x, fmt):
    return tuple(quantize_with_mx(x, fmt, -1, return_codes=True)[1:])


def flat_stacked(ac, asc, fa, bc, bsc, fb, bias=None, dt=torch.float32):
    lead = tuple(ac.shape[:-2])
    ops = tuple(t.reshape((-1,) + tuple(t.shape[-2:])) for t in (ac, asc, bc, bsc))
    return stacked(ops, fa, fb, bias, dt).reshape(lead + (ac.shape[-2], bc.shape[-2]))


def attention_composition(q, k, v, mask=None, fmts=("mxfp8_e4m3",) * 3, dt=torch.float32):
    qk, pf, vf = fmts
    s = flat_stacked(*codes_of(q, qk), qk, *codes_of(k, qk), qk) * q.shape[-1] ** -0.5
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = torch.zeros(mask.shape, dtype=torch.float32, device=mask.device).masked_fill(~mask, float("-inf"))
        s = s + mask
    return flat_stacked(*codes_of(torch.softmax(s, -1), pf), pf, *codes_of(v.transpose(-1, -2).contiguous(), vf), vf, None, dt)


@pytest.mark.parametrize("S", [37, 50])
@pytest.mark.parametrize("d", [40, 64])
def test_attention_is_the_composition_through_matmul(S, d):
    g = torch.Generator().manual_seed(S + d)
    B, h, T = 2, 3, 37
    q, k, v = (torch.randn(B, h, n, d, generator=g).to(DEV) for n in (T, S, S))
    add = torch.randn(T, S, generator=g).to(DEV)
    boolean = torch.rand(B, 1, T, S, generator=g) > 0.3
    boolean[..., 0] = True
    boolean = boolean.to(DEV)
    causal = torch.ones(T, S, dtype=torch.bool, device=DEV).tril()
    for kw, mask in (({}, None), ({"attn_mask": add}, add), ({"attn_mask": boolean}, boolean), ({"is_causal": True}, causal)):
        y = mx_attention(q, k, v, **kw)
        assert _hip.mx_bmm_last_route == (VEC if S % 16 == 0 else PLAIN)            # the second product: K = S
        assert y.shape == (B, h, T, d) and not y.isnan().any() and G.same(y, attention_composition(q, k, v, mask)), kw
    fmts = ("mxfp6_e2m3", "mxfp4_e2m1", "mxfp8_e5m2")
    y = mx_attention(q, k, v, qk_fmt=fmts[0], p_fmt=fmts[1], v_fmt=fmts[2], out_dtype=torch.bfloat16)
    assert G.same(y, attention_composition(q, k, v, None, fmts, torch.bfloat16))


@pytest.mark.parametrize("d,batch_first", [(40, True), (64, False)])
def test_layer_is_the_composition_through_matmul(d, batch_first):
    torch.manual_seed(d)
    B, h, T = 2, 3, 37
    E = h * d
    mha = nn.MultiheadAttention(E, h, batch_first=batch_first)
    layer = MXMultiheadAttention.from_float(mha).to(DEV)
    x = (torch.randn(B, T, E) if batch_first else torch.randn(T, B, E)).to(DEV)
    lin = []
    for w, b in ((mha.in_proj_weight, mha.in_proj_bias), (mha.out_proj.weight, mha.out_proj.bias)):
        _, c, s = quantize_with_mx(w.detach(), "mxfp8_e4m3", 1, return_codes=True)
        lin.append(MXLinear(c, s, "mxfp8_e4m3", b.detach()).to(DEV))
    xb = x if batch_first else x.transpose(0, 1)
    q, k, v = (t.reshape(B, T, h, d).transpose(1, 2) for t in lin[0](xb).chunk(3, -1))
    causal = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    for kw, mask in (({}, None), ({"is_causal": True}, causal)):
        want = lin[1](attention_composition(q, k, v, mask).transpose(1, 2).reshape(B, T, E))
        y, w = layer(x, **kw)
        assert w is None and y.is_cuda and G.same(y, want if batch_first else want.transpose(0, 1)), kw
    ref = mha.to(DEV)(x, x, x, need_weights=False)[0]
    assert (layer(x)[0] - ref).abs().max() < 0.25 * ref.abs().max()


# ---- slices that fill the GPU by themselves: launched one by one inside the entry point (qs_mx_bmm.h, kMxbForwardTiles) ----------------
@pytest.mark.parametrize("fa,fb,K,off", [("mxfp8_e4m3", "mxfp6_e2m3", 32, 0), ("mxfp4_e2m1", "mxfp8_e5m2", 33, 0), ("mxfp6_e3m2", "mxfp4_e2m1", 64, 1)])
def test_large_slices_take_the_per_slice_launches_with_the_same_bits(fa, fb, K, off):
    """23 x 23 = 529 tiles a slice, past the threshold of 512; M, N no multiples of the tile, N % 4 != 0; y carved out of a
    pattern-filled allocation, so a slice offset that is off shows in the margins or in the next slice.  Against the stacked
    mx_matmul, the float64 reference, and the batched kernel itself on the same operands cut just below the threshold"""
    from mx_guard import guarded, intact
    Gn, M, N = 2, 2817, 2818 + off
    assert -(-M // 128) * -(-N // 128) == 529
    g = torch.Generator().manual_seed(31 + K)
    cpu = batched_case(g, Gn, M, N, K, fa, fb)
    dev = tuple((offset_by_one(t) if off else t.to(DEV)) for t in cpu)
    route = VEC if K % 16 == 0 and not off else PLAIN
    bias = torch.randint(-64, 64, (Gn, N), generator=g).float()
    raw, body = guarded(Gn * M * N * 4)
    y = _hip.mx_bmm(dev[0], dev[1], fa, dev[2], dev[3], fb, bias.to(DEV), torch.float32, out=body.view(torch.float32))
    torch.cuda.synchronize()
    assert _hip.mx_bmm_last_route == route and intact(raw, Gn * M * N * 4)
    assert G.same(y, stacked(dev, fa, fb, bias.to(DEV), torch.float32, route))
    assert G.same(y, reference(cpu, fa, fb, bias, torch.float32))
    # the batched kernel on the first 22 x 23 tiles of every slice (506 < 512): the same rows of y
    rows = 22 * 128
    cut = (dev[0][:, :rows].contiguous(), dev[1][:, :rows].contiguous(), dev[2], dev[3])
    assert G.same(mx_bmm(cut[0], cut[1], fa, cut[2], cut[3], fb, bias.to(DEV)), y[:, :rows])
    # codes out, shared [N] bias
    codes, scales = mx_bmm(dev[0], dev[1], fa, dev[2], dev[3], fb, bias[0].to(DEV), out_fmt="mxfp8_e4m3", act="relu")
    want = stacked(dev, fa, fb, bias[0].to(DEV), out_fmt="mxfp8_e4m3", act="relu")
    assert _hip.mx_bmm_q_last_route == route and torch.equal(codes, want[0]) and torch.equal(scales, want[1])
