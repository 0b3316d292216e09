"""The MX rotary embedding on the GPU against the CPU path (tests/test_mx_rope.py pins that to the definition): bytes equal, for both
kernels -- qs_mx_rope_v and qs_mx_rope_quant2_v -- on both routes, every dtype, both layouts, forward and inverse, dense and strided x.

d covers the block of 32, the 64-column tile edge, a partner in the same tile (d <= 64) and in another (d = 128, 192) and h off the
vector width (8, 72); T covers the block along T, the 128-row tile edge and, through T % 16, 16-byte against byte stores of the col
pair.  The route is asserted for every launch from the header's conditions."""
import pytest
import torch

import mx_rope_ref as RR
import test_mx_rope as TR
from qsparse_amd import _hip, mx_attention, mx_rope, mx_rope_quantize, mx_rope_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_ROPE_ROUTE_VEC, _hip.MX_ROPE_ROUTE_PLAIN
DS = (2, 8, 30, 32, 64, 72, 128, 192)
TS = (1, 16, 31, 33, 128, 129)
RF, CF = "mxfp8_e4m3", "mxfp8_e5m2"
_tables = {}


def tables(T, d):
    if (T, d) not in _tables:
        cos, sin = RR.tables(T, d, T + d)
        _tables[T, d] = (cos, sin, cos.to(DEV), sin.to(DEV))
    return _tables[T, d]


def route_of(x, interleaved, col):
    """the header's conditions for QS_MX_ROPE_ROUTE_VEC on the view `x` [..., T, d] (at most two leading dimensions; fresh, 16-byte
    aligned tables and outputs); `col`: a col pair is written (None: the dense call)"""
    T, d = x.shape[-2:]
    v = 4 if x.dtype == torch.float32 else 8
    strides = [s for n, s in zip(x.shape[:-1], x.stride()[:-1]) if n > 1]
    vec = d % v == 0 and x.data_ptr() % 16 == 0 and all(s % v == 0 for s in strides) and (interleaved or (d // 2) % v == 0)
    if col:
        vec = vec and T % 16 == 0
    return VEC if vec else PLAIN


def check(x_cpu, x_dev, interleaved, inverse, pairs=((RF, CF),), dense=True):
    T, d = x_cpu.shape[-2:]
    cos, sin, dcos, dsin = tables(T, d)
    kw = dict(interleaved=interleaved, inverse=inverse)
    what = (tuple(x_cpu.shape), x_cpu.dtype, kw)
    for rf, cf in pairs:
        want = mx_rope_quantize(x_cpu, cos, sin, row_fmt=rf, col_fmt=cf, **kw)
        got = mx_rope_quantize(x_dev, dcos, dsin, row_fmt=rf, col_fmt=cf, **kw)
        assert _hip.mx_rope_quant2_last_route == route_of(x_dev, interleaved, cf is not None), (what, rf, cf)
        for name, g, w in zip(("row_codes", "row_scales", "col_codes", "col_scales"), got, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert g.shape == w.shape and g.is_contiguous() and torch.equal(g.cpu(), w), (name, what, rf, cf)
    if dense:
        for od in (x_cpu.dtype, torch.float32):
            want = mx_rope(x_cpu, cos, sin, out_dtype=od, **kw)
            got = mx_rope(x_dev, dcos, dsin, out_dtype=od, **kw)
            assert _hip.mx_rope_last_route == route_of(x_dev, interleaved, None), what
            assert got.dtype == od and got.is_contiguous() and RR.same_bits(got.cpu(), want), (what, od)


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("dtype", RR.DTS, ids=str)
def test_dense_shapes(dtype, interleaved):
    n = 0
    for d in DS:
        for T in TS:
            G, inverse = (1, 3)[n % 2], bool((n // 2 + n // 12) % 2)     # both G and both directions at every d and at every T
            n += 1
            x = RR.inputs(d * 1000 + T, (G, T, d), dtype)
            check(x, x.to(DEV), interleaved, inverse)


def test_the_route_is_vec_where_everything_is_aligned():
    for dtype in RR.DTS:
        for interleaved in (False, True):
            x = RR.inputs(1, (3, 16, 64), dtype).to(DEV)
            assert route_of(x, interleaved, True) == VEC and route_of(x[:, :15], interleaved, True) == PLAIN
            check(x.cpu(), x, interleaved, False)
            assert _hip.mx_rope_quant2_last_route is not None and _hip.mx_rope_last_route == VEC
    assert route_of(torch.empty(1, 16, 8, dtype=torch.bfloat16, device=DEV), False, True) == PLAIN           # h = 4 off the vector of 8
    assert route_of(torch.empty(1, 16, 8, dtype=torch.bfloat16, device=DEV), True, True) == VEC
    assert route_of(torch.empty(1, 16, 8, dtype=torch.float32, device=DEV), False, True) == VEC


@pytest.mark.parametrize("dtype", RR.DTS, ids=str)
def test_strided_views(dtype):
    B, H = 2, 3
    for T, d in ((16, 64), (33, 72), (129, 8), (16, 128)):
        for interleaved in (False, True):
            # the heads of a [B, T, H, d] projection output
            x = RR.inputs(T + d, (B, T, H, d), dtype)
            xd = x.to(DEV)
            check(x.transpose(1, 2), xd.transpose(1, 2), interleaved, False)
            # q, k, v as chunks of a packed [B, T, 3 H d] projection
            packed = RR.inputs(T + d + 1, (B, T, 3 * H * d), dtype)
            pd = packed.to(DEV)
            for c, cd in zip(packed.chunk(3, -1)[1:], pd.chunk(3, -1)[1:]):
                check(c.view(B, T, H, d).transpose(1, 2), cd.view(B, T, H, d).transpose(1, 2), interleaved, True, dense=interleaved)
            # a base one element off
            flat = RR.inputs(T + d + 2, (1, 1, 1 + 3 * T * d), dtype).reshape(-1)
            fd = flat.to(DEV)
            off = fd[1:].view(3, T, d)
            assert route_of(off, interleaved, True) == PLAIN
            check(flat[1:].view(3, T, d), off, interleaved, False)
    # more leading stride levels than the kernel addresses: through a contiguous copy, the same bits
    x = RR.inputs(3, (2, 2, 2, 33, 8), dtype)[:, :, :1]
    x6 = RR.inputs(4, (2, 3, 4, 16, 64), dtype)[:, ::2, ::2]
    for t in (x, x6):
        T, d = t.shape[-2:]
        cos, sin, dcos, dsin = tables(T, d)
        got = mx_rope_quantize(t.to(DEV), dcos, dsin, row_fmt=RF, col_fmt=CF)
        for g, w in zip(got, mx_rope_quantize(t, cos, sin, row_fmt=RF, col_fmt=CF)):
            assert torch.equal(g.cpu(), w)
        assert RR.same_bits(mx_rope(t.to(DEV), dcos, dsin).cpu(), mx_rope(t, cos, sin))


def test_each_pair_alone_and_every_format():
    for T, d in ((16, 64), (33, 72)):
        for dtype in RR.DTS:
            x = RR.inputs(T * d, (3, T, d), dtype)
            check(x, x.to(DEV), False, False, pairs=((RF, None), (None, CF), ("mxfp4_e2m1", "mxfp6_e3m2"), ("mxfp6_e2m3", None)), dense=False)
            check(x, x.to(DEV), True, True, pairs=((RF, None), (None, CF)), dense=False)


def test_empty_tensors_launch_nothing():
    cos, sin = torch.empty(0, 4, device=DEV), torch.empty(0, 4, device=DEV)
    x = torch.empty(2, 0, 8, device=DEV)
    out = mx_rope_quantize(x, cos, sin, row_fmt=RF, col_fmt=CF)
    assert _hip.mx_rope_quant2_last_route is None and [tuple(t.shape) for t in out] == [(2, 0, 8), (2, 0, 1), (2, 8, 0), (2, 8, 0)]
    assert mx_rope(x, cos, sin).shape == (2, 0, 8) and _hip.mx_rope_last_route is None
    c2, s2 = (t.to(DEV) for t in RR.tables(4, 8))
    assert mx_rope(torch.empty(0, 4, 8, device=DEV), c2, s2).shape == (0, 4, 8) and _hip.mx_rope_last_route is None


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
def test_special_values_reach_both_outputs_of_the_pair(interleaved):
    """NaN, +-Inf and -0.0 planted in ONE element of a pair: both outputs of the pair, their row blocks and their column blocks must be
    the CPU's bytes (a NaN / Inf block: scale 0xFF, codes 0), on both routes"""
    for T in (16, 33):                                             # VEC and PLAIN at d = 64
        for dtype in RR.DTS:
            x = RR.inputs(T, (2, T, 64), dtype)
            for i, val in enumerate((float("nan"), float("inf"), float("-inf"), -0.0)):
                x[0, (3 * i) % T, 5 + 7 * i] = val                 # a first element (half: column < 32) or either (interleaved)
                x[1, (5 * i + 1) % T, 40 + 3 * i] = val            # a second element (half)
            x[1, 0, :] = 0.0
            x[1, 0, 1] = -0.0                                      # a row of zeros with one negative zero
            check(x, x.to(DEV), interleaved, False)
            check(x, x.to(DEV), interleaved, True, dense=False)


def test_attention_with_a_longer_key_sequence():
    B, H, T, S, d = 2, 2, 5, 40, 32
    q, k, v = RR.inputs(1, (B, H, T, d), torch.bfloat16), RR.inputs(2, (B, H, S, d), torch.bfloat16), RR.inputs(3, (B, H, S, d), torch.bfloat16)
    ck, sk = mx_rope_table(S, d)
    cq, sq = mx_rope_table(T, d, positions=torch.arange(S - T, S))
    rope = (cq, sq, ck, sk)
    drope = tuple(t.to(DEV) for t in rope)
    for softmax in ("torch", "fused"):
        for interleaved in (False, True):
            qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
            got = mx_attention(qd, kd, vd, softmax=softmax, rope=drope, rope_interleaved=interleaved)
            # the products (and torch.softmax) are not the same bits on the two devices -- the rotation is: what the keyword adds, the
            # codes of the rotated q and k, against the CPU's bytes, and the attention, on the device, against the attention on the
            # float32 rotations (tests/test_mx_softmax_gpu.py compares the fused attention with its composition the same way)
            for t, td, c, s, cd, sd in ((q, qd, cq, sq, drope[0], drope[1]), (k, kd, ck, sk, drope[2], drope[3])):
                for g, w in zip(mx_rope_quantize(td, cd, sd, row_fmt=RF, interleaved=interleaved)[:2],
                                mx_rope_quantize(t, c, s, row_fmt=RF, interleaved=interleaved)[:2]):
                    assert torch.equal(g.cpu(), w), (softmax, interleaved)
            q32 = mx_rope(qd, drope[0], drope[1], interleaved=interleaved, out_dtype=torch.float32)
            k32 = mx_rope(kd, drope[2], drope[3], interleaved=interleaved, out_dtype=torch.float32)
            assert torch.equal(got, mx_attention(q32, k32, vd, softmax=softmax)), (softmax, interleaved)
            assert RR.same_bits(q32.cpu(), mx_rope(q, rope[0], rope[1], interleaved=interleaved, out_dtype=torch.float32))
            assert bool(got.isfinite().all()) and not torch.equal(got, mx_attention(qd, kd, vd, softmax=softmax))


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
def test_fused_attention_train_is_its_composition_on_the_device(interleaved):
    for dtype in (torch.bfloat16, torch.float32):
        q, k, v, do, rope = TR.attention_operands(dtype, DEV)
        # the heads as a layer hands them over: strided views of a [B, T, H, d] tensor
        q = q.transpose(1, 2).contiguous().transpose(1, 2)
        got = TR.train_call(q, k, v, do, rope, interleaved, "fused")
        ref = TR.fused_composition(q, k, v, do, rope, interleaved)
        for name, g, r in zip(("o", "dq", "dk", "dv"), got, ref):
            assert g.dtype == dtype and torch.equal(g, r), (name, dtype)
        # and the device agrees with the CPU on every step that is defined bit for bit: the rotated pairs
        cpu = [t.cpu() for t in (q, rope[0], rope[1])]
        for g, w in zip(mx_rope_quantize(q, rope[0], rope[1], row_fmt=RF, col_fmt=RF, interleaved=interleaved),
                        mx_rope_quantize(cpu[0], cpu[1], cpu[2], row_fmt=RF, col_fmt=RF, interleaved=interleaved)):
            assert torch.equal(g.cpu(), w)


def test_graph_capture_and_two_replays():
    T, d = 33, 64
    cos, sin, dcos, dsin = tables(T, d)
    xs = [RR.inputs(i, (3, T, d), torch.bfloat16) for i in range(3)]
    static = xs[0].to(DEV)
    run = lambda: mx_rope_quantize(static, dcos, dsin, row_fmt=RF, col_fmt=CF)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for x in xs[1:]:
        static.copy_(x.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(out, mx_rope_quantize(x, cos, sin, row_fmt=RF, col_fmt=CF)):
            assert torch.equal(g.cpu(), w)
