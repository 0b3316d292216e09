"""The training side of the fused softmax on the GPU: the bytes of qs_mx_softmax_quant2_v and qs_mx_softmax_bwd_quant_v against the CPU
path (tests/test_mx_softmax_train.py pins that to the definition) at the shapes where the kernels change their path, the routes,
``mx_attention_train(softmax="fused")`` against its composition on the device, and one linear graph capture."""
import pytest
import torch

import mx_softmax_ref as SR
import test_mx_softmax_train as TT
from qsparse_amd import _hip, mx_attention_train, mx_softmax_backward_quantize, mx_softmax_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_SOFTMAX_ROUTE_VEC, _hip.MX_SOFTMAX_ROUTE_PLAIN
SCALE = TT.SCALE
FMT_PAIRS = tuple((SR.FMTS[i], SR.FMTS[(i + 2) % 5]) for i in range(5))


def dev(t):
    return t.to(DEV) if isinstance(t, torch.Tensor) else t


def same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (i, what)
        if g is not None:
            assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, (i, what)
            assert torch.equal(g.cpu().view(torch.uint8), w.contiguous().view(torch.uint8)), (i, what)       # (bytes: a NaN equals a NaN)


def check(s, dp, fmts, scale=SCALE, sr=(), route=None, bwd_route=None, pairs=(True, True), **kw):
    """the forward with both keywords and the backward op on the GPU against the CPU path of the same calls, bit for bit"""
    rf, cf = fmts
    what = (tuple(s.shape), s.dtype, dp.dtype, fmts, sorted(kw), sr != ())
    want = mx_softmax_quantize(s, scale=scale, fmt=rf, col_fmt=cf, return_stats=True, **kw)
    dkw = {k: dev(v) for k, v in kw.items()}
    got = mx_softmax_quantize(dev(s), scale=scale, fmt=rf, col_fmt=cf, return_stats=True, **dkw)
    if route is not None:
        assert _hip.mx_softmax_quant2_last_route == route, what
    same(got, want, what)
    bf = dict(row_fmt=cf if pairs[0] else None, col_fmt=rf if pairs[1] else None)
    cpu_sr = dict(zip(("rounding", "seed", "step"), sr))
    dev_sr = dict(zip(("rounding", "seed", "step"), tuple(dev(x) for x in sr)))
    wantb = mx_softmax_backward_quantize(dp, s, want[4], want[5], scale=scale, **bf, **cpu_sr, **kw)
    gotb = mx_softmax_backward_quantize(dev(dp), dev(s), got[4], got[5], scale=scale, **bf, **dev_sr, **dkw)
    if bwd_route is not None:
        assert _hip.mx_softmax_bwd_last_route == bwd_route, what
    same(gotb, wantb, what)


def inputs(seed, shape, dtype, ddtype):
    return SR.scores(seed, shape, dtype), torch.randn(shape, generator=torch.Generator().manual_seed(seed + 1)).to(ddtype)


@pytest.mark.parametrize("S", (1, 31, 32, 33, 63, 65, 72, 197, 1024, 1025, 1056))
def test_columns(S):
    """the block, the 64-column tile edge, VEC / PLAIN, the one-launch kernel's register-resident bound; every dtype of s and of dp, every
    format, every kind of mask, stochastic rounding with a device step"""
    vec = VEC if S % 32 == 0 else PLAIN
    step = torch.tensor([7], dtype=torch.int64)
    for i, (dtype, ddtype) in enumerate(((torch.float32, torch.float32), (torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16))):
        G, T = (3, 5) if S < 1000 else (1, 4)
        s, dp = inputs(100 * S + i, (G, T, S), dtype, ddtype)
        fm = FMT_PAIRS[(i + S) % 5]
        check(s, dp, fm, route=vec, bwd_route=PLAIN)             # (T % 16 != 0: the backward's col pair takes byte stores)
        check(s, dp, FMT_PAIRS[(i + S + 1) % 5], route=vec, bwd_route=vec, pairs=(True, False), mask=SR.float_mask(S, (T, S)))
        check(s, dp, FMT_PAIRS[(i + S + 2) % 5], mask=SR.bool_mask(S + 1, (G, T, S)), sr=("stochastic", 11, step))
        check(s, dp, FMT_PAIRS[(i + S + 3) % 5], is_causal=True, sr=("stochastic", 12, step), pairs=(False, True))
        check(s, dp, FMT_PAIRS[(i + S + 4) % 5], mask=SR.float_mask(S + 2, (G, T, S)))


@pytest.mark.parametrize("T", (1, 4, 5, 31, 33, 127, 129))
def test_rows(T):
    """rows per work-group of the row launches, the block of 32 along T, the 128-row tile edge; causal with T != S"""
    step = torch.tensor([3], dtype=torch.int64)
    for i, (G, S, dtype, ddtype) in enumerate(((1, 72, torch.float32, torch.bfloat16), (3, 40, torch.bfloat16, torch.float32),
                                               (3, 64, torch.float16, torch.float16))):
        s, dp = inputs(10 * T + i, (G, T, S), dtype, ddtype)
        check(s, dp, FMT_PAIRS[(T + i) % 5])
        check(s, dp, FMT_PAIRS[(T + i + 1) % 5], is_causal=True, sr=("stochastic", 5, step))
        check(s, dp, FMT_PAIRS[(T + i + 2) % 5], mask=SR.float_mask(T, (T, S)))


def test_whole_tiles_take_the_vector_stores():
    """T % 16 == 0: the col pairs leave in 16-byte stores; T = 144 has a second tile row with one 16-row run"""
    step = torch.tensor([1], dtype=torch.int64)
    for T, S in ((16, 64), (144, 96), (128, 32)):
        for dtype, ddtype in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)):
            s, dp = inputs(T + S, (2, T, S), dtype, ddtype)
            check(s, dp, FMT_PAIRS[0], route=VEC, bwd_route=VEC)
            check(s, dp, FMT_PAIRS[3], route=VEC, bwd_route=VEC, sr=("stochastic", 9, step), mask=SR.float_mask(T, (2, T, S)))
            check(s, dp, FMT_PAIRS[1], route=VEC, bwd_route=VEC, is_causal=True, sr=("stochastic", 9, step))


@pytest.mark.parametrize("scale", (0.0, -0.37))
def test_zero_and_negative_scale(scale):
    s, dp = inputs(11, (2, 3, 70), torch.float32, torch.float32)
    check(s, dp, FMT_PAIRS[0], scale=scale)
    s[1, 1, 4] = float("inf") if scale == 0.0 else float("-inf")             # that row alone becomes NaN
    check(s, dp, FMT_PAIRS[1], scale=scale)


@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
def test_exceptional_rows_on_the_gpu(dtype):
    import test_mx_softmax as TS
    s, mask, _ = TS._special_rows(dtype)
    dp = torch.randn(1, 9, 40, generator=torch.Generator().manual_seed(3))
    check(s, dp, FMT_PAIRS[0], mask=mask)
    dp[0, 4, 7], dp[0, 6, 39] = float("nan"), float("inf")
    check(s, dp, FMT_PAIRS[2], mask=mask)


def _off_by_one(t):
    """`t` on the device at a base off its 16 bytes by one element"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    off = flat[1:].view(t.shape).copy_(t)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    return off


def test_a_misaligned_base_takes_the_plain_route():
    """a base off its 16 bytes by one element, for s, for dp and for the mask alone, at a shape that takes VEC"""
    fmt, gf = "mxfp8_e4m3", "mxfp8_e5m2"
    for dtype in SR.DTS:
        s, dp = inputs(5, (2, 16, 64), dtype, dtype)
        mask = SR.float_mask(7, (16, 64))
        want = mx_softmax_quantize(s, mask, scale=SCALE, fmt=fmt, col_fmt=fmt, return_stats=True)
        wantb = mx_softmax_backward_quantize(dp, s, want[4], want[5], mask, scale=SCALE, row_fmt=gf, col_fmt=gf)
        for which in ("none", "s", "dp", "mask"):
            ds_, dd, dm = (_off_by_one(t) if which == n else t.to(DEV) for n, t in (("s", s), ("dp", dp), ("mask", mask)))
            got = mx_softmax_quantize(ds_, dm, scale=SCALE, fmt=fmt, col_fmt=fmt, return_stats=True)
            assert _hip.mx_softmax_quant2_last_route == (PLAIN if which in ("s", "mask") else VEC), (dtype, which)
            same(got, want, (dtype, which))
            gotb = mx_softmax_backward_quantize(dd, ds_, got[4], got[5], dm, scale=SCALE, row_fmt=gf, col_fmt=gf)
            assert _hip.mx_softmax_bwd_last_route == (VEC if which == "none" else PLAIN), (dtype, which)
            same(gotb, wantb, (dtype, which))


def test_stats_alone_and_empty_tensors():
    s = SR.scores(1, (2, 5, 197), torch.bfloat16)
    want = mx_softmax_quantize(s, scale=SCALE, return_stats=True, is_causal=True)
    got = mx_softmax_quantize(s.to(DEV), scale=SCALE, return_stats=True, is_causal=True)
    assert len(got) == 4
    same(got, want, "stats alone")
    base = mx_softmax_quantize(s.to(DEV), scale=SCALE, is_causal=True)      # the one-launch kernel: the same row pair
    assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1])
    for shape in ((0, 4, 33), (2, 0, 33), (2, 4, 0)):
        z = torch.zeros(shape, device=DEV)
        out = mx_softmax_quantize(z, col_fmt="mxfp8_e4m3", return_stats=True)
        assert _hip.mx_softmax_quant2_last_route is None and all(t.is_cuda for t in out)
        assert [tuple(t.shape) for t in out] == [tuple(t.shape) for t in mx_softmax_quantize(z.cpu(), col_fmt="mxfp8_e4m3", return_stats=True)]
        outb = mx_softmax_backward_quantize(z, z, out[4], out[5], row_fmt="mxfp8_e5m2", col_fmt="mxfp8_e5m2")
        assert _hip.mx_softmax_bwd_last_route is None and outb[0].shape == shape and outb[2].shape == (shape[0], shape[2], shape[1])


@pytest.mark.parametrize("c", TT.TRAIN_CASES, ids=("causal", "masked_bf16_sr"))
def test_attention_train_fused_equals_its_composition_on_the_gpu(c):
    dtype = c.get("dtype", torch.float32)
    q, k, v = (t.to(DEV) for t in TT._qkv(11, c["lead"], c["T"], c["S"], c["d"], c["dv"], dtype))
    do = torch.randn(*c["lead"], c["T"], c["dv"], generator=torch.Generator().manual_seed(12)).to(dtype).to(DEV)
    mask = SR.float_mask(13, (c["T"], c["S"])).to(DEV) if c.get("mask") else None
    fmts = c.get("fmts", ("mxfp8_e4m3",) * 3 + ("mxfp8_e5m2",))
    step = torch.tensor([3], dtype=torch.int64, device=DEV) if c.get("sr") else None
    sr = ("stochastic", 99, step) if c.get("sr") else ()
    want = TT.fused_train_composition(q, k, v, do, mask, c.get("causal", False), c.get("scale"), fmts,
                                      ("stochastic", 99, step.clone()) if c.get("sr") else ())
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = mx_attention_train(qg, kg, vg, mask, c.get("causal", False), c.get("scale"), qk_fmt=fmts[0], p_fmt=fmts[1], v_fmt=fmts[2],
                           grad_fmt=fmts[3], softmax="fused", **dict(zip(("grad_rounding", "seed", "step"), sr)))
    o.backward(do)
    for name, got, ref in zip(("o", "dq", "dk", "dv"), (o.detach(), qg.grad, kg.grad, vg.grad), want):
        assert got.dtype == ref.dtype and torch.equal(got, ref), name
        assert bool(torch.isfinite(got.float()).all()) and bool(got.float().abs().sum() > 0), name
    if step is not None:
        assert int(step) == 5


def test_captured_forward_and_backward_replay_bit_for_bit():
    """one linear capture (no parallel branches) of a forward and a backward op call, replayed once on new data with the stochastic
    step advanced on the device"""
    shape, fmt, gf = (3, 7, 197), "mxfp8_e4m3", "mxfp8_e5m2"
    first, second = inputs(1, shape, torch.float32, torch.bfloat16), inputs(3, shape, torch.float32, torch.bfloat16)
    mask = SR.float_mask(5, (7, 197))
    want = mx_softmax_quantize(second[0], mask, scale=SCALE, fmt=fmt, col_fmt=fmt, return_stats=True)
    wantb = mx_softmax_backward_quantize(second[1], second[0], want[4], want[5], mask, scale=SCALE, row_fmt=gf, col_fmt=gf,
                                         rounding="stochastic", seed=21, step=torch.tensor([1], dtype=torch.int64))
    static_s, static_dp, dmask = first[0].to(DEV), first[1].to(DEV), mask.to(DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)

    def both():
        f = mx_softmax_quantize(static_s, dmask, scale=SCALE, fmt=fmt, col_fmt=fmt, return_stats=True)
        b = mx_softmax_backward_quantize(static_dp, static_s, f[4], f[5], dmask, scale=SCALE, row_fmt=gf, col_fmt=gf,
                                         rounding="stochastic", seed=21, step=step)
        return f, b

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, outb = both()
    static_s.copy_(second[0].to(DEV))
    static_dp.copy_(second[1].to(DEV))
    step.add_(1)
    graph.replay()
    torch.cuda.synchronize()
    same(out, want, "forward")
    same(outb, wantb, "backward")
