"""The fused MoE routing on the GPU, bit for bit against its definitions on the CPU: ``mx_moe_route`` at the smallest shapes that reach
each mechanism (one tile, two, three with a ragged last one, every register variant, dense ties, empty experts, a NaN row),
``mx_moe_dispatch_quantize`` against ``quantize_with_mx`` of the token's row between guard bytes, ``mx_moe_combine`` against
``_combine_def``, and the two blocks with ``routing="fused"`` against the composition that defines them."""
import pytest
import torch

import mx_guard as G
from qsparse_amd import (MXActivation, MXGatedMoEFeedForward, MXMoEFeedForward, _hip, mx_moe_combine, mx_moe_dispatch_quantize, mx_moe_route,
                         quantize_with_mx)
from qsparse_amd.mx_moe import _combine_def, _route_def

pytestmark = pytest.mark.gpu
DEV = G.DEV
E4, F4 = "mxfp8_e4m3", "mxfp4_e2m1"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def drawn(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def same_bits(a, b):
    """equal as bytes (-0 is not +0), a NaN equal to any NaN in the same place"""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        if not torch.equal(a.isnan(), b.isnan()):
            return False
        a, b = a.nan_to_num(nan=0.0, posinf=None, neginf=None), b.nan_to_num(nan=0.0, posinf=None, neginf=None)
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def logits_of(kind, T, E):
    x = drawn(T * 1031 + E, T, E)
    if kind == "one_expert":         # every token's first pick is expert E - 1: with k < E the others' counts are small or 0, offs repeats
        x = x * 1e-3
        x[:, E - 1] = 5.0
        x[:, : E // 2] = -9.0 - torch.arange(E // 2)       # ... and the lower half is never picked while k <= E - E // 2
    elif kind == "ties":             # four distinct values
        x = (x * 1.5).round().clamp(-1, 2)
        x = torch.where((x == 0) & (torch.arange(E) % 2 == 1), torch.tensor(-0.0), x)       # ... of which 0 comes with either sign
    elif kind == "nan_row" and T:
        x[T // 2] = float("nan")
        x[0, 0] = float("nan")
    return x


@pytest.mark.parametrize("kind", ("drawn", "one_expert", "ties", "nan_row"))
@pytest.mark.parametrize("T, E, k", ((1, 5, 2), (7, 64, 8), (65, 130, 3), (300, 1024, 32), (0, 8, 2), (150, 20, 20)))
def test_route_equals_its_definition(T, E, k, kind):
    x = logits_of(kind, T, E)
    got = mx_moe_route(x.to(DEV), k)
    want = _route_def(x, k)
    for name, a, b in zip(("gates", "experts", "offs", "order", "inv"), got, want):
        assert same_bits(a, b), name
    assert _hip.mx_moe_route_last_route == (None if T == 0 else _hip.MX_MOE_ROUTE_ONE if T <= 64 else _hip.MX_MOE_ROUTE_TILED)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_input_dtypes_and_strided_rows(dtype):
    x = logits_of("drawn", 70, 200).to(dtype)
    wide = torch.zeros(70, 333, dtype=dtype)
    wide[:, :200] = x
    want = _route_def(x, 6)
    for arg in (x.to(DEV), wide.to(DEV)[:, :200]):
        assert all(same_bits(a, b) for a, b in zip(mx_moe_route(arg, 6), want))


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32))
@pytest.mark.parametrize("fmt", (E4, F4))
@pytest.mark.parametrize("D", (32, 96, 200))
def test_dispatch_equals_the_quantizer_of_the_tokens_row(D, fmt, dtype):
    T, k, nb = 9, 3, -(-D // 32)
    x = (drawn(D, T, D) * torch.logspace(-3, 3, T)[:, None]).to(dtype)
    inv = torch.randperm(T * k, generator=torch.Generator().manual_seed(D)).to(torch.int32).reshape(T, k)
    _, c, s = quantize_with_mx(x, fmt, -1, return_codes=True)
    flat, token = inv.reshape(-1).long(), torch.arange(T).repeat_interleave(k)
    want_c, want_s = torch.empty(T * k, D, dtype=torch.uint8), torch.empty(T * k, nb, dtype=torch.uint8)
    want_c[flat], want_s[flat] = c[token], s[token]
    wide = torch.zeros(T, D + 40, dtype=dtype)
    wide[:, 8:D + 8] = x
    for arg in (x.to(DEV), wide.to(DEV)[:, 8:D + 8], wide.to(DEV)[:, 8:D + 8][:, 1:], MXActivation(c.to(DEV), s.to(DEV), fmt)):
        if isinstance(arg, torch.Tensor) and arg.shape[1] != D:         # an odd base: the PLAIN route on a narrower problem
            got = mx_moe_dispatch_quantize(arg, inv.to(DEV), fmt)
            _, c1, s1 = quantize_with_mx(x[:, 1:], fmt, -1, return_codes=True)
            assert _hip.mx_moe_dispatch_last_route == _hip.MX_MOE_DISPATCH_ROUTE_PLAIN
            assert torch.equal(got[0].cpu()[flat], c1[token]) and torch.equal(got[1].cpu()[flat], s1[token])
            continue
        got = mx_moe_dispatch_quantize(arg, inv.to(DEV), None if isinstance(arg, MXActivation) else fmt)
        assert torch.equal(got[0].cpu(), want_c) and torch.equal(got[1].cpu(), want_s)
    # an entry out of range between guard bytes: nothing is stored for it, its row and the margins keep their bytes
    bad = inv.clone()
    bad[2, 1], bad[5, 0] = T * k, -1
    raws, outs = zip(*(G.guarded(T * k * n) for n in (D, nb)))
    _hip.mx_moe_dispatch(x.to(DEV), None, None, bad.to(DEV), fmt, out=outs)
    assert all(G.intact(raw, T * k * n) for raw, n in zip(raws, (D, nb)))
    for out, want, n in zip(outs, (want_c, want_s), (D, nb)):
        out, keep = out.cpu().view(T * k, n), torch.ones(T * k, dtype=torch.bool)
        keep[[int(inv[2, 1]), int(inv[5, 0])]] = False
        assert torch.equal(out[keep], want[keep]) and bool((out[~keep] == G.PATTERN).all())


@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("D", (4, 100, 130))
def test_combine_equals_its_definition(D, k):
    T = 70
    inv = torch.randperm(T * k, generator=torch.Generator().manual_seed(D + k)).to(torch.int32).reshape(T, k)
    gates = torch.softmax(drawn(k, T, k), -1)
    inv[3, k - 1], gates[5, 0] = T * k, float("nan")
    for ydt, odt in zip(DTYPES, DTYPES if D == 100 else (torch.float32,) * 3):
        y = drawn(D, T * k, D).to(ydt)
        got = mx_moe_combine(y.to(DEV), inv.to(DEV), gates.to(DEV), odt)
        assert same_bits(got, _combine_def(y, inv, gates, odt)), (ydt, odt)
        assert _hip.mx_moe_combine_last_route == (_hip.MX_MOE_DISPATCH_ROUTE_PLAIN if D == 130 else _hip.MX_MOE_DISPATCH_ROUTE_VEC)
    assert bool(got[5].isnan().all()) and not bool(got[3].isnan().any())


def blocks(routing):
    T, E, D, H, k = 70, 5, 64, 64, 2
    w = [drawn(i, *s) * 0.3 for i, s in enumerate(((E, D), (E, H, D), (E, H, D), (E, D, H), (E, H), (E, D)))]
    w = [t.to(DEV) for t in w]
    plain = MXMoEFeedForward.from_float(w[0], w[1], w[4], w[3], w[5], k, routing=routing)
    gated = MXGatedMoEFeedForward.from_float(w[0], w[1], w[4], w[2], w[4], w[3], w[5], k, routing=routing)
    return plain, gated, drawn(9, T, D).to(DEV)


@pytest.mark.parametrize("which", (0, 1))
def test_fused_block_equals_the_composition_that_defines_it(which):
    moe, x = blocks("fused")[which], blocks("fused")[2]
    for arg in (x, x.bfloat16(), MXActivation(*quantize_with_mx(x, E4, -1, return_codes=True)[1:], E4)):
        taken = isinstance(arg, MXActivation)
        x32 = arg.dequantize() if taken else arg.float()
        gates, _, offs, _, inv = mx_moe_route(x32 @ moe.router.t(), moe.top_k)
        rows = MXActivation(*mx_moe_dispatch_quantize(arg, inv, None if taken else moe.up.act_fmt), E4)
        want = mx_moe_combine(moe.down(moe.up(rows, offs), offs), inv, gates)
        got = moe(arg)
        assert same_bits(got, want) and bool(got.isfinite().all())
        # and the parts on the CPU: the routing's definition, and the default block's result up to the gates' rounding
        assert all(same_bits(a, b) for a, b in zip((gates, offs, inv), [_route_def((x32 @ moe.router.t()).cpu(), moe.top_k)[i] for i in (0, 2, 4)]))
        torch.testing.assert_close(got, blocks("torch")[which](arg), rtol=1e-5, atol=1e-5)
    assert list(moe.state_dict()) == list(blocks("torch")[which].state_dict())


@pytest.mark.parametrize("which", (0, 1))
def test_torch_routing_is_the_default_and_unchanged(which):
    moe, x = blocks("torch")[which], blocks("torch")[2]
    E, k = moe.num_experts, moe.top_k
    top, experts = torch.topk(x @ moe.router.t(), k, -1)
    ids = experts.reshape(-1)
    order = torch.argsort(ids, stable=True)
    offs = (ids.unsqueeze(1) == torch.arange(E, device=DEV)).sum(0).cumsum(0).to(torch.int32)
    y = moe.down(moe.up(x[torch.div(order, k, rounding_mode="floor")], offs), offs)
    want = (y[torch.argsort(order)].reshape(-1, k, moe.embed_dim) * torch.softmax(top, -1).unsqueeze(-1)).sum(1)
    assert moe.routing == "torch" and same_bits(moe(x), want)
    assert same_bits(type(moe)(moe.router, moe.up, moe.down, k)(x), want)


def test_fused_block_replays_in_a_graph_with_other_boundaries():
    moe, _, x = blocks("fused")
    static = x.clone()
    moe(static)                                                 # (warm-up: the workspace and outputs come from the caching allocator)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = moe(static)
    for seed in (11, 12, 13):
        new = drawn(seed, *x.shape).to(DEV) * (seed - 10)
        static.copy_(new)
        graph.replay()
        assert same_bits(out, moe(new))
