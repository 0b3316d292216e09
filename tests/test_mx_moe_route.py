"""The definitions of the fused MoE routing on the CPU: ``_route_def`` on hand-written logits and against torch on tie-free ones, the
gate and combine errors against float64 (at most twice the error of the torch expression they replace), ``_dispatch_def`` against
``quantize_with_mx`` of the token's row, and the argument checks."""
import pytest
import torch

from qsparse_amd import MXActivation, mx_moe_combine, mx_moe_dispatch_quantize, mx_moe_route, quantize_with_mx
from qsparse_amd.mx_moe import _combine_def, _dispatch_def, _route_def

NAN, INF = float("nan"), float("inf")


def drawn(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("row, k, experts, gates", (
    ([1.0, 3.0, 3.0, 0.5, 3.0], 3, [1, 2, 4], [1 / 3] * 3),             # ties go to the lower index
    ([-0.0, -1.0, 0.0, -0.0], 3, [0, 2, 3], [1 / 3] * 3),               # -0 and +0 are a tie
    ([2.0, NAN, 5.0], 2, [1, 2], [NAN, NAN]),                           # a NaN ranks first and gives NaN gates
    ([NAN, 1.0, NAN], 2, [0, 2], [NAN, NAN]),                           # NaNs among themselves: the lower index
    ([-INF, 0.0, -INF], 2, [1, 0], [1.0, 0.0]),                         # -inf among the kept logits: gate 0
    ([INF, 0.0], 2, [0, 1], [NAN, NAN]),                                # top_0 = +inf
    ([0.25, 7.0, -3.0], 1, [1], [1.0]),                                 # k = 1: gate exactly 1
    ([1.0, 2.0, 3.0], 3, [2, 1, 0], None)))                             # k = E
def test_route_def_on_hand_written_logits(row, k, experts, gates):
    g, e, offs, order, inv = mx_moe_route(torch.tensor([row, row]), k)
    assert e.tolist() == [experts, experts] and e.dtype == offs.dtype == order.dtype == inv.dtype == torch.int32
    if gates is not None:
        want = torch.tensor([gates, gates])
        assert torch.equal(g.isnan(), want.isnan()) and torch.allclose(g.nan_to_num(), want.nan_to_num(), rtol=0, atol=1e-7)
        assert gates[0] != 1.0 or g[0, 0].item() == 1.0
    flat = torch.tensor(experts * 2)
    assert order.tolist() == torch.argsort(flat, stable=True).tolist()
    assert order[inv.reshape(-1).long()].tolist() == list(range(2 * k))
    assert offs.tolist() == torch.bincount(flat, minlength=len(row)).cumsum(0).tolist()


@pytest.mark.parametrize("T, E, k, dtype", ((70, 5, 2, torch.float32), (33, 130, 8, torch.bfloat16), (9, 1024, 32, torch.float32),
                                            (0, 8, 2, torch.float16)))
def test_route_def_equals_torch_on_tie_free_logits_and_its_gates_are_as_exact(T, E, k, dtype):
    """The gate bound: at most twice the float32 ``torch.softmax`` error, both against float64.  It is why Z is a balanced tree: summed
    one by one, 31 float32 additions made the k = 32 case miss it (2.271e-08 against 7.857e-09)."""
    # a permutation of distinct values per row, exact in every dtype: no ties
    logits = torch.stack([torch.randperm(E, generator=torch.Generator().manual_seed(t)) for t in range(T)] or
                         [torch.zeros(E)]).to(dtype)[:T] / 8 - 3
    gates, experts, offs, order, inv = _route_def(logits, k)
    top, idx = torch.topk(logits.float(), k, -1)
    ids = idx.reshape(-1)
    assert torch.equal(experts.long(), idx) and torch.equal(order.long(), torch.argsort(ids, stable=True))
    assert torch.equal(offs, (ids.unsqueeze(1) == torch.arange(E)).sum(0).cumsum(0).to(torch.int32))
    assert torch.equal(inv.reshape(-1).long(), torch.argsort(order.long()))
    if T:
        exact = torch.softmax(top.double(), -1)
        err, err_torch = (gates - exact).abs().max().item(), (torch.softmax(top, -1) - exact).abs().max().item()
        print(f"gate error {err:.3e}, float32 torch.softmax {err_torch:.3e}")
        assert err <= 2 * err_torch          # (the 0.84-ulp written-out exponential against torch's own)


def test_route_refuses_what_lies_outside_its_range():
    for logits, k in ((torch.zeros(2, 1025), 2), (torch.zeros(2, 64), 33), (torch.zeros(2, 3), 4), (torch.zeros(2, 3, 4), 1),
                      (torch.zeros(2, 4), 0), (torch.zeros(4, 8).t(), 2)):
        with pytest.raises(ValueError):
            mx_moe_route(logits, k)


@pytest.mark.parametrize("fmt", ("mxfp8_e4m3", "mxfp4_e2m1"))
def test_dispatch_def_is_the_quantizer_of_the_tokens_row(fmt):
    T, k, D = 6, 3, 72
    x, inv = drawn(0, T, D), torch.randperm(T * k, generator=torch.Generator().manual_seed(1)).to(torch.int32).reshape(T, k)
    inv[4, 1] = T * k                                                    # out of range: nothing stored, nothing else disturbed
    codes, scales = mx_moe_dispatch_quantize(x, inv, fmt)
    assert codes.shape == (T * k, D) and scales.shape == (T * k, 3)
    for t in range(T):
        _, c, s = quantize_with_mx(x[t], fmt, -1, return_codes=True)
        for j in range(k):
            if (t, j) != (4, 1):
                assert torch.equal(codes[inv[t, j]], c) and torch.equal(scales[inv[t, j]], s)
    act = MXActivation(*quantize_with_mx(x, fmt, -1, return_codes=True)[1:], fmt)
    assert all(torch.equal(a, b) for a, b in zip(mx_moe_dispatch_quantize(act, inv), _dispatch_def(x, inv, fmt)))
    with pytest.raises(ValueError):
        mx_moe_dispatch_quantize(act, inv, "mxfp8_e5m2")


def test_combine_def_against_float64():
    T, k, D = 40, 4, 33
    y, gates = drawn(2, T * k, D), torch.softmax(drawn(3, T, k), -1)
    inv = torch.randperm(T * k, generator=torch.Generator().manual_seed(4)).to(torch.int32).reshape(T, k)
    rows = y[inv.reshape(-1).long()].reshape(T, k, D)
    exact = (rows.double() * gates.double().unsqueeze(-1)).sum(1)
    err = (_combine_def(y, inv, gates).double() - exact).abs().max().item()
    err_torch = ((rows * gates.unsqueeze(-1)).sum(1).double() - exact).abs().max().item()
    print(f"combine error {err:.3e}, (y * gates).sum(1) {err_torch:.3e}")
    assert err <= 2 * err_torch
    inv[3, 2], gates[5, 0] = -1, NAN                                     # an entry out of range counts as +0; a NaN gate is a NaN row
    out = mx_moe_combine(y, inv, gates, torch.bfloat16)
    rows[3, 2] = 0
    want = ((gates[3, 0] * rows[3, 0] + gates[3, 1] * rows[3, 1]) + gates[3, 2] * rows[3, 2]) + gates[3, 3] * rows[3, 3]
    assert out.dtype == torch.bfloat16 and torch.equal(out[3], want.bfloat16()) and bool(out[5].isnan().all())
    assert not bool(out[:5].isnan().any())
