"""``mx_flash_attention(rows="streamed")`` on the GPU: the bytes of the one launch against ``_streamed_def`` on the same device, and its
error against float64 attention next to the composition's."""
import pytest
import torch

import test_mx_flash as TF
import test_mx_flash_stream as TS
from qsparse_amd import _hip
from qsparse_amd.mx_bmm import _attention_mask
from qsparse_amd.mx_flash import _streamed_def
from test_mx_flash_gpu import DEV, DIMS, DTYPES, E4, F62, FP4, G, TRIPLES, masks, same_bytes

pytestmark = pytest.mark.gpu
SHAPES = ((1, 1), (5, 127), (17, 129), (64, 256), (65, 257), (33, 513), (130, 640), (300, 260))       # (T, S)


def both(ops, trip, mask=None, *, scale=0.21, is_causal=False, out_dtype=torch.float32):
    """(the one launch, the definition on the device) for the format triple `trip`"""
    got = TF.flash(ops, trip[0], trip[2], mask, scale=scale, is_causal=is_causal, p_fmt=trip[1], out_dtype=out_dtype, rows="streamed")
    T, S = ops[0].shape[-2], ops[2].shape[-2]
    return got, _streamed_def(*ops[:2], trip[0], *ops[2:], trip[2], _attention_mask(mask, False, T, S, ops[0].device), scale, is_causal,
                              trip[1], out_dtype)


@pytest.mark.parametrize("n,TS", enumerate(SHAPES), ids=lambda v: str(v))
def test_one_launch_equals_the_definition(n, TS):
    (T, S), (d, dv), trip, dtype = TS, DIMS[n % 4], TRIPLES[n % 5], DTYPES[n % 3]
    ops = TF.operands(n, (G,), T, S, d, dv, trip[0], trip[2], DEV)
    fmask, bmask = masks(T + S, T, S)
    for kw in ({}, {"mask": fmask}, {"mask": bmask}, {"is_causal": True}):
        got, want = both(ops, trip, out_dtype=dtype, **kw)
        assert same_bytes(got, want), (T, S, trip, dtype, sorted(kw))
    assert bool(want.float().isfinite().all()) and bool((want != 0).any())


@pytest.mark.parametrize("trip", TRIPLES, ids=lambda t: "-".join(f[2:] for f in t))
@pytest.mark.parametrize("d,dv", DIMS)
def test_formats_and_head_sizes(d, dv, trip):
    """every head size under every triple at (65, 257): two work-groups per slice, a third chunk of one key"""
    ops = TF.operands(d, (G,), 65, 257, d, dv, trip[0], trip[2], DEV)
    for kw in ({"mask": masks(3, 65, 257)[0]}, {"is_causal": True}):
        assert same_bytes(*both(ops, trip, **kw))


def test_the_running_maximum_moves():
    """row t % 5: 0 nothing added; 1 +8 in chunk 0 (alpha = 1 afterwards); 2 +8 in the last chunk (alpha small); 3 +100 there (alpha
    underflows to 0); 4 -inf over the whole of chunks 0 and 1 and admitted later (E(NaN) = 0)"""
    T, S = 70, 640
    ops = TF.operands(20, (G,), T, S, 64, 64, E4, E4, DEV)
    mask = torch.zeros(T, S, device=DEV)
    mask[1::5, 7], mask[2::5, 600], mask[3::5, 639], mask[4::5, :256] = 8.0, 8.0, 100.0, float("-inf")
    for trip in (TRIPLES[0], TRIPLES[1]):
        got, want = both(ops, trip, mask)
        assert same_bytes(got, want) and bool(got.isfinite().all())


@pytest.mark.parametrize("what", ("q_scale_nan", "masked_row", "inf_mask", "nan_scale", "vt_scale_nan_causal"))
def test_exceptional_rows_beside_ordinary_ones(what):
    T, S, row = 300, 384, 6
    qc, qs, kc, ks, vc, vs = TF.operands(7, (G,), T, S, 48, 40, E4, E4, DEV)
    mask, kw = torch.zeros(G, T, S, device=DEV), {}
    clean, _ = both((qc, qs, kc, ks, vc, vs), TRIPLES[0], mask)
    nan = torch.zeros(G, T, 40, dtype=torch.bool, device=DEV)
    nan[1, row] = True
    if what == "q_scale_nan":
        qs = qs.clone()
        qs[1, row, 0] = 0xFF
    elif what == "masked_row":
        mask[1, row] = float("-inf")
    elif what == "inf_mask":
        mask[1, row, 300] = float("inf")
    elif what == "nan_scale":
        kw["scale"], nan[:] = float("nan"), True
    else:                    # block 8 of vt's row 3 = keys 256 .. 287 = chunk 2: only the rows whose limit reaches it see the NaN
        mask, kw["is_causal"] = None, True
        clean, _ = both((qc, qs, kc, ks, vc, vs), TRIPLES[0], **kw)
        vs = vs.clone()
        vs[1, 3, 8] = 0xFF
        nan[1, row] = False
        nan[1, 256:, 3] = True
    got, want = both((qc, qs, kc, ks, vc, vs), TRIPLES[0], mask, **kw)
    assert same_bytes(got, want) and torch.equal(got.isnan(), nan)
    assert same_bytes(got[~nan], clean[~nan]), "an exceptional row changed its neighbours"


@pytest.mark.parametrize("which", ("q", "k", "vt", "mask"))
def test_a_misaligned_base_takes_the_plain_route(which):
    T, S = 20, 192
    ops = list(TF.operands(8, (G,), T, S, 64, 32, E4, E4, DEV))
    mask = masks(9, T, S)[0]
    want = TF.flash(ops, E4, E4, mask, scale=0.21, rows="streamed")
    assert _hip.mx_flash_last_route == _hip.MX_FLASH_ROUTE_VEC
    def shifted(t):          # the same values one element off a 16-byte base
        out = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)[1:].view(t.shape).copy_(t)
        assert out.data_ptr() % 16 != 0 and out.is_contiguous()
        return out
    if which == "mask":
        mask = shifted(mask)
    else:
        ops[{"q": 0, "k": 2, "vt": 4}[which]] = shifted(ops[{"q": 0, "k": 2, "vt": 4}[which]])
    got = TF.flash(ops, E4, E4, mask, scale=0.21, rows="streamed")
    assert _hip.mx_flash_last_route == _hip.MX_FLASH_ROUTE_PLAIN and same_bytes(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_nothing_outside_the_output_is_written(dtype):
    Gs, T, S, dv = 2, 65, 197, 33
    ops = TF.operands(10, (Gs,), T, S, 32, dv, E4, FP4, DEV)
    want = both(ops, (E4, E4, FP4), out_dtype=dtype)[1]
    n, pad = Gs * T * dv, 256
    flat = torch.full((n + 2 * pad,), -123.0, dtype=dtype, device=DEV)
    got = _hip.mx_flash_attention(*ops[:2], E4, *ops[2:], FP4, None, 0.21, False, E4, dtype, out=flat[pad:pad + n], streamed=True)
    assert same_bytes(got, want)
    assert bool((flat[:pad] == -123.0).all()) and bool((flat[pad + n:] == -123.0).all())


def test_captured_call_replays_bit_for_bit():
    first, second = TF.operands(12, (G,), 70, 300, 64, 64, E4, E4, DEV), TF.operands(13, (G,), 70, 300, 64, 64, E4, E4, DEV)
    want = both(second, TRIPLES[0], is_causal=True)[1]
    static = tuple(t.clone() for t in first)
    run = lambda: TF.flash(static, E4, E4, scale=0.21, is_causal=True, rows="streamed")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for t, s in zip(static, second):
        t.copy_(s)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same_bytes(out, want)


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("fmt", (E4, F62))
@pytest.mark.parametrize("T,S", ((197, 197), (40, 640)))
def test_error_against_float64_attention_stays_within_a_tenth_of_the_compositions(T, S, fmt, causal):
    """both paths round each weight once to p_fmt, the streamed one adds one float32 rounding per chunk: at most 10 % above"""
    assert TS.rms_ratio(TF.operands(14, (G,), T, S, 64, 64, fmt, fmt, DEV), fmt, causal) <= 1.10
