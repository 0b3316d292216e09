"""``mx_flash_decode`` on the GPU: the bytes of the launch(es) against ``_decode_def`` on the same device -- shapes on either side of every
row tile, chunk and split bound, valid lengths with a poisoned cache behind them, a maximum that moves across the splits, exceptional
rows, the PLAIN route, guard bytes, graph capture -- and the error against float64 attention next to the streamed route's."""
import pytest
import torch

import test_mx_flash_decode as TD
from qsparse_amd import _hip
from qsparse_amd.mx_flash import _decode_def
from test_mx_flash_gpu import DEV, DIMS, DTYPES, E4, F62, FP4, TRIPLES, same_bytes

pytestmark = pytest.mark.gpu
B, HKV = 2, 2
SHAPES = ((1, 1, 1, 1), (8, 1, 129, 1), (8, 1, 129, 2), (4, 4, 513, 1), (4, 4, 513, 2), (4, 4, 513, 3), (4, 4, 513, 5), (5, 3, 257, 2),
          (8, 3, 300, 3), (16, 4, 260, 2))                                                              # (r, T, S, splits)


def both(ops, trip, kv_len=None, *, splits, scale=0.21, is_causal=False, out_dtype=torch.float32):
    """(the launch(es), the definition on the device) for the format triple `trip`"""
    got = TD.decode(ops, trip[0], trip[2], kv_len, scale=scale, is_causal=is_causal, p_fmt=trip[1], out_dtype=out_dtype, kv_splits=splits)
    return got, _decode_def(*ops[:2], trip[0], *ops[2:], trip[2], kv_len, scale, is_causal, trip[1], out_dtype, splits)


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("n,shape", enumerate(SHAPES), ids=lambda v: str(v))
def test_launches_equal_the_definition(n, shape, causal):
    (r, T, S, splits), (d, dv), trip, dtype = shape, DIMS[n % 4], TRIPLES[n % 5], DTYPES[n % 3]
    ops = TD.operands(n, B, HKV, r, T, S, d, dv, trip[0], trip[2], DEV)
    got, want = both(ops, trip, splits=splits, is_causal=causal, out_dtype=dtype)
    assert same_bytes(got, want), (shape, trip, dtype)
    assert bool((want != 0).any()) and bool(want.float().isfinite().all())


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("splits", (1, 3, 5))
def test_valid_lengths_hide_a_poisoned_cache(splits, causal):
    """mid-block, a chunk boundary, whole splits empty, L < T under causal (rows NaN); then the same with 0xFF behind every L"""
    lens = (0, 1, 31, 127, 128, 129, 500, 513)
    ops = TD.operands(30, len(lens), HKV, 4, 4, 513, 64, 48, E4, E4, DEV)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    got, want = both(ops, TRIPLES[0], kv_len, splits=splits, is_causal=causal)
    assert same_bytes(got, want)
    nan = torch.arange(4, device=DEV) < (4 - kv_len if causal else 4 * (kv_len == 0))[:, None]      # token t admits L - T + t + 1 keys
    assert torch.equal(got.isnan(), nan[:, None, :, None].expand_as(got))
    qc, qs, kc, ks, vc, vs = (t.clone() for t in ops)
    for b, L in enumerate(lens):
        kc[b, :, L:], ks[b, :, L:], vc[b, :, :, L:], vs[b, :, :, -(-L // 32):] = 0xFF, 0xFF, 0xFF, 0xFF
    assert same_bytes(both((qc, qs, kc, ks, vc, vs), TRIPLES[0], kv_len, splits=splits, is_causal=causal)[0], want)


def test_the_maximum_moves_across_splits():
    """S = 640 in 5 splits of one chunk.  One key of a (sequence, kv head) takes the codes of its first query head with the scale byte
    raised, so that head's maximum lies there: (0, 0) nothing changed; (0, 1) key 7, split 0; (1, 1) key 300, split 2, both some 12
    above the rest; (1, 0) key 639, the last split, 2048 above: every other weight underflows to 0 and the row is v's column 639"""
    ops = qc, qs, kc, ks, vc, vs = TD.operands(31, B, HKV, 4, 1, 640, 64, 64, E4, E4, DEV)
    for (b, hk), key, up in (((0, 1), 7, 1), ((1, 0), 639, 8), ((1, 1), 300, 1)):
        kc[b, hk, key], ks[b, hk, key] = qc[b, 4 * hk, 0], qs[b, 4 * hk, 0] + up
    got, want = both(ops, TRIPLES[0], splits=5, scale=0.125)
    assert same_bytes(got, want) and bool(got.isfinite().all())
    assert torch.equal(got[1, 0, 0], TD.mx_dequantize(vc, vs, E4, -1)[1, 0, :, 639]), "alpha underflows: only the last key is left"


@pytest.mark.parametrize("what", ("q_scale_nan", "vt_scale_nan"))
def test_exceptional_rows_beside_ordinary_ones(what):
    qc, qs, kc, ks, vc, vs = TD.operands(32, B, HKV, 4, 2, 384, 48, 40, E4, E4, DEV)
    clean, _ = both((qc, qs, kc, ks, vc, vs), TRIPLES[0], splits=3)
    nan = torch.zeros(B, 4 * HKV, 2, 40, dtype=torch.bool, device=DEV)
    if what == "q_scale_nan":
        qs[1, 5, 1, 0], nan[1, 5, 1] = 0xFF, True
    else:                    # block 5 of vt's row 3 = keys 160 .. 191 = chunk 1 = split 1 of 3: that column of every row of the kv head
        vs[1, 1, 3, 5], nan[1, 4:, :, 3] = 0xFF, True
    got, want = both((qc, qs, kc, ks, vc, vs), TRIPLES[0], splits=3)
    assert same_bytes(got, want) and torch.equal(got.isnan(), nan)
    assert same_bytes(got[~nan], clean[~nan]), "an exceptional row changed its neighbours"


@pytest.mark.parametrize("which", (0, 2, 4), ids=("q", "k", "vt"))
def test_a_misaligned_base_takes_the_plain_route(which):
    ops = list(TD.operands(33, B, HKV, 4, 2, 192, 64, 32, E4, E4, DEV))
    kv_len = torch.tensor([192, 77], dtype=torch.int32, device=DEV)
    want = TD.decode(ops, E4, E4, kv_len, scale=0.21, kv_splits=2)
    assert _hip.mx_flash_last_route == _hip.MX_FLASH_ROUTE_VEC
    t = ops[which]           # the same values one element off a 16-byte base
    ops[which] = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)[1:].view(t.shape).copy_(t)
    assert ops[which].data_ptr() % 16 != 0
    got = TD.decode(ops, E4, E4, kv_len, scale=0.21, kv_splits=2)
    assert _hip.mx_flash_last_route == _hip.MX_FLASH_ROUTE_PLAIN and same_bytes(got, want)


@pytest.mark.parametrize("splits", (1, 2))
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_nothing_outside_the_output_is_written(dtype, splits):
    r, T, S, dv = 5, 3, 197, 33
    ops = TD.operands(34, B, HKV, r, T, S, 32, dv, E4, FP4, DEV)
    want = both(ops, (E4, E4, FP4), splits=splits, out_dtype=dtype)[1]
    n, pad = want.numel(), 256
    flat = torch.full((n + 2 * pad,), -123.0, dtype=dtype, device=DEV)
    got = _hip.mx_flash_decode(*ops[:2], E4, *ops[2:], FP4, None, 0.21, False, E4, dtype, splits, out=flat[pad:pad + n])
    assert same_bytes(got, want)
    assert bool((flat[:pad] == -123.0).all()) and bool((flat[pad + n:] == -123.0).all())


def test_captured_call_replays_with_kv_len_updated_in_place():
    first, second = TD.operands(35, B, HKV, 4, 2, 300, 64, 64, E4, E4, DEV), TD.operands(36, B, HKV, 4, 2, 300, 64, 64, E4, E4, DEV)
    static, kv_len = tuple(t.clone() for t in first), torch.tensor([300, 140], dtype=torch.int32, device=DEV)
    run = lambda: TD.decode(static, E4, E4, kv_len, scale=0.21, is_causal=True, kv_splits=3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for ops, lens in ((first, (300, 141)), (second, (17, 257))):
        for t, s in zip(static, ops):
            t.copy_(s)
        kv_len.copy_(torch.tensor(lens, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bytes(out, both(ops, TRIPLES[0], kv_len, splits=3, is_causal=True)[1])


@pytest.mark.parametrize("splits", (1, 5))
@pytest.mark.parametrize("fmt", (E4, F62))
def test_error_against_float64_attention_stays_within_a_tenth_of_the_streamed_routes(fmt, splits):
    assert TD.rms_ratio(TD.operands(5, 2, 2, 4, 1, 640, 64, 64, fmt, fmt, DEV), 4, fmt, splits) <= 1.10
