"""``mx_flash_prefill`` / ``mx_flash_prefill_paged`` on the GPU: the one launch against its definition on the same device, against the
decode launch, and against the streamed launch on the repeated, sliced cache.  Pools are carved as in ``test_mx_paged_gpu.py``: two 0xFF
guard pages, only -1 and P as dead entries, so a missing guard shows as a NaN or a changed guard page, never as a fault."""
import pytest
import torch

import test_mx_flash_decode as TD
from qsparse_amd import MXPagedKVCache, _hip, mx_flash_prefill, mx_flash_prefill_paged, mx_rope_table
from qsparse_amd.mx_flash import _decode_def, _decode_paged_def
from qsparse_amd.mx_kv_cache import _append_paged_def
from qsparse_amd.quantize import mx_dequantize
from test_mx_flash_gpu import DEV, DIMS, DTYPES, E4, F62, TRIPLES, same_bytes
from test_mx_paged import gather, pool_of
from test_mx_paged_gpu import table_of
from test_mx_prefill import parents_route

pytestmark = pytest.mark.gpu
B, HKV = 2, 2
SHAPES = ((1, 1, 32, 1), (4, 16, 32, 5), (5, 13, 32, 5), (3, 50, 64, 5), (8, 33, 128, 3), (1, 130, 32, 9), (16, 9, 256, 2))   # (r, T, page, NP)


def flat(ops, trip, kv_len, *, scale=0.21, is_causal=False, out_dtype=torch.float32):
    """(the contiguous launch, the definition on the device)"""
    got = mx_flash_prefill(*ops[:2], trip[0], *ops[2:], trip[2], kv_len, scale=scale, is_causal=is_causal, p_fmt=trip[1], out_dtype=out_dtype)
    return got, _decode_def(*ops[:2], trip[0], *ops[2:], trip[2], kv_len, scale, is_causal, trip[1], out_dtype, 1)


def paged(q, pools, trip, table, kv_len, *, scale=0.21, is_causal=False, out_dtype=torch.float32):
    """(the paged launch, the definition on the device)"""
    got = mx_flash_prefill_paged(*q, trip[0], *pools[:2], *pools[2:], trip[2], table, kv_len, scale=scale, is_causal=is_causal, p_fmt=trip[1],
                                 out_dtype=out_dtype)
    return got, _decode_paged_def(*q, trip[0], *pools[:2], *pools[2:], trip[2], table, kv_len, scale, is_causal, trip[1], out_dtype, 1)


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("n,shape", enumerate(SHAPES), ids=lambda v: str(v))
def test_launches_equal_the_definition_each_other_and_the_decode_launch(n, shape, causal):
    (r, T, page, NP), (d, dv), trip, dtype = shape, DIMS[n % 4], TRIPLES[n % 5], DTYPES[n % 3]
    S, kw = NP * page, dict(is_causal=causal, out_dtype=dtype)
    ops = TD.operands(n, B, HKV, r, T, S, d, dv, trip[0], trip[2], DEV)
    table = table_of(n, B, NP, B * NP + 3)
    pools = pool_of(ops[2:], page, B * NP + 3, table, guard=True)
    kv_len = torch.tensor([S, S - 5], dtype=torch.int32, device=DEV)
    got, want = flat(ops, trip, kv_len, **kw)
    assert same_bytes(got, want), (shape, trip, dtype)
    nan = (torch.arange(T, device=DEV) < T - kv_len[:, None])[:, None, :, None].expand_as(want) if causal else torch.zeros_like(want).bool()
    assert torch.equal(want.isnan(), nan) and bool((want.float().nan_to_num() != 0).any())
    gotp, wantp = paged(ops[:2], pools, trip, table, kv_len, **kw)
    assert same_bytes(gotp, wantp), "the paged launch and its definition"
    assert same_bytes(gotp, flat(ops[:2] + gather(pools, table), trip, kv_len, **kw)[0]), "the paged launch and the contiguous one, gathered"
    if r * T <= 64:
        assert same_bytes(got, TD.decode(ops, trip[0], trip[2], kv_len, scale=0.21, p_fmt=trip[1], kv_splits=1, **kw))


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("page", (32, 128))
def test_lengths_hide_poison_and_dead_entries(page, causal):
    NP, T = 4, 40
    S, P = NP * page, 8 * NP + 2
    lens = (0, 1, 31, page - 1, page, page + 1, S - 1, S)
    ops = TD.operands(40, len(lens), HKV, 2, T, S, 64, 48, E4, E4, DEV)
    table, kv_len = table_of(41, len(lens), NP, P, shared=False), torch.tensor(lens, dtype=torch.int32, device=DEV)
    want = flat(ops, TRIPLES[0], kv_len, is_causal=causal)[1]
    nan = torch.arange(T, device=DEV) < (T - kv_len if causal else T * (kv_len == 0))[:, None]          # rows with L - T + t < 0
    assert torch.equal(want.isnan(), nan[:, None, :, None].expand_as(want))
    cache = [t.clone() for t in ops[2:]]
    for b, L in enumerate(lens):                                 # 0xFF behind every L; entries at or behind ceil(L / page) are -1 or P
        cache[0][b, :, L:], cache[1][b, :, L:], cache[2][b, :, :, L:], cache[3][b, :, :, -(-L // 32):] = 0xFF, 0xFF, 0xFF, 0xFF
        table[b, -(-L // page):] = (-1, P)[b % 2]
    assert same_bytes(flat(ops[:2] + tuple(cache), TRIPLES[0], kv_len, is_causal=causal)[0], want)
    got, again = paged(ops[:2], pool_of(cache, page, P, table, guard=True), TRIPLES[0], table, kv_len, is_causal=causal)
    assert same_bytes(got, want) and same_bytes(again, want)


def test_a_nan_scale_byte_in_chunk_2_leaves_the_rows_that_end_before_it():
    T, S, page = 40, 512, 128
    ops = list(TD.operands(48, B, HKV, 2, T, S, 64, 48, E4, E4, DEV))
    ops[5] = ops[5].clone()
    ops[5][..., 8] = 0xFF                                        # the vt scale block of the keys 256 .. 287
    kv_len, table = torch.tensor([280, 280], dtype=torch.int32, device=DEV), table_of(49, B, 4, 11, shared=False)
    got, want = flat(tuple(ops), TRIPLES[0], kv_len, is_causal=True)
    gotp = paged(ops[:2], pool_of(ops[2:], page, 11, table, guard=True), TRIPLES[0], table, kv_len, is_causal=True)[0]
    assert same_bytes(got, want) and same_bytes(gotp, want)
    assert bool(got[:, :, :16].isfinite().all()) and bool(got[:, :, 16:].isnan().all())         # lim = 241 + t <= 256 for t <= 15


@pytest.mark.parametrize("page", (32, 128))
def test_an_out_of_range_live_entry_reads_as_zero_codes(page):
    NP, P = 4, 11
    ops = TD.operands(42, B, HKV, 4, 20, NP * page, 64, 64, E4, E4, DEV)
    table = table_of(43, B, NP, P)
    table[0, 1], table[1, 2] = -1, P
    kv_len = torch.tensor([NP * page, NP * page - 40], dtype=torch.int32, device=DEV)
    pools = pool_of(ops[2:], page, P, table, guard=True)
    got, want = paged(ops[:2], pools, TRIPLES[0], table, kv_len)
    assert same_bytes(got, want) and bool(got.isfinite().all())
    for t in pools:                                              # other bytes in both guard pages: the same output
        t._base[0], t._base[P + 1] = 0x3C, 0x3C
    assert same_bytes(paged(ops[:2], pools, TRIPLES[0], table, kv_len)[0], want)


@pytest.mark.parametrize("which", ("k_pool", "vt_pool", "d40"))
def test_the_plain_route_gives_the_same_bytes(which):
    page, NP, P, d = 64, 3, 8, 40 if which == "d40" else 64
    ops = TD.operands(44, B, HKV, 4, 20, NP * page, d, 32, E4, E4, DEV)
    table, kv_len = table_of(45, B, NP, P), torch.tensor([NP * page, 77], dtype=torch.int32, device=DEV)
    pools = list(pool_of(ops[2:], page, P, table, guard=True))
    got, want = paged(ops[:2], pools, TRIPLES[0], table, kv_len, is_causal=True)
    route = _hip.mx_flash_last_route
    assert same_bytes(got, want) and same_bytes(flat(ops[:2] + gather(pools, table), TRIPLES[0], kv_len, is_causal=True)[0], want)
    assert route == _hip.mx_flash_last_route == (_hip.MX_FLASH_ROUTE_PLAIN if which == "d40" else _hip.MX_FLASH_ROUTE_VEC)
    if which == "d40":
        return
    i = 0 if which == "k_pool" else 2                            # the same pool one byte off a 16-byte base, inside its own guard pages
    big = torch.full((pools[i]._base.numel() + 1,), 0xFF, dtype=torch.uint8, device=DEV)
    pools[i] = big[1:].view(pools[i]._base.shape)[1:P + 1].copy_(pools[i])
    assert pools[i].data_ptr() % 16 != 0
    assert same_bytes(paged(ops[:2], pools, TRIPLES[0], table, kv_len, is_causal=True)[0], want)
    assert _hip.mx_flash_last_route == _hip.MX_FLASH_ROUTE_PLAIN


@pytest.fixture(scope="module")
def chunk():
    """r = 4, T = 70 behind prefixes: R = 280, S = 300, lens (300, 131), per format (operands, launch, parent's route on the device)"""
    lens, out = (300, 131), {}
    for fmt in (E4, F62):
        ops = TD.operands(1, 2, 2, 4, 70, 300, 64, 64, fmt, fmt, DEV)
        kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
        out[fmt] = (ops, mx_flash_prefill(*ops[:2], fmt, *ops[2:], fmt, kv_len, scale=0.125, is_causal=True, p_fmt=fmt),
                    parents_route(ops, 4, fmt, fmt, lens, True, scale=0.125, p_fmt=fmt))
    return lens, out


@pytest.mark.parametrize("fmt", (E4, F62))
def test_the_launch_is_the_parents_streamed_route_with_a_mask(chunk, fmt):
    assert same_bytes(chunk[1][fmt][1], chunk[1][fmt][2])


@pytest.mark.parametrize("fmt", (E4, F62))
def test_error_against_float64_attention_stays_within_a_tenth_of_the_parents_route(chunk, fmt):
    """float64 attention on the de-quantized operands, the bottom-right limit per sequence.  Measured on an MI355X: rms 0.0037705 for
    both routes in E4M3 and 0.0050591 in E2M3 (ratio 1.0000: the same bytes) against a reference rms of 0.136"""
    lens, (ops, got, parent) = chunk[0], chunk[1][fmt]
    rep = TD.repeated(ops, 4)
    q, k, vt = (mx_dequantize(rep[i], rep[i + 1], fmt, -1, torch.float64) for i in (0, 2, 4))
    j, t = torch.arange(300, device=DEV)[None, :], torch.arange(70, device=DEV)[:, None]
    keep = torch.stack([j <= L - 70 + t for L in lens])[:, None]
    ref = torch.softmax((q @ k.transpose(-1, -2) * 0.125).masked_fill(~keep, float("-inf")), -1) @ vt.transpose(-1, -2)
    rms = lambda y: (y.double() - ref).pow(2).mean().sqrt().item()
    print(f"{fmt}: prefill {rms(got):.6g} parent's route {rms(parent):.6g} ratio {rms(got) / rms(parent):.4f} reference rms {rms(0 * got):.4g}")
    assert rms(got) / rms(parent) <= 1.10


def test_captured_append_and_prefill_replay_while_lengths_and_table_change():
    page, T, d, NP = 32, 70, 64, 4
    cache, ref = (MXPagedKVCache(10, B, NP, HKV, page, d, d, device=DEV) for _ in range(2))
    rope = tuple(t.to(DEV) for t in mx_rope_table(NP * page, d))
    g = torch.Generator().manual_seed(9)
    new = lambda n: tuple(torch.randn(B, h, n, d, generator=g).to(DEV) for h in (HKV, HKV, 4 * HKV))
    for c in (cache, ref):
        c.block_table[:] = torch.tensor([[4, 1, 7, 9], [3, 8, 0, 5]], dtype=torch.int32)
    first = new(27)
    cache.append(*first, rope=rope), ref.append(*first, rope=rope)
    static = new(T)
    step = lambda c: c.prefill(*c.append(*static, rope=rope), scale=0.125, is_causal=True)
    bufs = lambda c: (c.kv_len, c.v_tail, c.k_pool, c.k_pool_scales, c.vt_pool, c.vt_pool_scales)
    keep = [t.clone() for t in bufs(cache)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(cache)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(cache)
    for i in range(2):
        for t, s in zip(bufs(cache), keep):                      # undo the step before: each replay appends behind the 27 tokens
            t.copy_(s)
        fresh = new(T)
        for t, s in zip(static, fresh):
            t.copy_(s)
        if i == 1:                                               # in place, between the replays: a shorter prefix, another page 2
            for c in (cache, ref):
                c.kv_len[1] = 20
                c.block_table[:, 2] = torch.tensor([2, 6], dtype=torch.int32)
        graph.replay()
        torch.cuda.synchronize()
        mine = [t.clone() for t in bufs(ref)]
        qc = _append_paged_def(*mine[2:4], E4, *mine[4:6], E4, mine[1], ref.block_table, mine[0], *fresh, rope, False)
        want = _decode_paged_def(*qc, E4, *mine[2:4], *mine[4:6], E4, ref.block_table, mine[0] + T, 0.125, True, E4, torch.float32, 1)
        assert same_bytes(out, want) and torch.equal(cache.kv_len, mine[0] + T) and same_bytes(cache.k_pool, mine[2]), i
