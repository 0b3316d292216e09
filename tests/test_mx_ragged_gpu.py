"""The ragged launches on the GPU: ``mx_flash_prefill_ragged(_paged)`` and ``mx_kv_append_ragged_paged`` against their definitions and
against a loop of the per-sequence launches, at the smallest length vectors that reach every branch of the item map.  Only the rows below
``cu[B]`` are compared; the three padding tokens hold 0xFF codes (attention) or NaN (append).  Pools are carved between 0xFF guard pages
as in ``test_mx_paged_gpu.py``, so a missing guard shows as a NaN or a changed guard page, never as a fault."""
import pytest
import torch

import test_mx_flash_decode as TD
from qsparse_amd import (MXPagedKVCache, mx_flash_prefill, mx_flash_prefill_paged, mx_flash_prefill_ragged, mx_flash_prefill_ragged_paged,
                         mx_kv_append_paged, mx_kv_append_ragged_paged, mx_rope_table)
from qsparse_amd.mx_flash import _ragged_def
from qsparse_amd.mx_kv_cache import _append_ragged_paged_def
from qsparse_amd.quantize import mx_dequantize
from test_mx_flash_gpu import DEV, DIMS, DTYPES, E4, F62, TRIPLES, same_bytes
from test_mx_paged import pool_of
from test_mx_paged_gpu import table_of
from test_mx_ragged import cu_of, flatten

pytestmark = pytest.mark.gpu
HKV = 2
CASES = ((4, (1, 0, 17, 40), 32, 4),            # (r, T_b, page, NP): an empty sequence; one, two and three tiles
         (5, (13, 1, 27), 128, 1),              # r does not divide 64: a tile ends inside a token
         (16, (9, 1, 1, 5), 32, 3),
         (1, (130, 1, 64), 128, 2),             # an exact tile edge
         (1, (0, 1, 2) * 23 + (0,), 32, 2))     # B = 70: the scan's second round of 64 entries
KV_LEN = (lambda T, S: T - 1, lambda T, S: T, lambda T, S: T + 70, lambda T, S: S)


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("kv", range(4))
@pytest.mark.parametrize("n", range(len(CASES)))
def test_attention_equals_the_definition_and_the_per_sequence_launches(n, kv, causal):
    (r, Ts, page, NP), (d, dv), trip, dtype = CASES[n], DIMS[n % 4], TRIPLES[n % 5], DTYPES[n % 3]
    B, S, ntok, kw = len(Ts), NP * page, sum(Ts), dict(scale=0.21, is_causal=causal, p_fmt=trip[1], out_dtype=dtype)
    ops = TD.operands(n, B, HKV, r, max(Ts), S, d, dv, trip[0], trip[2], DEV)
    table = table_of(n, B, NP, B * NP + 3, shared=False)
    pools = pool_of(ops[2:], page, B * NP + 3, table, guard=True)
    q, cu = tuple(flatten(t, Ts, 0xFF) for t in ops[:2]), cu_of(Ts, DEV)
    kv_len = torch.tensor([KV_LEN[kv](T, S) for T in Ts], dtype=torch.int32, device=DEV)       # -1 and > S included: the kernel clamps
    got = mx_flash_prefill_ragged(*q, trip[0], *ops[2:], trip[2], kv_len, cu, **kw)
    want = _ragged_def(*q, trip[0], *ops[2:], trip[2], None, kv_len, cu, 0.21, causal, trip[1], dtype)
    assert got.shape == (ntok + 3, r * HKV, dv) and same_bytes(got[:ntok], want[:ntok]), "the launch and its definition"
    L = kv_len.clamp(0, S).repeat_interleave(torch.tensor(Ts, device=DEV))
    t, T = torch.cat([torch.arange(T) for T in Ts]).to(DEV), torch.tensor(Ts, device=DEV).repeat_interleave(torch.tensor(Ts, device=DEV))
    nan = (L - T + t < 0) if causal else (L == 0)
    assert torch.equal(want[:ntok].isnan(), nan[:, None, None].expand_as(want[:ntok])) and bool((want.float().nan_to_num() != 0).any())
    gotp = mx_flash_prefill_ragged_paged(*q, trip[0], *pools, trip[2], table, kv_len, cu, **kw)
    assert same_bytes(gotp[:ntok], got[:ntok]), "the paged launch and the contiguous one"
    one = lambda b, T: tuple(x[b:b + 1, :, :T] for x in ops[:2])
    loop = [mx_flash_prefill_paged(*one(b, T), trip[0], *pools, trip[2], table[b:b + 1], kv_len[b:b + 1], **kw)[0].permute(1, 0, 2)
            for b, T in enumerate(Ts) if T]
    assert same_bytes(gotp[:ntok], torch.cat(loop)), "the paged launch and a loop of mx_flash_prefill_paged"
    if n < 4:
        loop = [mx_flash_prefill(*one(b, T), trip[0], *(x[b:b + 1] for x in ops[2:]), trip[2], kv_len[b:b + 1], **kw)[0].permute(1, 0, 2)
                for b, T in enumerate(Ts) if T]
        assert same_bytes(got[:ntok], torch.cat(loop)), "the launch and a loop of mx_flash_prefill"


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("page", (32, 128))
def test_lengths_hide_poison_and_dead_entries_and_a_live_entry_out_of_range_reads_as_zero(page, causal):
    r, Ts, NP = 4, (1, 0, 17, 40, 3, 20), 4
    S, P, B, ntok = NP * page, 6 * NP + 2, len(Ts), sum(Ts)
    lens = (1, 0, 31, page - 1, page + 1, S)
    ops = TD.operands(40, B, HKV, r, max(Ts), S, 64, 48, E4, E4, DEV)
    q, cu = tuple(flatten(t, Ts, 0xFF) for t in ops[:2]), cu_of(Ts, DEV)
    table, kv_len = table_of(41, B, NP, P, shared=False), torch.tensor(lens, dtype=torch.int32, device=DEV)
    args = lambda cache, tab: (*q, E4, *cache, E4, tab, kv_len, cu, 0.21, causal, E4, torch.float32)
    want = _ragged_def(*args(ops[2:], None))[:ntok]
    cache = [x.clone() for x in ops[2:]]
    for b, L in enumerate(lens):                                 # 0xFF behind every L; entries at or behind ceil(L / page) are -1 or P
        cache[0][b, :, L:], cache[1][b, :, L:], cache[2][b, :, :, L:], cache[3][b, :, :, -(-L // 32):] = 0xFF, 0xFF, 0xFF, 0xFF
        table[b, -(-L // page):] = (-1, P)[b % 2]
    kw = dict(scale=0.21, is_causal=causal)
    assert same_bytes(mx_flash_prefill_ragged(*q, E4, *cache, E4, kv_len, cu, **kw)[:ntok], want)
    pools = pool_of(cache, page, P, table, guard=True)
    assert same_bytes(mx_flash_prefill_ragged_paged(*q, E4, *pools, E4, table, kv_len, cu, **kw)[:ntok], want)
    table[5, 1] = (-1, P)[causal]                                # live: keys page .. 2 page - 1 of the last sequence read as zero codes
    got = mx_flash_prefill_ragged_paged(*q, E4, *pools, E4, table, kv_len, cu, **kw)[:ntok]
    assert same_bytes(got, _ragged_def(*args(pools, table))[:ntok]) and not same_bytes(got[-20:], want[-20:]) and bool(got[-20:].isfinite().all())


START = lambda page, S: (0, 31, 32, page - 1, S - 2)


@pytest.mark.parametrize("rope", (False, True))
@pytest.mark.parametrize("n", range(len(CASES)))
def test_append_equals_the_definition_and_the_per_sequence_launches(n, rope):
    (r, Ts, page, NP), (d, dv), trip, dtype = CASES[n], DIMS[(n + 1) % 4], TRIPLES[n % 5], DTYPES[n % 3]
    B, S, ntok, P = len(Ts), NP * page, sum(Ts), len(Ts) * NP + 1
    g = torch.Generator().manual_seed(n)
    new = [torch.randn(B, h, max(Ts), x, generator=g).to(dtype) for h, x in ((HKV, d), (HKV, dv), (r * HKV, d))]
    flat, cu = [flatten(x, Ts, float("nan")).to(DEV) for x in new], cu_of(Ts)
    tables = mx_rope_table(S + 5, d) if rope else None
    ref = MXPagedKVCache(P, B, NP, HKV, page, d, dv, trip[0], trip[2])
    ref.block_table[:] = torch.randperm(P, generator=g)[:B * NP].to(torch.int32).view(B, NP)
    ref.block_table[1::2, -1] = P                                # a dead last page for every second sequence: its tokens are dropped
    ref.kv_len[:] = torch.tensor([START(page, S)[(b + n) % 5] for b in range(B)], dtype=torch.int32)
    ref.v_tail.copy_(torch.randn(ref.v_tail.shape, generator=g))
    names = ("k_pool", "k_pool_scales", "vt_pool", "vt_pool_scales", "v_tail")
    for name in names[:4]:
        getattr(ref, name).fill_(0x11)

    def carve():                                                 # the five buffers on the device, each between two 0xFF guard pages
        bigs = [torch.full((x.shape[0] + 2,) + x.shape[1:], 0xFF if x.dtype == torch.uint8 else float("nan"), dtype=x.dtype, device=DEV)
                for x in (getattr(ref, name) for name in names)]
        for big, name in zip(bigs, names):
            big[1:-1] = getattr(ref, name).to(DEV)
        return bigs, [big[1:-1] for big in bigs]
    (bigs, mine), (_, per_seq) = carve(), carve()
    table, kv_len, dev_rope = ref.block_table.to(DEV), ref.kv_len.to(DEV), None if not rope else tuple(x.to(DEV) for x in tables)
    got = mx_kv_append_ragged_paged(*mine[:2], trip[0], *mine[2:4], trip[2], mine[4], table, kv_len, *flat[:2], cu.to(DEV), q_new=flat[2],
                                    rope=dev_rope, interleaved=bool(n % 2))
    tail0 = ref.v_tail.clone()
    want = _append_ragged_paged_def(*(getattr(ref, name) for name in names[:2]), trip[0], ref.vt_pool, ref.vt_pool_scales, trip[2], ref.v_tail,
                                    ref.block_table, ref.kv_len, cu, *(x.cpu() for x in flat), tables, bool(n % 2))
    assert all(torch.equal(a[:ntok].cpu(), w[:ntok]) for a, w in zip(got, want)), "q codes"
    for a, big, name in zip(mine, bigs, names):
        assert same_bytes(a.cpu(), getattr(ref, name)), name
        guard = torch.stack((big[0], big[-1]))
        assert bool((guard == 0xFF).all() if guard.dtype == torch.uint8 else guard.isnan().all()), name
    assert all(torch.equal(ref.v_tail[b], tail0[b]) for b, T in enumerate(Ts) if not T) and not bool(mine[4].isnan().any())
    for b, T in enumerate(Ts):                                   # the parent's route: one launch per sequence, head-major
        if T:
            one = mx_kv_append_paged(*per_seq[:2], trip[0], *per_seq[2:4], trip[2], per_seq[4][b:b + 1], table[b:b + 1], kv_len[b:b + 1],
                                     *(x[b:b + 1, :, :T].to(DEV) for x in new[:2]), q_new=new[2][b:b + 1, :, :T].to(DEV), rope=dev_rope,
                                     interleaved=bool(n % 2))
            assert all(torch.equal(a[int(cu[b]):int(cu[b + 1])], w[0].permute(1, 0, 2)) for a, w in zip(got, one)), b
    assert all(same_bytes(a, w) for a, w in zip(mine, per_seq))


def test_captured_append_and_prefill_replay_while_cu_seqlens_tokens_and_a_table_row_change():
    page, d, NP, B, Ttot = 32, 64, 4, 4, 51
    cache, ref = (MXPagedKVCache(17, B, NP, HKV, page, d, d, device=DEV) for _ in range(2))
    rope = tuple(t.to(DEV) for t in mx_rope_table(NP * page, d))
    g = torch.Generator().manual_seed(9)
    new = lambda: tuple(torch.randn(Ttot, h, d, generator=g).to(DEV) for h in (HKV, HKV, 4 * HKV))
    for c in (cache, ref):
        c.block_table[:] = torch.randperm(17, generator=torch.Generator().manual_seed(3))[:16].to(torch.int32).view(B, NP)
    first, static, cu = new(), new(), cu_of((1, 0, 17, 30), DEV)
    step = lambda c, toks, cu: c.prefill_ragged(*c.append_ragged(*toks[:2], cu, q=toks[2], rope=rope), cu, scale=0.125, is_causal=True)
    for c in (cache, ref):                                       # prefixes of 27, 0, 20 and 4 tokens
        step(c, first, cu_of((27, 0, 20, 4), DEV))
    bufs = lambda c: (c.kv_len, c.v_tail, c.k_pool, c.k_pool_scales, c.vt_pool, c.vt_pool_scales)
    keep = [t.clone() for t in bufs(cache)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(cache, static, cu)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(cache, static, cu)
    for i, Ts in enumerate(((1, 0, 17, 30), (20, 5, 0, 23), (0, 48, 0, 0))):
        for c in (cache, ref):                                   # undo the step before; then, in place: lengths, tokens, one table row
            for t, s in zip(bufs(c), keep):
                t.copy_(s)
            c.block_table[i] = c.block_table[i].flip(0)
        fresh = new()
        for t, s in zip(static, fresh):
            t.copy_(s)
        cu.copy_(cu_of(Ts, DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = step(ref, fresh, cu_of(Ts, DEV))
        assert same_bytes(out[:sum(Ts)], want[:sum(Ts)]) and all(same_bytes(a, w) for a, w in zip(bufs(cache), bufs(ref))), i


@pytest.mark.parametrize("fmt", (E4, F62))
def test_error_against_float64_attention_stays_within_a_tenth_of_the_per_sequence_loop(fmt):
    """float64 softmax attention on the de-quantized operands, per sequence with the bottom-right limit; r = 4, T_b = (70, 1, 17), S = 300.
    The ratio is 1.0000 where the bytes are the same; the rms figures are recorded in DESIGN.md 3zh"""
    Ts, lens, S = (70, 1, 17), (300, 131, 200), 300
    ops = TD.operands(1, 3, 2, 4, 70, S, 64, 64, fmt, fmt, DEV)
    kv_len, kw = torch.tensor(lens, dtype=torch.int32, device=DEV), dict(scale=0.125, is_causal=True, p_fmt=fmt)
    got = mx_flash_prefill_ragged(*(flatten(t, Ts, 0xFF) for t in ops[:2]), fmt, *ops[2:], fmt, kv_len, cu_of(Ts, DEV), **kw)[:sum(Ts)]
    loop = torch.cat([mx_flash_prefill(*(x[b:b + 1, :, :T] for x in ops[:2]), fmt, *(x[b:b + 1] for x in ops[2:]), fmt, kv_len[b:b + 1],
                                       **kw)[0].permute(1, 0, 2) for b, T in enumerate(Ts)])
    rep = TD.repeated(ops, 4)
    qf, k, vt = (mx_dequantize(rep[i], rep[i + 1], fmt, -1, torch.float64) for i in (0, 2, 4))
    j, t = torch.arange(S, device=DEV)[None, :], torch.arange(70, device=DEV)[:, None]
    keep = torch.stack([j <= L - T + t for L, T in zip(lens, Ts)])[:, None]
    ref = torch.softmax((qf @ k.transpose(-1, -2) * 0.125).masked_fill(~keep, float("-inf")), -1) @ vt.transpose(-1, -2)
    ref = flatten(ref, Ts, 0.0, pad=0)
    rms = lambda y: (y.double() - ref).pow(2).mean().sqrt().item()
    print(f"{fmt}: ragged {rms(got):.6g} per-sequence loop {rms(loop):.6g} ratio {rms(got) / rms(loop):.4f} reference rms {rms(0 * got):.4g}")
    assert rms(got) / rms(loop) <= 1.10
