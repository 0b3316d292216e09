"""``mx_flash_prefill_ragged(_paged)`` and ``mx_kv_append_ragged_paged`` on the CPU: both definitions against the per-sequence public
calls they are built from, the cache methods, the refusals and the empty cases."""
import pytest
import torch

import test_mx_flash_decode as TD
from qsparse_amd import (MXPagedKVCache, mx_flash_prefill, mx_flash_prefill_paged, mx_flash_prefill_ragged, mx_flash_prefill_ragged_paged,
                         mx_kv_append_paged, mx_kv_append_ragged_paged, mx_rope_table)
from test_mx_paged import pool_of

E4, FP4 = TD.E4, TD.FP4
I32 = dict(dtype=torch.int32)


def flatten(t, Ts, fill, pad=3):
    """per-sequence ``t [B, H, >= max(Ts), x]`` to token-major ``[sum(Ts) + pad, H, x]``, the padding tokens holding ``fill``"""
    rows = [t[b, :, :T].permute(1, 0, 2) for b, T in enumerate(Ts)] + [torch.full((pad,) + (t.shape[1], t.shape[3]), fill, dtype=t.dtype,
                                                                                  device=t.device)]
    return torch.cat(rows).contiguous()


def cu_of(Ts, device="cpu"):
    return torch.tensor([0] + list(Ts), device=device).cumsum(0).to(torch.int32)


@pytest.mark.parametrize("causal", (False, True))
def test_attention_is_the_per_sequence_call_on_either_cache(causal):
    Ts, r, page, NP = (1, 0, 17, 5), 4, 32, 3
    ops = TD.operands(7, len(Ts), 2, r, max(Ts), NP * page, 40, 24, FP4, E4)
    table = torch.tensor([[7, 2, 5], [0, 8, 3], [1, 9, 4], [6, 10, 11]], **I32)
    pools, kv_len, cu = pool_of(ops[2:], page, 12, table), torch.tensor([60, 9, 16, NP * page], **I32), cu_of(Ts)
    q = tuple(flatten(t, Ts, 0xFF) for t in ops[:2])
    kw = dict(scale=0.3, is_causal=causal, out_dtype=torch.bfloat16)
    flat = mx_flash_prefill_ragged(*q, FP4, *ops[2:], E4, kv_len, cu, **kw)
    paged = mx_flash_prefill_ragged_paged(*q, FP4, *pools, E4, table, kv_len, cu, **kw)
    assert flat.shape == (sum(Ts) + 3, 8, 24) and bool((flat[-3:] == 0).all()) and bool((paged[-3:] == 0).all())
    for b, T in enumerate(Ts):
        if T:
            one = tuple(t[b:b + 1, :, :T] for t in ops[:2])
            rows = slice(int(cu[b]), int(cu[b + 1]))
            want = mx_flash_prefill(*one, FP4, *(t[b:b + 1] for t in ops[2:]), E4, kv_len[b:b + 1], **kw)[0].permute(1, 0, 2)
            assert torch.equal(flat[rows].view(torch.int16), want.view(torch.int16)), b
            want = mx_flash_prefill_paged(*one, FP4, *pools, E4, table[b:b + 1], kv_len[b:b + 1], **kw)[0].permute(1, 0, 2)
            assert torch.equal(paged[rows].view(torch.int16), want.view(torch.int16)), b
    assert bool(flat[1].isnan().all()) == causal and bool(flat[2:-3].isfinite().all())       # L = 16 < T = 17: token 0 admits nothing


@pytest.mark.parametrize("rope", (False, True))
def test_append_is_the_per_sequence_call_and_the_cache_methods_chain(rope):
    Ts, L0, d, dv, page, NP = (1, 0, 40, 17), (31, 5, 0, 94), 32, 16, 32, 3
    g = torch.Generator().manual_seed(11)
    k, v, q = (torch.randn(len(Ts), h, max(Ts), n, generator=g).bfloat16() for h, n in ((2, d), (2, dv), (4, d)))
    tables = mx_rope_table(NP * page, d) if rope else None
    mine, ref = (MXPagedKVCache(13, len(Ts), NP, 2, page, d, dv, FP4, E4) for _ in range(2))
    for c in (mine, ref):
        c.block_table[:] = torch.randperm(13, generator=torch.Generator().manual_seed(1))[:12].to(torch.int32).view(4, 3)
        c.kv_len[:] = torch.tensor(L0, **I32)
        c.v_tail.copy_(torch.randn(c.v_tail.shape, generator=torch.Generator().manual_seed(2)))
        c.k_pool.fill_(0x11), c.vt_pool.fill_(0x11)
    cu = cu_of(Ts)
    qc = mine.append_ragged(*(flatten(t, Ts, float("nan")) for t in (k, v)), cu, q=flatten(q, Ts, float("nan")), rope=tables)
    assert bool((qc[0][-3:] == 0).all()) and torch.equal(mine.kv_len, torch.tensor([32, 5, 40, 111], **I32))    # (> S = 96: clamped where read)
    bufs = lambda c: (c.k_pool, c.k_pool_scales, c.vt_pool, c.vt_pool_scales, c.v_tail)
    for b, T in enumerate(Ts):
        if T:
            one = mx_kv_append_paged(*bufs(ref)[:2], FP4, *bufs(ref)[2:4], E4, ref.v_tail[b:b + 1], ref.block_table[b:b + 1], ref.kv_len[b:b + 1],
                                     k[b:b + 1, :, :T], v[b:b + 1, :, :T], q_new=q[b:b + 1, :, :T], rope=tables)
            assert all(torch.equal(a[int(cu[b]):int(cu[b + 1])], w[0].permute(1, 0, 2)) for a, w in zip(qc, one)), b
    assert all(torch.equal(a, w) for a, w in zip(bufs(mine), bufs(ref)))
    y = mine.prefill_ragged(*qc, cu, scale=0.2, is_causal=True)
    want = mx_flash_prefill_ragged_paged(*qc, FP4, *bufs(mine)[:4], E4, mine.block_table, mine.kv_len, cu, scale=0.2, is_causal=True)
    assert torch.equal(y.nan_to_num(7.0), want.nan_to_num(7.0)) and bool(y[:1].isfinite().all()) and bool(y[1:41].isfinite().all())


def test_refusals():
    Ts = (3, 2)
    ops = TD.operands(4, 2, 2, 2, 3, 64, 32, 16)
    q, cu, kv_len = tuple(flatten(t, Ts, 0) for t in ops[:2]), cu_of(Ts), torch.tensor([9, 9], **I32)
    call = lambda q=q, cache=ops[2:], cu=cu, kv_len=kv_len: mx_flash_prefill_ragged(*q, E4, *cache, E4, kv_len, cu, scale=1.0)
    assert call().shape == (8, 4, 16)
    for bad in (cu.long(), cu[:2], cu.tolist(), cu[None]):
        with pytest.raises(ValueError, match=r"cu_seqlens must be an int32 tensor of shape \(3,\)"):
            call(cu=bad)
    with pytest.raises(ValueError, match="kv_len must be an int32 tensor"):
        call(kv_len=None)
    with pytest.raises(ValueError, match="exactly 3 dimensions"):
        call(q=ops[:2])
    with pytest.raises(ValueError, match="multiple of Hkv"):
        call(cache=TD.operands(4, 2, 3, 1, 1, 64, 32, 16)[2:])
    with pytest.raises(ValueError, match="<= 128, got d = 160"):
        call(q=tuple(t[0].permute(1, 0, 2) for t in TD.operands(4, 2, 1, 1, 1, 64, 160, 16)[:2]), cache=TD.operands(4, 2, 1, 1, 1, 64, 160, 16)[2:])
    with pytest.raises(ValueError, match="<= 128, got dv = 160"):
        call(cache=TD.operands(4, 2, 2, 1, 1, 64, 32, 160)[2:])
    cache = MXPagedKVCache(4, 2, 2, 2, 32, 32, 16)
    k, v = torch.zeros(8, 2, 32), torch.zeros(8, 2, 16)
    with pytest.raises(ValueError, match="with k_new's Ttot"):
        cache.append_ragged(k, v[:7], cu)
    with pytest.raises(ValueError, match="with k_new's Ttot"):
        cache.append_ragged(k, v, cu, q=torch.zeros(7, 4, 32))
    with pytest.raises(ValueError, match="cu_seqlens must be an int32 tensor"):
        cache.append_ragged(k, v, cu.to(torch.int64))
    with pytest.raises(ValueError, match="<= 128, got d = 160"):
        MXPagedKVCache(4, 2, 2, 2, 32, 160, 16).append_ragged(torch.zeros(8, 2, 160), v, cu)
    with pytest.raises(ValueError, match="cu_seqlens must be an int32 tensor"):
        call(cu=cu.to("meta"))


def test_empty_batches_and_empty_token_axes():
    for B, Ttot in ((0, 5), (2, 0)):
        cache = MXPagedKVCache(4, B, 2, 2, 32, 32, 16)
        cu = torch.zeros(B + 1, **I32)
        qc = cache.append_ragged(torch.ones(Ttot, 2, 32), torch.ones(Ttot, 2, 16), cu, q=torch.ones(Ttot, 4, 32))
        assert qc[0].shape == (Ttot, 4, 32) and qc[1].shape == (Ttot, 4, 1) and not bool(cache.k_pool.any()) and not bool(qc[0].any())
        y = cache.prefill_ragged(*qc, cu, scale=1.0)
        assert y.shape == (Ttot, 4, 16) and not bool(y.any())
        flat = mx_flash_prefill_ragged(*qc, E4, *(torch.zeros(s, dtype=torch.uint8) for s in ((B, 2, 64, 32), (B, 2, 64, 1), (B, 2, 16, 64), (B, 2, 16, 2))),
                                       E4, cache.kv_len, cu, scale=1.0)
        assert flat.shape == (Ttot, 4, 16) and not bool(flat.any())
