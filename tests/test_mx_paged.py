"""The paged MX KV cache on the CPU: ``_decode_paged_def`` / ``_append_paged_def`` against the contiguous definitions on an explicitly
gathered cache -- permuted tables, garbage in dead entries, 0xFF in unreferenced pages, out-of-range live entries -- and the refusals."""
import pytest
import torch

import test_mx_flash_decode as TD
from qsparse_amd import MXPagedKVCache, mx_flash_decode_paged, mx_kv_append_paged, mx_rope_table
from qsparse_amd.mx_flash import _decode_def
from qsparse_amd.mx_kv_cache import _append_def

E4, FP4 = TD.E4, TD.FP4
GARBAGE = (-2 ** 31, 2 ** 31 - 1)


def pool_of(cache, page, P, table, guard=False):
    """the four pool tensors [P, Hkv, ...] that hold the contiguous `cache` (k, ks, vt, vts with S = NP page) where `table` [B, NP] says;
    entries outside [0, P) are skipped, pages nobody names hold 0xFF.  `guard`: each pool is big[1:P + 1] of an 0xFF allocation"""
    (B, NP), out, entries = table.shape, [], table.tolist()
    for i, t in enumerate(cache):
        t = t.unflatten(2 if i < 2 else 3, (NP, -1))
        pages = t.permute(0, 2, 1, 3, 4) if i < 2 else t.permute(0, 3, 1, 2, 4)         # [B, NP, Hkv, ...]
        big = torch.full((P + 2,) + tuple(pages.shape[2:]), 0xFF, dtype=torch.uint8, device=t.device)
        pool = big[1:P + 1] if guard else big[1:P + 1].clone()
        for b, n in ((b, n) for b in range(B) for n in range(NP) if 0 <= entries[b][n] < P):
            pool[entries[b][n]] = pages[b, n]
        out.append(pool)
    return tuple(out)


def gather(pools, table):
    """the contiguous cache the (valid) entries of `table` name, by index_select and permute"""
    pages = [t.index_select(0, table.reshape(-1).long()).unflatten(0, tuple(table.shape)) for t in pools]
    return tuple(t.permute(0, 2, 1, 3, 4).flatten(2, 3) for t in pages[:2]) + tuple(t.permute(0, 2, 3, 1, 4).flatten(3, 4) for t in pages[2:])


@pytest.mark.parametrize("page", (32, 64, 128, 256))
def test_decode_is_the_contiguous_definition_on_the_gathered_cache(page):
    NP, P = 3, 9
    ops = TD.operands(page, 2, 2, 3, 2, NP * page, 40, 24, FP4, E4)
    table = torch.tensor([[7, 2, 5], [0, 8, 3]], dtype=torch.int32)
    pools = pool_of(ops[2:], page, P, table)
    kv_len = torch.tensor([NP * page, page + 9], dtype=torch.int32)
    dirty = table.clone()
    dirty[1, 2] = GARBAGE[page // 32 % 2]                        # page 2 of sequence 1 starts behind its length
    for causal, splits in ((False, 1), (True, 2)):
        got = mx_flash_decode_paged(*ops[:2], FP4, *pools[:2], *pools[2:], E4, dirty, kv_len, scale=0.3, is_causal=causal, kv_splits=splits)
        want = _decode_def(*ops[:2], FP4, *gather(pools, table)[:2], *gather(pools, table)[2:], E4, kv_len, 0.3, causal, E4, torch.float32, splits)
        assert torch.equal(got, want) and bool(got.isfinite().all())
    dirty[0, 1] = -1                                             # a live entry out of range: zero codes under the byte 127
    k, ks, vt, vts = (t.clone() for t in gather(pools, table))
    k[0, :, page:2 * page], vt[0, :, :, page:2 * page], ks[0, :, page:2 * page], vts[0, :, :, page // 32:2 * page // 32] = 0, 0, 127, 127
    got = mx_flash_decode_paged(*ops[:2], FP4, *pools[:2], *pools[2:], E4, dirty, kv_len, scale=0.3, kv_splits=2)
    assert torch.equal(got, _decode_def(*ops[:2], FP4, k, ks, vt, vts, E4, kv_len, 0.3, False, E4, torch.float32, 2))


@pytest.mark.parametrize("page", (32, 64))
def test_append_is_the_contiguous_definition_on_the_gathered_cache(page):
    lens, NP, T, Hkv, d, dv = (0, 31, page - 1, page, page + 1), 3, 37, 2, 32, 24
    B, P = len(lens), 20
    table = torch.randperm(P, generator=torch.Generator().manual_seed(page))[:B * NP].to(torch.int32).view(B, NP)
    table[3, 1] = P                                              # sequence 3 (L = page) writes its first 32 tokens nowhere
    g = torch.Generator().manual_seed(7)
    pools = pool_of(TD.operands(8, B, Hkv, 1, 1, NP * page, d, dv)[2:], page, P, table)
    kv_len, v_tail = torch.tensor(lens, dtype=torch.int32), torch.randn(B, Hkv, dv, 32, generator=g)
    k, v, q = (torch.randn(B, h, T, n, generator=g) for h, n in ((Hkv, d), (Hkv, dv), (2 * Hkv, d)))
    rope = mx_rope_table(NP * page, d)
    # the contiguous definition on the gathered cache (the dead entry reads some page: its positions are written from new values alone)
    want = tuple(t.clone() for t in gather(pools, table.clamp(max=P - 1))) + (v_tail.clone(),)
    want_q = _append_def(*want[:2], E4, *want[2:4], FP4, want[4], kv_len, k, v, q, rope, True)
    got_q = mx_kv_append_paged(*pools[:2], E4, *pools[2:], FP4, v_tail, table, kv_len, k, v, q_new=q, rope=rope, interleaved=True)
    assert all(torch.equal(a, b) for a, b in zip(got_q, want_q)) and torch.equal(v_tail, want[4])
    # scattered again, it is the whole pool: unreferenced pages still 0xFF, untouched pages as before, nothing stored for the dead entry
    assert all(torch.equal(a, b) for a, b in zip(pools, pool_of(want[:4], page, P, table)))


@pytest.mark.parametrize("what,match", (("page48", "power of two"), ("page16", "power of two"), ("vt_page", "disagree on P, Hkv or page"),
                                        ("table_dtype", "block_table must be an int32"), ("table_shape", "block_table must be an int32"),
                                        ("vts", "vt_pool_scales has shape"), ("kv_len", "kv_len must be an int32")))
def test_refusals(what, match):
    page = {"page48": 48, "page16": 16}.get(what, 32)
    c = MXPagedKVCache(4, 2, 2, 2, 32, 32, 16) if page == 32 else None
    if c is None:
        with pytest.raises(ValueError, match=match):
            MXPagedKVCache(4, 2, 2, 2, page, 32, 16)
        z = lambda *s: torch.zeros(s, dtype=torch.uint8)
        pools = (z(4, 2, page, 32), z(4, 2, page, 1), z(4, 2, 16, page), z(4, 2, 16, -(-page // 32)))
    else:
        pools = [c.k_pool, c.k_pool_scales, c.vt_pool, c.vt_pool_scales]
    table, kv_len = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    if what == "vt_page":
        pools[2], pools[3] = pools[2].repeat(1, 1, 1, 2), pools[3].repeat(1, 1, 1, 2)
    elif what == "vts":
        pools[3] = pools[3].repeat(1, 1, 1, 2)
    elif what == "table_dtype":
        table = table.long()
    elif what == "table_shape":
        table = table[:1]
    elif what == "kv_len":
        kv_len = None
    q = TD.operands(1, 2, 2, 2, 1, 32, 32, 16)[:2]
    with pytest.raises(ValueError, match=match):
        mx_flash_decode_paged(*q, E4, *pools[:2], *pools[2:], E4, table, kv_len, scale=1.0)
    if what != "table_shape":                                    # (the append takes B from the table)
        with pytest.raises(ValueError, match=match):
            mx_kv_append_paged(*pools[:2], E4, *pools[2:], E4, torch.zeros(2, 2, 16, 32), table, kv_len, torch.zeros(2, 2, 1, 32),
                               torch.zeros(2, 2, 1, 16))
