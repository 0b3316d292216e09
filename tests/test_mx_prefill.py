"""``mx_flash_prefill`` / ``mx_flash_prefill_paged`` on the CPU: the call is ``_decode_def`` at one split for any ``R = r T``, which is the
streamed call on the repeated, sliced cache with the bottom-right limit as an additive mask; the paged form; the refusals."""
import pytest
import torch

import test_mx_flash_decode as TD
from qsparse_amd import MXKVCache, MXPagedKVCache, mx_flash_attention, mx_flash_prefill, mx_flash_prefill_paged
from qsparse_amd.mx_flash import _decode_def
from test_mx_paged import GARBAGE, gather, pool_of

E4, F62, FP4 = TD.E4, TD.F62, TD.FP4


def prefill(ops, qk_fmt, v_fmt, kv_len=None, **kw):
    return mx_flash_prefill(*ops[:2], qk_fmt, *ops[2:], v_fmt, kv_len, **kw)


def parents_route(ops, r, qk_fmt, v_fmt, lens, causal, **kw):
    """what served a prefill chunk before: per sequence the cache sliced to L (read on the host) and repeated r times, the bottom-right
    limit as an additive [T, L] mask, through ``rows="streamed"``"""
    T, out = ops[0].shape[2], []
    for b, L in enumerate(lens):
        one = tuple(t[b:b + 1] for t in ops[:2]) + (ops[2][b:b + 1, :, :L], ops[3][b:b + 1, :, :L], ops[4][b:b + 1, ..., :L],
                                                   ops[5][b:b + 1, ..., :-(-L // 32)])
        j, t = torch.arange(L, device=ops[0].device)[None, :], torch.arange(T, device=ops[0].device)[:, None]
        mask = torch.zeros(T, L, device=ops[0].device).masked_fill(j > L - T + t, float("-inf")) if causal else None
        rep = TD.repeated(one, r)
        out.append(mx_flash_attention(*rep[:2], qk_fmt, *rep[2:], v_fmt, mask, rows="streamed", **kw))
    return torch.cat(out)


@pytest.mark.parametrize("fmt", (E4, F62))
def test_the_call_is_the_definition_and_the_parents_route_at_280_rows(fmt):
    ops, lens = TD.operands(1, 2, 2, 4, 70, 300, 64, 64, fmt, fmt), (300, 131)
    kv_len = torch.tensor(lens, dtype=torch.int32)
    got = prefill(ops, fmt, fmt, kv_len, scale=0.125, is_causal=True, p_fmt=fmt)
    assert got.shape == (2, 8, 70, 64) and bool(got.isfinite().all())
    assert torch.equal(got, _decode_def(*ops[:2], fmt, *ops[2:], fmt, kv_len, 0.125, True, fmt, torch.float32, 1))
    assert torch.equal(got, parents_route(ops, 4, fmt, fmt, lens, True, scale=0.125, p_fmt=fmt))
    full = prefill(ops, fmt, fmt, scale=0.125, p_fmt=fmt, out_dtype=torch.bfloat16)     # no length, no limit: the streamed call itself
    assert torch.equal(full, mx_flash_attention(*TD.repeated(ops, 4)[:2], fmt, *TD.repeated(ops, 4)[2:], fmt, scale=0.125, p_fmt=fmt,
                                                out_dtype=torch.bfloat16, rows="streamed"))


@pytest.mark.parametrize("causal", (False, True))
def test_up_to_64_rows_it_is_the_decode_call_at_one_split(causal):
    ops, kv_len = TD.operands(2, 2, 2, 4, 16, 200, 40, 24, FP4, E4), torch.tensor([200, 9], dtype=torch.int32)     # 9 < T: NaN rows
    got = prefill(ops, FP4, E4, kv_len, scale=0.3, is_causal=causal)
    assert torch.equal(got.isnan(), TD.decode(ops, FP4, E4, kv_len, scale=0.3, is_causal=causal, kv_splits=1).isnan())
    assert torch.equal(got.nan_to_num(7.0), TD.decode(ops, FP4, E4, kv_len, scale=0.3, is_causal=causal, kv_splits=1).nan_to_num(7.0))
    assert bool(got[1, :, :7].isnan().all()) == causal and bool(got[1, :, 7:].isfinite().all())


@pytest.mark.parametrize("page", (32, 128))
def test_the_paged_call_is_the_contiguous_call_on_the_gathered_cache(page):
    NP, P = 3, 9
    ops = TD.operands(page, 2, 2, 5, 13, NP * page, 40, 24, FP4, E4)
    table = torch.tensor([[7, 2, 5], [0, 8, 3]], dtype=torch.int32)
    pools, kv_len = pool_of(ops[2:], page, P, table), torch.tensor([NP * page, page + 9], dtype=torch.int32)
    dirty = table.clone()
    dirty[1, 2] = GARBAGE[page // 32 % 2]                        # page 2 of sequence 1 starts behind its length
    got = mx_flash_prefill_paged(*ops[:2], FP4, *pools[:2], *pools[2:], E4, dirty, kv_len, scale=0.3, is_causal=True)
    assert torch.equal(got, prefill(ops[:2] + gather(pools, table), FP4, E4, kv_len, scale=0.3, is_causal=True)) and bool(got.isfinite().all())


def test_refusals():
    ok = TD.operands(4, 2, 2, 2, 70, 40, 32, 16)
    call = lambda ops, kv_len=None: prefill(ops, E4, E4, kv_len, scale=1.0)
    assert call(ok).shape == (2, 4, 70, 16)                      # R = 140: no bound
    with pytest.raises(ValueError, match="multiple of Hkv"):
        call(ok[:2] + TD.operands(4, 2, 3, 1, 1, 40, 32, 16)[2:])
    with pytest.raises(ValueError, match="<= 128, got d = 160"):
        call(TD.operands(4, 1, 1, 1, 1, 40, 160, 16))
    with pytest.raises(ValueError, match="<= 128, got dv = 160"):
        call(TD.operands(4, 1, 1, 1, 1, 40, 32, 160))
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), [40, 40]):
        with pytest.raises(ValueError, match="kv_len must be an int32 tensor"):
            call(ok, bad)
    table, kv_len = torch.zeros(2, 1, dtype=torch.int32), torch.full((2,), 9, dtype=torch.int32)
    pools = pool_of(TD.operands(4, 2, 2, 1, 1, 32, 32, 16)[2:], 32, 4, table)
    paged = lambda p, kl=kv_len: mx_flash_prefill_paged(*ok[:2], E4, *p[:2], *p[2:], E4, table, kl, scale=1.0)
    assert paged(pools).shape == (2, 4, 70, 16)
    with pytest.raises(ValueError, match="k_pool must be contiguous"):
        paged((pools[0].transpose(0, 1).contiguous().transpose(0, 1),) + pools[1:])
    with pytest.raises(ValueError, match="kv_len must be an int32 tensor"):
        paged(pools, None)


def test_the_caches_prefill_behind_their_append():
    g = torch.Generator().manual_seed(3)
    k, v, q = (torch.randn(2, h, 70, 32, generator=g) for h in (2, 2, 8))
    flat, paged = MXKVCache(2, 2, 96, 32, 32), MXPagedKVCache(7, 2, 3, 2, 32, 32, 32)
    paged.block_table[:] = torch.tensor([[4, 0, 6], [2, 5, 1]], dtype=torch.int32)
    qc = [c.append(k, v, q) for c in (flat, paged)]
    ys = [c.prefill(*codes, scale=0.2, is_causal=True) for c, codes in zip((flat, paged), qc)]
    assert torch.equal(ys[0], ys[1]) and ys[0].shape == (2, 8, 70, 32) and bool(ys[0].isfinite().all())
    assert torch.equal(ys[0], _decode_def(*qc[0], E4, flat.k_codes, flat.k_scales, flat.vt_codes, flat.vt_scales, E4, flat.kv_len, 0.2,
                                          True, E4, torch.float32, 1))
