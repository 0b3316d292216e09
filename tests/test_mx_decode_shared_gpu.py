"""``mx_flash_decode_paged(shared=...)`` on the GPU: the launch against ``_decode_shared_def`` on the same device, byte for byte.  Every pool
is carved as big[1:P + 1] of an 0xFF allocation and only -1 and P stand for out-of-range entries, so a missing guard shows as a NaN or a
changed byte, never as a fault."""
import pytest
import torch

from qsparse_amd import mx_flash_decode_paged
from qsparse_amd.mx_flash import _decode_shared_def, _shared_chunks
from test_mx_decode_shared import shared_case, slen
from test_mx_flash_gpu import DEV, DIMS, DTYPES, TRIPLES, same_bytes

pytestmark = pytest.mark.gpu
HKV = 2
# (r, T, B, page, NP, NPs, shared_len, sp, so): two tiles with a sequence across their edge; R no divisor of 16; R = 64; R = 1 and 17
# sequences; shared_len 0, exact, rounded down (200 -> 128; 300 -> 256 at page 256), beyond NPs * page; windows of 64 pages at page 32
CASES = ((4, 1, 5, 32, 12, 8, 256, 1, 2), (1, 3, 6, 64, 6, 4, 200, 3, 1), (64, 1, 2, 128, 3, 2, 128, 1, 1), (1, 1, 17, 32, 10, 4, 128, 3, 2),
         (2, 3, 3, 128, 4, 2, 0, 1, 2), (4, 1, 5, 256, 3, 2, 300, 3, 2), (8, 1, 3, 64, 7, 3, 10 ** 6, 3, 2), (4, 3, 4, 32, 70, 68, 2176, 3, 1))


def lengths(B, Ls, S):
    """kv_len mixing S, Ls + 1, Ls, a length inside the shared part and 0"""
    return torch.tensor(([S, Ls + 1, Ls, max(Ls - 37, 1), 0] * B)[:B], dtype=torch.int32, device=DEV)


def both(q, pools, trip, table, kv_len, shared, *, sp, so, causal=False, dtype=torch.float32):
    """(the launches, the definition on the device)"""
    got = mx_flash_decode_paged(*q, trip[0], *pools, trip[2], table, kv_len, scale=0.21, is_causal=causal, p_fmt=trip[1], out_dtype=dtype,
                                kv_splits=so, shared=shared, shared_splits=sp)
    return got, _decode_shared_def(*q, trip[0], *pools, trip[2], table, kv_len, *shared, 0.21, causal, trip[1], dtype, so, sp)


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("n,case", enumerate(CASES), ids=lambda v: str(v))
def test_the_launch_equals_the_definition(n, case, causal):
    (r, T, B, page, NP, NPs, sl, sp, so), (d, dv), trip, dtype = case, DIMS[n % 4], TRIPLES[n % 5], DTYPES[n % 3]
    q, pools, table, stable, _ = shared_case(n, B, HKV, r, T, page, NP, NPs, d, dv, trip[0], trip[2], DEV, guard=True)
    kv_len = lengths(B, _shared_chunks(page, NP, NPs, sl)[0], NP * page)
    got, want = both(q, pools, trip, table, kv_len, (stable, slen(sl, DEV)), sp=sp, so=so, causal=causal, dtype=dtype)
    assert same_bytes(got, want), (case, trip, dtype)
    admits = (kv_len[:, None] - T + 1 + torch.arange(T, device=DEV) if causal else kv_len[:, None].expand(B, T)) > 0
    assert torch.equal(want.isnan(), ~admits[:, None, :, None].expand_as(want)) and bool((want[admits.any(1)].nan_to_num() != 0).any())


@pytest.mark.parametrize("page,sl", ((32, 256), (128, 300)))
def test_block_table_is_not_read_below_the_shared_length_and_guards_hold(page, sl):
    B, NP, NPs, trip = 5, 6, 4, TRIPLES[0]
    q, pools, table, stable, P = shared_case(20, B, HKV, 4, 2, page, NP, NPs, 64, 48, device=DEV, guard=True)
    Ls, S = _shared_chunks(page, NP, NPs, sl)[0], NP * page
    kv_len, shared = lengths(B, Ls, S), (stable, slen(sl, DEV))
    want = both(q, pools, trip, table, kv_len, shared, sp=2, so=2, causal=True)[1]
    dirty = table.clone()                                        # below Ls: -1, P and other sequences' pages
    dirty[:, :Ls // page] = torch.tensor([-1, P, int(table[1, -1]), int(table[0, -1])], device=DEV, dtype=torch.int32).repeat(NP)[:Ls // page]
    top = int(kv_len.max())                                      # 0xFF behind every L_b: own pages behind L_b, shared pages behind the longest
    for b, L in enumerate(kv_len.tolist()):
        for n in range(NP):
            src, lo = (stable[n], max(top, n * page)) if (n + 1) * page <= Ls else (table[b, n], max(L, n * page))
            lo = min(lo - n * page, page)
            pools[0][src, :, lo:], pools[1][src, :, lo:], pools[2][src, :, :, lo:], pools[3][src, :, :, -(-lo // 32):] = 0xFF, 0xFF, 0xFF, 0xFF
    got, again = both(q, pools, trip, dirty, kv_len, shared, sp=2, so=2, causal=True)
    assert same_bytes(got, want) and same_bytes(again, want)
    stable[1], dirty[0, NP - 1] = (-1, P)[page // 32 % 2], (P, -1)[page // 32 % 2]       # live entries out of range: zero codes under 127
    got, zeroed = both(q, pools, trip, dirty, kv_len, shared, sp=2, so=2, causal=True)
    assert same_bytes(got, zeroed) and not same_bytes(got, want)
    for t in pools:                                              # other bytes in both guard pages: the same output
        t._base[0], t._base[P + 1] = 0x3C, 0x3C
    assert same_bytes(both(q, pools, trip, dirty, kv_len, shared, sp=2, so=2, causal=True)[0], zeroed)


@pytest.mark.parametrize("r,T,B", ((4, 1, 5), (1, 3, 6)))
def test_rows_do_not_depend_on_the_rows_that_share_their_tile(r, T, B):
    page, NP, NPs, trip = 64, 5, 3, TRIPLES[4]
    q, pools, table, stable, _ = shared_case(21, B, HKV, r, T, page, NP, NPs, 64, 64, trip[0], trip[2], DEV, guard=True)
    kv_len, shared = lengths(B, 128, NP * page), (stable, slen(191, DEV))
    got = both(q, pools, trip, table, kv_len, shared, sp=2, so=2)[0]
    for b in range(B):
        one = both(tuple(t[b:b + 1] for t in q), pools, trip, table[b:b + 1], kv_len[b:b + 1], shared, sp=2, so=2)[0]
        assert same_bytes(got[b:b + 1], one), b


def test_a_captured_call_replays_on_a_rewritten_prefix_and_lengths():
    B, page, NP, NPs, trip = 5, 32, 12, 8, TRIPLES[0]
    q, pools, table, stable, _ = shared_case(22, B, HKV, 4, 1, page, NP, NPs, 64, 64, device=DEV, guard=True)
    kv_len, sl = lengths(B, 128, NP * page), slen(128, DEV)
    call = lambda: mx_flash_decode_paged(*q, trip[0], *pools, trip[2], table, kv_len, scale=0.21, kv_splits=2, shared=(stable, sl), shared_splits=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for n in (128, 256, 0):                                      # in place, between the replays; twice each
        sl.fill_(n), kv_len.copy_(lengths(B, n, NP * page).flip(0)), stable.copy_(stable.roll(1) if n == 256 else stable)
        want = _decode_shared_def(*q, trip[0], *pools, trip[2], table, kv_len, stable, sl, 0.21, False, trip[1], torch.float32, 2, 2)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert same_bytes(out, want), n
