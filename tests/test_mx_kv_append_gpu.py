"""``mx_kv_append`` on the GPU: the bytes of the one launch against ``_append_def`` on CPU copies -- every position of the write point in
its block, tokens that do not fit, the PLAIN route, NaN / Inf -- then a decoding loop and a captured graph against the eager result."""
import pytest
import torch

import test_mx_kv_append as TA
from qsparse_amd import MXKVCache, _hip, mx_flash_decode, mx_kv_append, mx_rope_table
from qsparse_amd.mx_kv_cache import _append_def
from qsparse_amd.mx_rope import _rope_def
from test_mx_kv_append import FORMATS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
DIMS = ((64, 64), (48, 40), (128, 96), (2, 1))
CASES = ((0, 1, 64), (31, 1, 64), (32, 1, 64), (33, 1, 70), (30, 33, 128), (0, 70, 70), (60, 8, 64), (5, 1, 37))       # (L, T, S)
B, HKV, HQ = 3, 2, 4


def operands(n, L, T, S, d, dv, dtype, with_q=True):
    """a CPU cache as 0xAB / NaN with the tail's defined columns filled, lengths (L, L / 2, min(S, L + 3)), and the new tokens"""
    g = torch.Generator().manual_seed(n)
    cache = TA.fresh(B, HKV, S, d, dv)
    cache[5] = torch.tensor((L, L // 2, min(S, L + 3)), dtype=torch.int32)
    for b, Lb in enumerate(cache[5].tolist()):
        cache[4][b, :, :, :Lb % 32] = torch.randn(HKV, dv, Lb % 32, generator=g)
    new = [torch.randn(B, h, T, n_, generator=g).to(dtype) for h, n_ in ((HKV, d), (HKV, dv))]
    return cache, new, (torch.randn(B, HQ, T, d, generator=g).to(dtype) if with_q else None)


def both(cache, fmts, new, q, rope, il):
    """(the launch's cache, tail and q pair on the GPU, the definition's on the CPU), each a list of tensors"""
    dev = [t.to(DEV) for t in cache]
    to = lambda t: None if t is None else t.to(DEV)
    got = mx_kv_append(*dev[:2], fmts[0], *dev[2:4], fmts[1], *dev[4:], *map(to, new), q_new=to(q), interleaved=il,
                       rope=None if rope is None else tuple(map(to, rope)))
    cpu = [t.clone() for t in cache]
    want = _append_def(*cpu[:2], fmts[0], *cpu[2:4], fmts[1], *cpu[4:], *new, q, rope, il)
    bits = lambda ts: [t.view(torch.int32) if t.dtype == torch.float32 else t for t in ts]      # (the tail holds NaN)
    return bits(dev[:5] + list(got or ())), bits(cpu[:5] + list(want or ()))


def untouched(kc, ks, vc, vs, lens, T):
    """do the bytes that the definition leaves alone still read 0xAB"""
    S, ok = kc.shape[2], True
    for b, L in enumerate(lens):
        Lp, lo = min(L + T, S), L // 32 * 32
        end = min(S, -(-Lp // 32) * 32) if Lp > L else lo
        for part in (kc[b, :, :L], kc[b, :, Lp:], ks[b, :, :L], ks[b, :, Lp:], vc[b, ..., :lo], vc[b, ..., end:], vs[b, ..., :lo // 32],
                     vs[b, ..., -(-end // 32):]):
            ok = ok and bool((part == 0xAB).all())
    return ok


@pytest.mark.parametrize("rope", (None, "half", "interleaved"))
@pytest.mark.parametrize("n,case", enumerate(CASES), ids=str)
def test_the_launch_equals_the_definition(n, case, rope):
    (L, T, S), (d, dv), dtype, fmts = case, DIMS[n % 4], DTYPES[n % 3], (FORMATS[n % 5], FORMATS[(n + 3) % 5])
    cache, new, q = operands(n, L, T, S, d, dv, dtype, with_q=n % 2 == 0)
    got, want = both(cache, fmts, new, q, None if rope is None else mx_rope_table(S + 2, d), rope == "interleaved")
    assert TA.same(got, want), (case, fmts, dtype)
    assert untouched(*got[:4], cache[5].tolist(), T)
    vec = S % 16 == 0 and d % 8 == 0 and dv % 8 == 0
    assert _hip.mx_kv_append_last_route == (_hip.MX_KV_APPEND_ROUTE_VEC if vec else _hip.MX_KV_APPEND_ROUTE_PLAIN)


@pytest.mark.parametrize("which", (2, 6), ids=("vt_codes", "k_new"))
def test_a_misaligned_base_takes_the_plain_route(which):
    cache, new, q = operands(20, 30, 33, 128, 64, 64, torch.bfloat16)
    rope, il = tuple(t.to(DEV) for t in mx_rope_table(128, 64)), False
    ops = [t.to(DEV) for t in cache + new + [q]]
    want = _append_def(*cache[:2], FORMATS[0], *cache[2:4], FORMATS[4], *cache[4:], *new, q, mx_rope_table(128, 64), il)    # (in place)
    t = ops[which]           # the same values one element off a 16-byte base
    ops[which] = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)[1:].view(t.shape).copy_(t)
    assert ops[which].data_ptr() % 16 != 0
    got = mx_kv_append(*ops[:2], FORMATS[0], *ops[2:4], FORMATS[4], *ops[4:8], q_new=ops[8], rope=rope, interleaved=il)
    assert _hip.mx_kv_append_last_route == _hip.MX_KV_APPEND_ROUTE_PLAIN
    assert TA.same(ops[:4] + list(got), cache[:4] + list(want)) and untouched(*(o.cpu() for o in ops[:4]), cache[5].tolist(), 33)


def test_nan_and_inf_mark_their_own_block_or_row():
    cache, new, _ = operands(21, 10, 40, 128, 64, 64, torch.float32, with_q=False)          # lengths (10, 5, 13)
    new[1][0, 0, 5, 3], new[1][1, 1, 30, 7], new[0][2, 0, 4, 9] = float("nan"), float("inf"), float("nan")
    got, want = both(cache, (FORMATS[0], FORMATS[1]), new, None, None, False)
    assert TA.same(got, want) and untouched(*got[:4], cache[5].tolist(), 40)
    ks, vs = got[1].cpu() == 0xFF, got[3].cpu() == 0xFF
    assert ks.nonzero().tolist() == [[2, 0, 13 + 4, 0]] and vs.nonzero().tolist() == [[0, 0, 3, 0], [1, 1, 7, 1]]


def test_a_growing_block_is_quantized_from_the_tail():
    assert TA.growing_block(DEV)


def decode_inputs(steps):
    g = torch.Generator().manual_seed(22)
    k, v, q = (torch.randn(2, h, 100 + steps, 64, generator=g).to(DEV) for h in (HKV, HKV, HQ))
    return k, v, q, tuple(t.to(DEV) for t in mx_rope_table(128, 64))


def test_a_decoding_loop_equals_decoding_on_a_cache_quantized_at_once():
    k, v, q, rope = decode_inputs(8)
    k_rot = _rope_def(k.cpu(), rope[0][:108].cpu(), rope[1][:108].cpu(), False, False)
    cache = MXKVCache(2, HKV, 128, 64, 64, FORMATS[0], FORMATS[4], DEV)
    cache.append(k[:, :, :100], v[:, :, :100], rope=rope)
    for L in range(100, 108):
        qc, qs = cache.append(k[:, :, L:L + 1], v[:, :, L:L + 1], q[:, :, L:L + 1], rope=rope)
        once = [t.to(DEV) for t in TA.one_shot(k_rot, v, (L + 1, L + 1), 128, FORMATS[0], FORMATS[4])]
        want = mx_flash_decode(qc, qs, FORMATS[0], *once, FORMATS[4], cache.kv_len, scale=0.125)
        assert torch.equal(cache.attend(qc, qs, scale=0.125), want) and bool(want.isfinite().all()), L
    assert cache.kv_len.tolist() == [108, 108]


def test_a_captured_step_replays_like_the_eager_loop():
    k, v, q, rope = decode_inputs(4)
    eager, cache = (MXKVCache(2, HKV, 128, 64, 64, FORMATS[0], FORMATS[0], DEV) for _ in range(2))
    for c in (eager, cache):
        c.append(k[:, :, :100], v[:, :, :100], rope=rope)
    static = [t[:, :, 100:101].clone() for t in (k, v, q)]
    step = lambda c, new: c.attend(*c.append(*new, rope=rope), scale=0.125)
    state = [t.clone() for t in vars(cache).values() if isinstance(t, torch.Tensor)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(cache, static)
    torch.cuda.current_stream().wait_stream(side)
    for t, s in zip((t for t in vars(cache).values() if isinstance(t, torch.Tensor)), state):
        t.copy_(s)                                               # (the warm-up step is undone)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(cache, static)
    for L in range(101, 104):
        new = [t[:, :, L:L + 1] for t in (k, v, q)]
        for t, s in zip(static, new):
            t.copy_(s)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, step(eager, new)) and torch.equal(cache.kv_len, eager.kv_len), L
    assert all(torch.equal(a, b) for a, b in zip((cache.k_codes, cache.vt_codes, cache.vt_scales), (eager.k_codes, eager.vt_codes, eager.vt_scales)))
