"""``mx_kv_append`` on the CPU: ``_append_def`` appended in uneven steps against ONE quantization of the whole float history, a block whose
scale grows a millionfold with its last token, and the argument refusals.  The caches start as 0xAB and ``v_tail`` as NaN, so a byte
written where the definition writes none, or an unspecified tail column that is read, shows."""
import pytest
import torch

from qsparse_amd import MXKVCache, mx_kv_append, mx_rope_table, quantize_with_mx
from qsparse_amd.mx_rope import _rope_def
from qsparse_amd.quantize import MX_FORMATS

FORMATS = tuple(MX_FORMATS)
DIMS = ((64, 64), (48, 40), (2, 1))
STEPS = (1, 1, 30, 1, 33, 64, 5)


def fresh(B, Hkv, S, d, dv, dev="cpu"):
    """(k_codes, k_scales, vt_codes, vt_scales, v_tail, kv_len): 0xAB, NaN, zero lengths"""
    ab = lambda *shape: torch.full(shape, 0xAB, dtype=torch.uint8, device=dev)
    return [ab(B, Hkv, S, d), ab(B, Hkv, S, -(-d // 32)), ab(B, Hkv, dv, S), ab(B, Hkv, dv, -(-S // 32)),
            torch.full((B, Hkv, dv, 32), float("nan"), device=dev), torch.zeros(B, dtype=torch.int32, device=dev)]


def codes(x, fmt):
    return quantize_with_mx(x, fmt, -1, return_codes=True)[1:]


def one_shot(k_rot, v, lens, S, qk_fmt, v_fmt):
    """the cache after `lens[b]` tokens of the float32 histories `k_rot` [B, Hkv, N, d] (rotated), `v` [B, Hkv, N, dv], quantized at once
    on the CPU; 0xAB wherever no append from an empty cache writes"""
    kc, ks, vc, vs = fresh(*k_rot.shape[:2], S, k_rot.shape[3], v.shape[3])[:4]
    for b, L in enumerate(lens):
        end = min(S, -(-L // 32) * 32)
        kc[b, :, :L], ks[b, :, :L] = codes(k_rot[b, :, :L].cpu(), qk_fmt)
        vc[b, :, :, :end], vs[b, :, :, :-(-end // 32)] = codes(torch.nn.functional.pad(v[b, :, :L].cpu().transpose(-1, -2), (0, end - L)), v_fmt)
    return kc, ks, vc, vs


def same(got, want):
    return all(torch.equal(g.cpu(), w) for g, w in zip(got, want))


@pytest.mark.parametrize("dims", DIMS, ids=str)
@pytest.mark.parametrize("n,fmt", enumerate(FORMATS), ids=str)
def test_uneven_appends_equal_one_quantization_of_the_history(n, fmt, dims):
    (d, dv), S, N, il = dims, 140, sum(STEPS), bool(n & 1)
    g = torch.Generator().manual_seed(n)
    k, v = torch.randn(2, 2, N, d, generator=g), torch.randn(2, 2, N, dv, generator=g) * 3
    rope = mx_rope_table(S, d)
    k_rot = _rope_def(k, rope[0][:N], rope[1][:N], il, False)
    cache, v_fmt, L = fresh(2, 2, S, d, dv), FORMATS[(n + 2) % 5], 0
    for T in STEPS:
        assert mx_kv_append(*cache[:2], fmt, *cache[2:4], v_fmt, *cache[4:], k[:, :, L:L + T], v[:, :, L:L + T], rope=rope, interleaved=il) is None
        L += T
        cache[5] += T
        assert same(cache[:4], one_shot(k_rot, v, (L, L), S, fmt, v_fmt)), (L, T)
    assert torch.equal(cache[4][..., :L % 32], v[:, :, 128:].transpose(-1, -2)) and bool(cache[4][..., L % 32:].isnan().all())


def growing_block(dev):
    """positions 0 .. 30 of size 1e-3, position 31 of size 1e3, appended one by one: the block's scale rises 20 binades with its last
    token and the 31 old codes must come from the tail's floats, not from their old codes"""
    g = torch.Generator().manual_seed(7)
    k, v = torch.randn(1, 2, 32, 64, generator=g), torch.randn(1, 2, 32, 40, generator=g) * 1e-3
    v[:, :, 31] *= 1e6
    cache = fresh(1, 2, 64, 64, 40, dev)
    for t in range(32):
        mx_kv_append(*cache[:2], FORMATS[0], *cache[2:4], FORMATS[0], *cache[4:], k[:, :, t:t + 1].to(dev), v[:, :, t:t + 1].to(dev))
        cache[5] += 1
    return same(cache[:4], one_shot(k, v, (32,), 64, FORMATS[0], FORMATS[0]))


def test_a_block_that_grows_is_quantized_from_the_tail():
    assert growing_block("cpu")


def test_the_cache_class_appends_and_counts():
    g = torch.Generator().manual_seed(8)
    k, v, q = (torch.randn(2, h, 5, 32, generator=g) for h in (2, 2, 4))
    cache = MXKVCache(2, 2, 40, 32, 32, FORMATS[0], FORMATS[4])
    qc, qs = cache.append(k, v, q)
    assert cache.kv_len.tolist() == [5, 5] and same((qc, qs), codes(q, FORMATS[0]))
    assert same((cache.k_codes[:, :, :5], cache.vt_codes[..., :5]), (codes(k, FORMATS[0])[0], codes(v.transpose(-1, -2), FORMATS[4])[0]))
    assert cache.attend(qc, qs, scale=0.2).shape == (2, 4, 5, 32)


BAD = {
    "v_tail": lambda a, kw: a.__setitem__(6, a[6][..., :31]),
    "kv_len": lambda a, kw: a.__setitem__(7, a[7].long()),
    "v_new has shape": lambda a, kw: a.__setitem__(9, a[9][:, :, :1]),
    "share one dtype": lambda a, kw: a.__setitem__(9, a[9].half()),
    "no multiple of Hkv": lambda a, kw: kw.update(q_new=torch.zeros(2, 3, 2, 6)),
    "q_new has shape": lambda a, kw: kw.update(q_new=torch.zeros(2, 4, 2, 8)),
    "P, d / 2": lambda a, kw: kw.update(rope=mx_rope_table(39, 6)),
    "unknown MX format": lambda a, kw: a.__setitem__(2, "mxfp8"),
    "written in place": lambda a, kw: a.__setitem__(3, torch.zeros(2, 2, 40, 5, dtype=torch.uint8).transpose(-1, -2)),
    "T >= 1": lambda a, kw: (a.__setitem__(8, a[8][:, :, :0]), a.__setitem__(9, a[9][:, :, :0])),
    "dv <= 128": lambda a, kw: (a.__setitem__(3, torch.zeros(2, 2, 129, 40, dtype=torch.uint8)),
                                a.__setitem__(4, torch.zeros(2, 2, 129, 2, dtype=torch.uint8))),
    "an even d": lambda a, kw: (a.__setitem__(0, a[0][..., :5].contiguous()), a.__setitem__(8, a[8][..., :5]),
                                kw.update(rope=mx_rope_table(40, 6))),
}


@pytest.mark.parametrize("message", BAD, ids=str)
def test_arguments_outside_the_range_are_refused(message):
    c = fresh(2, 2, 40, 6, 5)
    args, kw = [c[0], c[1], FORMATS[0], c[2], c[3], FORMATS[0], c[4], c[5], torch.zeros(2, 2, 2, 6), torch.zeros(2, 2, 2, 5)], {}
    mx_kv_append(*args)
    BAD[message](args, kw)
    with pytest.raises(ValueError, match=message):
        mx_kv_append(*args, **kw)
