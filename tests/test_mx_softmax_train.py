"""The training side of the fused softmax on the CPU: ``mx_softmax_quantize(col_fmt=, return_stats=)``, ``mx_softmax_backward_quantize``
and ``mx_attention_train(softmax="fused")`` -- the torch expression of each definition against the definition written out here, the
distance to torch's own softmax backward as a condition, the exceptional rows, the layers, the refusals and empty tensors."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mx_softmax_ref as SR
import test_mx_softmax as TS
from qsparse_amd import (MXMultiheadAttention, MXTrainMultiheadAttention, mx_attention, mx_attention_train, mx_bmm,
                         mx_quantize_2way_batched, mx_softmax_backward_quantize, mx_softmax_quantize, quantize_with_mx)
from qsparse_amd.mx_norm import _row_sum
from qsparse_amd.mx_softmax import _exp_def, _mx_softmax_p

SCALE = 0.37
NAN_BITS = 0x7fc00000


def bits(t):
    return t.contiguous().view(torch.int32)


def stats_def(s3, add, scale, causal):
    """(m, Z) of the definition, op by op: float32 [G, T], the quiet NaN where the row is NaN as a whole"""
    G, T, S = s3.shape
    u = s3.to(torch.float32) * torch.tensor(scale, dtype=torch.float32)
    if add is not None:
        u = u + add
    if causal:
        u = u.masked_fill(~torch.ones(T, S, dtype=torch.bool).tril(), float("-inf"))
    m = u.amax(-1)
    Z = _row_sum(_exp_def(u - m[..., None]).reshape(G * T, S)).reshape(G, T)
    whole = ~torch.isfinite(m)
    nan = torch.tensor(NAN_BITS, dtype=torch.int32).view(torch.float32)
    return torch.where(whole, nan, m + 0.0), torch.where(whole, nan, Z), u      # (a zero maximum of either sign is handed out as +0)


def ds_def(dp3, s3, add, scale, causal):
    """ds float32 [G, T, S] of mx_softmax_backward_quantize's definition, one torch op per float32 operation, from s alone"""
    G, T, S = s3.shape
    m, Z, u = stats_def(s3, add, scale, causal)
    p = _exp_def(u - m[..., None]) / Z[..., None]
    p = torch.where(torch.isnan(m)[..., None], torch.full_like(p, float("nan")), p)
    dp32 = dp3.to(torch.float32)
    t = p * dp32
    D = _row_sum(t.reshape(G * T, S)).reshape(G, T, 1)
    d = dp32 - D
    return (p * d) * torch.tensor(scale, dtype=torch.float32)


def variant_add(kw):
    add = kw.get("mask")
    return SR.additive(add) if add is not None and add.dtype == torch.bool else add


@pytest.mark.parametrize("S", (1, 33, 197, 513))
@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
def test_forward_keywords_are_the_definition(dtype, S):
    for variant in ("none", "float", "bool_gts", "causal_lt") + (("causal_gt",) if S < 512 else ()):      # (T = S + 2 rows of the reference)
        s, kw, _ = TS.case(dtype, S, variant)
        T = s.shape[-2]
        s3, add, causal = s.reshape(-1, T, S), variant_add(kw), variant.startswith("causal")
        if add is not None and add.dim() > 2:
            add = add.reshape(-1, T, S)
        p = _mx_softmax_p(s3, add, SCALE, causal)
        m, Z, _ = stats_def(s3, add, SCALE, causal)
        for fmt, cfmt in (("mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp4_e2m1", "mxfp6_e2m3"), ("mxfp6_e3m2", "mxfp8_e4m3")):
            base = mx_softmax_quantize(s, scale=SCALE, fmt=fmt, **kw)
            full = mx_softmax_quantize(s, scale=SCALE, fmt=fmt, col_fmt=cfmt, return_stats=True, **kw)
            assert len(base) == 2 and len(full) == 6
            assert torch.equal(full[0], base[0]) and torch.equal(full[1], base[1])
            _, cc, cs = quantize_with_mx(p.transpose(-1, -2), cfmt, -1, return_codes=True)
            assert full[2].shape == s.shape[:-2] + (S, T) and full[3].shape == s.shape[:-2] + (S, (T + 31) // 32)
            assert torch.equal(full[2].reshape(cc.shape), cc) and torch.equal(full[3].reshape(cs.shape), cs), (variant, fmt)
            assert full[4].shape == s.shape[:-1] and full[4].dtype == torch.float32
            assert torch.equal(bits(full[4]).reshape(-1), bits(m).reshape(-1)) and torch.equal(bits(full[5]).reshape(-1), bits(Z).reshape(-1))
            only_col = mx_softmax_quantize(s, scale=SCALE, fmt=fmt, col_fmt=cfmt, **kw)
            only_stats = mx_softmax_quantize(s, scale=SCALE, fmt=fmt, return_stats=True, **kw)
            assert len(only_col) == 4 and len(only_stats) == 4
            assert all(torch.equal(a, b) for a, b in zip(only_col, full[:4]))
            assert torch.equal(only_stats[0], full[0]) and torch.equal(only_stats[1], full[1])
            assert torch.equal(bits(only_stats[2]), bits(full[4])) and torch.equal(bits(only_stats[3]), bits(full[5]))


def _bwd_case(dtype, ddtype, S, variant):
    s, kw, _ = TS.case(dtype, S, variant)
    dp = torch.randn(s.shape, generator=torch.Generator().manual_seed(S + 7)).to(ddtype)
    m, Z = mx_softmax_quantize(s, scale=SCALE, return_stats=True, **kw)[2:]
    T = s.shape[-2]
    add = variant_add(kw)
    if add is not None and add.dim() > 2:
        add = add.expand(s.shape[:-2] + (T, S)).reshape(-1, T, S)
    ds = ds_def(dp.reshape(-1, T, S), s.reshape(-1, T, S), add, SCALE, variant.startswith("causal")).reshape(s.shape)
    return s, kw, dp, m, Z, ds


@pytest.mark.parametrize("S", (1, 33, 197, 513))
@pytest.mark.parametrize("dtype,ddtype", ((torch.float32, torch.float32), (torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)),
                         ids=str)
def test_backward_is_the_two_way_quantizer_of_the_written_out_ds(dtype, ddtype, S):
    step = torch.tensor([5], dtype=torch.int64)
    for variant in ("none", "float", "bool_b1ts", "causal_lt", "causal_gt"):
        s, kw, dp, m, Z, ds = _bwd_case(dtype, ddtype, S, variant)
        for i, fmt in enumerate(SR.FMTS):
            cfmt = SR.FMTS[(i + 2) % 5]
            for sr in ((), ("stochastic", 1234, step)):
                got = mx_softmax_backward_quantize(dp, s, m, Z, scale=SCALE, row_fmt=fmt, col_fmt=cfmt,
                                                   **dict(zip(("rounding", "seed", "step"), sr)), **kw)
                want = mx_quantize_2way_batched(ds if ds.dim() > 2 else ds[None], fmt, cfmt, *sr)
                assert all(torch.equal(a.reshape(b.shape), b) for a, b in zip(got, want)), (variant, fmt, sr != ())
                assert got[0].shape == s.shape and got[2].shape == s.shape[:-2] + s.shape[-2:][::-1]
        assert int(step) == 5                                    # the op reads the counter, it does not advance it
        row = mx_softmax_backward_quantize(dp, s, m, Z, scale=SCALE, row_fmt="mxfp8_e5m2", col_fmt=None, **kw)
        col = mx_softmax_backward_quantize(dp, s, m, Z, scale=SCALE, row_fmt=None, col_fmt="mxfp8_e5m2", **kw)
        both = mx_softmax_backward_quantize(dp, s, m, Z, scale=SCALE, row_fmt="mxfp8_e5m2", col_fmt="mxfp8_e5m2", **kw)
        assert row[2] is None and row[3] is None and col[0] is None and col[1] is None
        assert torch.equal(row[0], both[0]) and torch.equal(row[1], both[1]) and torch.equal(col[2], both[2]) and torch.equal(col[3], both[3])


@pytest.mark.parametrize("fmt", ("mxfp8_e5m2", "mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e2m3"))
def test_distance_to_torch_softmax_backward(fmt):
    """a condition, not an identity: against the two-way quantizer of the ds torch's own softmax backward gives, the share of differing
    codes and of differing scale bytes stays at or below 1e-3 in both pairs.  Measured here: 0 of either, every case"""
    for shape, causal in (((8, 33, 197), False), ((8, 33, 197), True), ((4, 70, 64), False), ((2, 40, 1056), False)):
        g = torch.Generator().manual_seed(0)
        s = 3 * torch.randn(*shape, generator=g)
        dp = torch.randn(*shape, generator=g)
        T, S = shape[-2:]
        m, Z = mx_softmax_quantize(s, scale=0.125, is_causal=causal, return_stats=True)[2:]
        got = mx_softmax_backward_quantize(dp, s, m, Z, scale=0.125, is_causal=causal, row_fmt=fmt, col_fmt=fmt)
        st = s.clone().requires_grad_(True)
        u = st * 0.125
        if causal:
            u = u + torch.zeros(T, S).masked_fill(~torch.ones(T, S, dtype=torch.bool).tril(), float("-inf"))
        torch.softmax(u, -1).backward(dp)
        want = mx_quantize_2way_batched(st.grad, fmt, fmt)
        shares = [float((a != b).float().mean()) for a, b in zip(got, want)]
        print(f"{fmt} {shape} causal={causal}: differing row codes {shares[0]:.3e}, row scales {shares[1]:.3e}, col codes {shares[2]:.3e}, "
              f"col scales {shares[3]:.3e}")
        assert max(shares) <= 1e-3


def _qkv(seed, lead, T, S, d, dv, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(*lead, n, w, generator=g).to(dtype) for n, w in ((T, d), (S, d), (S, dv)))


def fused_train_composition(q, k, v, do, mask=None, causal=False, scale=None, fmts=("mxfp8_e4m3",) * 3 + ("mxfp8_e5m2",), sr=(),
                            need=(True, True, True)):
    """what ``mx_attention_train(softmax="fused")`` is defined as, from public calls: (o, dq, dk, dv)"""
    qk, pf, vf, gf = fmts
    Q2 = mx_quantize_2way_batched
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    need_ds = need[0] or need[1]
    q_row, q_rs, q_col, q_cs = Q2(q, qk, qk if need[1] else None)
    k_row, k_rs, k_col, k_cs = Q2(k, qk, qk if need[0] else None)
    s = mx_bmm(q_row, q_rs, qk, k_row, k_rs, qk)
    p = mx_softmax_quantize(s, mask, scale=scale, is_causal=causal, fmt=pf, col_fmt=pf if need[2] else None, return_stats=True)
    v_row, v_rs, v_col, v_cs = Q2(v, vf if need_ds else None, vf)
    o = mx_bmm(p[0], p[1], pf, v_col, v_cs, vf, None, q.dtype)
    rounding, seed, step = sr if sr else ("nearest", 0, None)
    g_row, g_rs, g_col, g_cs = Q2(do, gf if need_ds else None, gf if need[2] else None, rounding, seed, step)
    if step is not None:
        step = step + 1
    dq = dk = dv = None
    if need[2]:
        dv = mx_bmm(p[2], p[3], pf, g_col, g_cs, gf, None, v.dtype)
    if need_ds:
        dp = mx_bmm(g_row, g_rs, gf, v_row, v_rs, vf)
        ds = mx_softmax_backward_quantize(dp, s, p[-2], p[-1], mask, scale=scale, is_causal=causal, row_fmt=gf if need[0] else None,
                                          col_fmt=gf if need[1] else None, rounding=rounding, seed=seed + 1, step=step)
        if need[0]:
            dq = mx_bmm(ds[0], ds[1], gf, k_col, k_cs, qk, None, q.dtype)
        if need[1]:
            dk = mx_bmm(ds[2], ds[3], gf, q_col, q_cs, qk, None, k.dtype)
    return o, dq, dk, dv


TRAIN_CASES = (dict(lead=(2, 3), T=37, S=37, d=16, dv=16, causal=True),
               dict(lead=(2, 2), T=33, S=45, d=40, dv=24, dtype=torch.bfloat16, mask=True, scale=0.2, sr=True,
                    fmts=("mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e2m3", "mxfp8_e5m2")))


@pytest.mark.parametrize("c", TRAIN_CASES, ids=("causal", "masked_bf16_sr"))
def test_attention_train_fused_is_its_composition(c):
    dtype = c.get("dtype", torch.float32)
    q, k, v = _qkv(11, c["lead"], c["T"], c["S"], c["d"], c["dv"], dtype)
    do = torch.randn(*c["lead"], c["T"], c["dv"], generator=torch.Generator().manual_seed(12)).to(dtype)
    mask = SR.float_mask(13, (c["T"], c["S"])) if c.get("mask") else None
    fmts = c.get("fmts", ("mxfp8_e4m3",) * 3 + ("mxfp8_e5m2",))
    kw = dict(qk_fmt=fmts[0], p_fmt=fmts[1], v_fmt=fmts[2])
    step = torch.tensor([3], dtype=torch.int64) if c.get("sr") else None
    sr = ("stochastic", 99, step) if c.get("sr") else ()
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = mx_attention_train(qg, kg, vg, mask, c.get("causal", False), c.get("scale"), grad_fmt=fmts[3], softmax="fused",
                           **dict(zip(("grad_rounding", "seed", "step"), sr)), **kw)
    assert o.dtype == dtype and o.shape == q.shape[:-1] + (c["dv"],)
    with torch.no_grad():
        inf = mx_attention(q, k, v, mask, c.get("causal", False), c.get("scale"), out_dtype=dtype, softmax="fused", **kw)
    assert torch.equal(o.detach(), inf)
    want = fused_train_composition(q, k, v, do, mask, c.get("causal", False), c.get("scale"), fmts,
                                   ("stochastic", 99, torch.tensor([3], dtype=torch.int64)) if c.get("sr") else ())
    o.backward(do)
    for name, got, ref in zip(("o", "dq", "dk", "dv"), (o.detach(), qg.grad, kg.grad, vg.grad), want):
        assert got.dtype == ref.dtype and torch.equal(got, ref), name
        assert bool(torch.isfinite(got.float()).all()) and bool(got.float().abs().sum() > 0), name
    if step is not None:
        assert int(step) == 5                                    # by two
    # the default is "torch", which is what it always was
    a = mx_attention_train(q, k, v, mask, c.get("causal", False), c.get("scale"), **kw)
    b = mx_attention_train(q, k, v, mask, c.get("causal", False), c.get("scale"), softmax="torch", **kw)
    assert torch.equal(a, b)
    with pytest.raises(TypeError):
        mx_attention_train(q, k, v, None, False, None, "fused")
    with pytest.raises(ValueError):
        mx_attention_train(q, k, v, softmax="flash")


def test_only_the_pairs_somebody_needs(monkeypatch):
    import qsparse_amd.mx_batched_train as M
    calls, ds_calls, fwd_calls = [], [], []
    real, real_ds, real_fwd = M.mx_quantize_2way_batched, M.mx_softmax_backward_quantize, M.mx_softmax_quantize

    def spy(x, row_fmt=None, col_fmt=None, *args, **kw):
        if tuple(x.shape) != (2, 9, 12):                         # (the backward op's CPU path quantizes its ds [T, S] through it)
            calls.append((tuple(x.shape), row_fmt is not None, col_fmt is not None))
        return real(x, row_fmt, col_fmt, *args, **kw)

    def spy_ds(*args, **kw):
        ds_calls.append((kw["row_fmt"] is not None, kw["col_fmt"] is not None))
        return real_ds(*args, **kw)

    def spy_fwd(*args, **kw):
        fwd_calls.append(kw.get("col_fmt") is not None)
        return real_fwd(*args, **kw)

    monkeypatch.setattr(M, "mx_quantize_2way_batched", spy)
    monkeypatch.setattr(M, "mx_softmax_backward_quantize", spy_ds)
    monkeypatch.setattr(M, "mx_softmax_quantize", spy_fwd)
    q, k, v = _qkv(21, (2,), 9, 12, 32, 8)
    do = torch.randn(2, 9, 8, generator=torch.Generator().manual_seed(22))
    Q, K, V, DO = (2, 9, 32), (2, 12, 32), (2, 12, 8), (2, 9, 8)
    table = (((False, False, True), [(Q, True, False), (K, True, False), (V, False, True), (DO, False, True)], [], True),
             ((True, False, False), [(Q, True, False), (K, True, True), (V, True, True), (DO, True, False)], [(True, False)], False),
             ((False, True, True), [(Q, True, True), (K, True, False), (V, True, True), (DO, True, True)], [(False, True)], True),
             ((True, True, True), [(Q, True, True), (K, True, True), (V, True, True), (DO, True, True)], [(True, True)], True))
    for need, want, want_ds, want_col in table:
        calls.clear(), ds_calls.clear(), fwd_calls.clear()
        ts = [t.clone().requires_grad_(n) for t, n in zip((q, k, v), need)]
        o = mx_attention_train(*ts, softmax="fused")
        o.backward(do)
        assert calls == want and ds_calls == want_ds and fwd_calls == [want_col], (need, calls, ds_calls, fwd_calls)
        assert [t.grad is not None for t in ts] == list(need)
        ref = fused_train_composition(q, k, v, do, need=need)
        for t, r in zip(ts, ref[1:]):
            assert (t.grad is None and r is None) or torch.equal(t.grad, r)
    calls.clear()
    with torch.no_grad():                                        # nothing is kept, no col pair is computed
        mx_attention_train(q.clone().requires_grad_(True), k, v, softmax="fused")
    assert calls == [(Q, True, False), (K, True, False), (V, False, True)]


def test_near_float_attention():
    """the bound of test_mx_bmm_train.py, (a - b).norm() < 0.2 * b.norm(), for the output and the three gradients"""
    q, k, v = _qkv(31, (2, 2), 48, 48, 32, 32)
    do = torch.randn(2, 2, 48, 32, generator=torch.Generator().manual_seed(32))
    ref = [t.clone().requires_grad_(True) for t in (q, k, v)]
    F.scaled_dot_product_attention(*ref, is_causal=True).backward(do)
    for mode in ("fused", "torch"):
        ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
        o = mx_attention_train(*ts, is_causal=True, softmax=mode)
        o.backward(do)
        want_o = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        errs = [float((o.detach() - want_o).norm() / want_o.norm())] + [float((t.grad - r.grad).norm() / r.grad.norm()) for t, r in zip(ts, ref)]
        print(f"{mode}: relative error of o, dq, dk, dv = " + ", ".join(f"{e:.4f}" for e in errs))
        if mode == "fused":
            assert max(errs) < 0.2


@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
def test_exceptional_rows(dtype):
    s, mask, expect = TS._special_rows(dtype)
    fmt = "mxfp8_e4m3"
    rc, rs, cc, cs, m, Z = mx_softmax_quantize(s, mask, scale=SCALE, fmt=fmt, col_fmt=fmt, return_stats=True)
    p = _mx_softmax_p(s, mask, SCALE, False)
    _, wc, ws = quantize_with_mx(p.transpose(-1, -2), fmt, -1, return_codes=True)
    assert torch.equal(cc, wc) and torch.equal(cs, ws)
    base = mx_softmax_quantize(s, mask, scale=SCALE, fmt=fmt)
    assert torch.equal(rc, base[0]) and torch.equal(rs, base[1])
    wm, wZ, _ = stats_def(s, mask, SCALE, False)
    assert torch.equal(bits(m), bits(wm)) and torch.equal(bits(Z), bits(wZ))
    for r in range(9):
        nan = expect.get(r) == "nan"
        assert (int(bits(m)[0, r]) == NAN_BITS) == nan and (int(bits(Z)[0, r]) == NAN_BITS) == nan, r
        if not nan:
            assert float(Z[0, r]) >= 1.0 and bool(torch.isfinite(m[0, r]))
    assert bool((cs == 0xFF).all())                              # T = 9: every column block touches a NaN row
    assert float(m[0, 8]) == float((s[0, 8].float() * SCALE).max())          # -inf beside finite values: a plain row
    dp = torch.randn(1, 9, 40, generator=torch.Generator().manual_seed(3))
    ds = ds_def(dp, s, mask, SCALE, False)
    got = mx_softmax_backward_quantize(dp, s, m, Z, mask, scale=SCALE, row_fmt="mxfp8_e5m2", col_fmt="mxfp8_e5m2")
    want = mx_quantize_2way_batched(ds, "mxfp8_e5m2", "mxfp8_e5m2")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    for r in range(9):
        nan = expect.get(r) == "nan"
        assert bool(torch.isnan(ds[0, r]).all()) == nan and bool(torch.isnan(ds[0, r]).any()) == nan, r
        assert bool((got[1][0, r] == 0xFF).all()) == nan, r
    assert not bool((got[0][0, 8, 5:30] & 0x7F).any())           # p = 0 there: ds is a (signed) zero


@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
def test_a_nan_or_inf_in_dp_takes_its_row_alone(bad):
    s = SR.scores(41, (2, 6, 70), torch.float32)
    dp = torch.randn(2, 6, 70, generator=torch.Generator().manual_seed(42))
    m, Z = mx_softmax_quantize(s, scale=SCALE, is_causal=True, return_stats=True)[2:]
    clean = mx_softmax_backward_quantize(dp, s, m, Z, scale=SCALE, is_causal=True, row_fmt="mxfp8_e5m2", col_fmt="mxfp8_e5m2")
    dp2 = dp.clone()
    dp2[1, 2, 50] = bad                                          # behind the causal limit of row 2: the definition reads it all the same
    got = mx_softmax_backward_quantize(dp2, s, m, Z, scale=SCALE, is_causal=True, row_fmt="mxfp8_e5m2", col_fmt="mxfp8_e5m2")
    assert bool((got[1][1, 2] == 0xFF).all()) and not bool(got[0][1, 2].any())
    assert bool((got[3][1, :, 0] == 0xFF).all())                 # every column's first block holds row 2
    keep = torch.ones(2, 6, dtype=torch.bool)
    keep[1, 2] = False
    assert torch.equal(got[0][keep], clean[0][keep]) and torch.equal(got[1][keep], clean[1][keep])
    assert torch.equal(got[2][0], clean[2][0]) and torch.equal(got[3][0], clean[3][0])


def test_layers_forward_the_keyword():
    torch.manual_seed(0)
    mha = nn.MultiheadAttention(32, 4, batch_first=True)
    x = torch.randn(2, 9, 32)
    assert MXTrainMultiheadAttention.from_float(mha).softmax == "torch"
    layer = MXTrainMultiheadAttention.from_float(mha, softmax="fused", grad_rounding="stochastic", seed=5)
    assert layer.softmax == "fused" and "softmax='fused'" in repr(layer)
    y = layer(x, is_causal=True)[0]
    y.sum().backward()
    assert int(layer.sr_step) == 2
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0) for p in mha.parameters())
    inf = layer.to_inference()
    assert isinstance(inf, MXMultiheadAttention) and inf.softmax == "fused"
    with torch.no_grad():
        assert torch.equal(inf(x, is_causal=True)[0], layer(x, is_causal=True)[0])
    assert MXTrainMultiheadAttention.from_float(mha, softmax="torch").to_inference().softmax == "torch"
    direct = MXTrainMultiheadAttention(layer.in_proj, layer.out_proj, 4, True, softmax="fused")
    with torch.no_grad():
        assert torch.equal(direct(x)[0], layer(x)[0])
    with pytest.raises(ValueError):
        MXTrainMultiheadAttention.from_float(mha, softmax="flash")


def test_refusals():
    s = SR.scores(3, (2, 4, 33), torch.float32)
    dp = torch.randn(2, 4, 33)
    m, Z = mx_softmax_quantize(s, return_stats=True)[2:]
    ok = dict(row_fmt="mxfp8_e5m2", col_fmt="mxfp8_e5m2")
    with pytest.raises(ValueError):
        mx_softmax_backward_quantize(dp, s, m, Z, row_fmt=None, col_fmt=None)
    with pytest.raises(TypeError):
        mx_softmax_backward_quantize(dp, s, m, Z)                # the formats are required keywords
    with pytest.raises(ValueError):
        mx_softmax_backward_quantize(dp, s, m, Z, torch.zeros(4, 33), is_causal=True, **ok)
    with pytest.raises(ValueError):
        mx_softmax_quantize(s, torch.zeros(4, 33), is_causal=True, col_fmt="mxfp8_e4m3")
    for bad in (dict(dp=dp.double()), dict(s=s.double()), dict(m=m.double()), dict(Z=Z.to(torch.bfloat16)), dict(dp=dp.numpy())):
        with pytest.raises(TypeError):
            mx_softmax_backward_quantize(**{**dict(dp=dp, s=s, m=m, Z=Z), **bad}, **ok)
    for bad in (dict(dp=dp[:, :3]), dict(m=m[:, :3]), dict(Z=Z[0]), dict(m=m.to("meta")), dict(dp=dp.to("meta"))):
        with pytest.raises(ValueError):
            mx_softmax_backward_quantize(**{**dict(dp=dp, s=s, m=m, Z=Z), **bad}, **ok)
    with pytest.raises(ValueError):
        mx_softmax_backward_quantize(dp, s, m, Z, torch.zeros(4, 33, device="meta"), **ok)
    with pytest.raises(ValueError):
        mx_softmax_backward_quantize(dp, s, m, Z, row_fmt="mxfp7", col_fmt=None)
    with pytest.raises(ValueError):
        mx_softmax_quantize(s, col_fmt="mxfp7")
    with pytest.raises(ValueError):
        mx_softmax_backward_quantize(dp, s, m, Z, rounding="up", **ok)
    for name in ("dp", "s", "m", "Z"):
        ops = dict(dp=dp, s=s, m=m, Z=Z)
        ops[name] = ops[name].clone().requires_grad_(True)
        with pytest.raises(RuntimeError):
            mx_softmax_backward_quantize(**ops, **ok)
        with torch.no_grad():
            assert not mx_softmax_backward_quantize(**ops, **ok)[0].requires_grad
    with pytest.raises(RuntimeError):
        mx_softmax_backward_quantize(dp, s, m, Z, torch.zeros(4, 33, requires_grad=True), **ok)
    with pytest.raises(RuntimeError):
        mx_softmax_quantize(s.clone().requires_grad_(True), col_fmt="mxfp8_e4m3", return_stats=True)
    q, k, v = _qkv(1, (2,), 4, 33, 16, 8)
    with pytest.raises(RuntimeError):
        mx_attention_train(q, k, v, torch.zeros(4, 33, requires_grad=True), softmax="fused")
    with pytest.raises(ValueError):
        mx_attention_train(q, k, v, torch.zeros(4, 33), True, softmax="fused")
    with pytest.raises(TypeError):
        mx_attention_train(q.double(), k, v, softmax="fused")
    with pytest.raises(ValueError):
        mx_attention_train(q, k.to("meta"), v, softmax="fused")
    with pytest.raises(ValueError):
        mx_attention_train(q, k, v, torch.zeros(4, 32), softmax="fused")


@pytest.mark.parametrize("shape", ((0, 4, 33), (2, 0, 33), (2, 4, 0)))
def test_empty_tensors(shape):
    G, T, S = shape
    s, dp = torch.zeros(shape), torch.zeros(shape)
    out = mx_softmax_quantize(s, fmt="mxfp8_e4m3", col_fmt="mxfp4_e2m1", return_stats=True)
    assert [tuple(t.shape) for t in out] == [(G, T, S), (G, T, (S + 31) // 32), (G, S, T), (G, S, (T + 31) // 32), (G, T), (G, T)]
    assert [t.dtype for t in out] == [torch.uint8] * 4 + [torch.float32] * 2
    got = mx_softmax_backward_quantize(dp, s, out[4], out[5], row_fmt="mxfp8_e5m2", col_fmt="mxfp8_e5m2")
    assert [tuple(t.shape) for t in got] == [(G, T, S), (G, T, (S + 31) // 32), (G, S, T), (G, S, (T + 31) // 32)]
    assert mx_softmax_backward_quantize(dp, s, out[4], out[5], row_fmt=None, col_fmt="mxfp8_e5m2")[:2] == (None, None)
