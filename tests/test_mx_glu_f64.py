"""The gated (GLU) MX family against float64 without a GPU: the reference and the bounds of tests/mx_glu_ref.py checked against
float32 arithmetic on the CPU and against the constants of tests/test_mx_glu_train.py, the CPU paths held to them, the exemption
caps of every input set that tests/test_mx_glu_f64_gpu.py uses asserted from the reference alone, and mutated float32 references
standing in for a wrong kernel, which the bounds and the code-level comparison must catch."""
import pytest
import torch
import torch.nn.functional as F

import mx_gemm_ref as G
import mx_glu_ref as R
from qsparse_amd import (mx_glu_backward_quantize, mx_glu_linear, mx_glu_deinterleave, mx_glu_interleave, mx_glu_matmul, mx_grouped_glu_matmul,
                         mx_matmul, mx_quantize_2way, quantize_with_mx)
from qsparse_amd.mx_glu_train import _glu_dv
from test_mx_glu_train import ACT_ERR

DTS = (torch.float32, torch.bfloat16, torch.float16)
ALPHA32, BETA32 = torch.tensor(R.ALPHA).float(), torch.tensor(R.BETA).float()


def test_the_interleave_is_the_packages():
    g, u = torch.arange(3 * 96.0).reshape(3, 96), -torch.arange(3 * 96.0).reshape(3, 96)
    v = R.interleave(g, u)
    assert torch.equal(v, mx_glu_interleave(g, u, dim=-1))
    assert all(torch.equal(a, b) for a, b in zip(R.deinterleave(v), mx_glu_deinterleave(v, dim=-1)))


# ---- the float32 expressions of the header, one torch op per rounding, with the mutations that stand in for a wrong kernel ---------------
def f32_parts(g, act, mutation=None):
    """(act(g), act'(g)) in float32 by elementary torch ops in the header's order.  The one fma of gelu's derivative is a float64 product
    and sum rounded to float32 (a second rounding of 2^-29 of an ulp at most: inside SLACK).  `mutation`: "tanh" (the tanh-form gelu),
    "no_term" (silu' without g (1 - s)), "beta" (kBeta times 1 + 2^-10), "expf" (every expf times 1 + 2^-12)"""
    assert g.dtype == torch.float32
    wrong_exp = (1 + 2.0 ** -12) if mutation == "expf" else 1.0
    if act == "relu":
        pos = g > 0
        return torch.where(pos, g, torch.where(g != g, g, torch.zeros_like(g))), torch.where(pos, torch.ones_like(g), torch.where(g != g, g, torch.zeros_like(g)))
    if act == "silu":
        e = torch.exp(-g) * wrong_exp
        s = 1.0 / (1.0 + e)
        return g / (1.0 + e), s if mutation == "no_term" else s * (1.0 + g * (1.0 - s))
    w = 1.0 + torch.erf(g * ALPHA32)
    a = F.gelu(g, approximate="tanh") if mutation == "tanh" else (g * 0.5) * w
    beta = (BETA32.double() * (1 + 2.0 ** -10)).float() if mutation == "beta" else BETA32
    pdf = (torch.exp(-0.5 * g * g) * wrong_exp) * beta
    return a, (g.double() * pdf.double() + (0.5 * w).double()).float()


def f32_glu(d, v, act, mutation=None):
    """(z [T, H], dv [T, 2 H]) in float32 from f32_parts; "swap" takes the up half for the gate and the gate half for up"""
    g, up = R.deinterleave(v.float())
    if mutation == "swap":
        g, up = up, g
    a, da = f32_parts(g, act, mutation)
    d = d.float()
    return a * up, R.interleave((d * up) * da, d * a)


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", R.ACTS)
def test_pointwise_bounds_stay_inside_the_constants_of_the_float64_check(act):
    g = torch.cat([torch.linspace(-8, 8, 400001, dtype=torch.float64), torch.tensor([-8.0, 8.0, 0.0, -0.0, 1.0, -1.0, 0.5, -0.5]).double()])
    e_da, e_a = ACT_ERR[act]
    got_da, got_a = float(R.E_da(g, act).max()), float(R.E_a(g, act).max())
    print(f"{act}: max E_da = {got_da / R.U:.2f} u (ACT_ERR {e_da / R.U:.0f} u), max E_a = {got_a / R.U:.2f} u (ACT_ERR {e_a / R.U:.0f} u)")
    assert got_da <= e_da and got_a <= e_a


def whole_range():
    mags = torch.cat([torch.logspace(-45, 38, 2000, dtype=torch.float64), torch.linspace(80, 110, 3001, dtype=torch.float64),
                      torch.linspace(0, 20, 20001, dtype=torch.float64),
                      torch.tensor([0.0, 1.0, 20.0, 90.0, 104.0, 448.0, 57344.0, 448 * 2.0 ** -20, 448 * 2.0 ** 100, 1e-30, 3.0e38, 88.72, 88.73, 87.3, 87.4])])
    g = torch.cat([mags, -mags]).float()
    return g[g.isfinite()]


@pytest.mark.parametrize("act", R.ACTS)
def test_bounds_hold_for_float32_arithmetic_over_the_whole_range(act):
    """the CPU's float32 evaluation (its expf and erff are within 1 ulp) stays inside E_a / E_da from the subnormals to 3e38, through the
    saturation of expf at |g| = 87.3 .. 88.7 and the cancellations; the results are finite and the classes agree"""
    g = whole_range()
    a, da = f32_parts(g, act)
    for name, got, want, E in (("act", a, R.act64(g, act), R.E_a(g, act)), ("act'", da, R.dact64(g, act), R.E_da(g, act))):
        assert bool(got.isfinite().all()) and bool(want.isfinite().all())
        err = (got.double() - want).abs()
        worst = int((err - E).argmax())
        print(f"{act} {name}: max err / bound = {float((err / E.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= E).all()), (name, float(g[worst]), float(err[worst]), float(E[worst]))
    if act == "silu":
        assert bool((a[g == -90.0] == 0).all()) and float(R.act64(torch.tensor([-90.0]), act).abs()) > R.ETA      # the saturation is real
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")])
    a, da = f32_parts(bad, act)
    for got, want in ((a, R.act64(bad, act)), (da, R.dact64(bad, act))):
        assert torch.equal(got.isnan(), want.isnan()) and torch.equal(got.double()[~want.isnan()], want[~want.isnan()])


@pytest.mark.parametrize("act", R.ACTS)
def test_dv_bound_on_the_inputs_of_the_existing_float64_check(act):
    """the inputs of test_dv_float32_against_float64: ``_glu_dv`` stays inside dv_bound, which stays inside the form stated there"""
    T, H = 64, 64
    g = (torch.rand(T, H, generator=torch.Generator().manual_seed(1)) * 16 - 8)
    g[0, :8] = torch.tensor([-8.0, 8.0, 0.0, -0.0, 1.0, -1.0, 0.5, -0.5])
    up = torch.randn(T, H, generator=torch.Generator().manual_seed(2)) * 2
    d = torch.randn(T, H, generator=torch.Generator().manual_seed(3))
    v = R.interleave(g, up)
    want, tol = R.dv64(d, v, act)
    stated = R.dv_bound_stated(d, up, g, act)
    e_da, e_a = ACT_ERR[act]
    constants = R.interleave((d.double() * up.double()).abs() * (e_da + 3 * R.U), d.double().abs() * (e_a + 8 * R.U))
    assert bool((tol <= stated).all()) and bool((stated <= constants).all())
    err = (_glu_dv(d, v, act).double() - want).abs()
    print(f"{act}: max error / bound = {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= tol).all())


# ---- the CPU paths ------------------------------------------------------------------------------------------------------------------
def fwd_reference(M, H, K, E=None, offs=None):
    """(ops, v64): the exact-class operands and the float64 product, asserted to be a float32 exactly (the tail rows of a grouped
    product +0)"""
    ops = R.fwd_operands(M, H, K, E)
    if E is None:
        v64 = G.reference(ops[0], ops[1], R.FA, ops[2], ops[3], R.FB, ops[4])[1]
    else:
        v64 = torch.zeros(M, 2 * H, dtype=torch.float64)
        for e, (lo, hi) in enumerate(zip([0] + offs[:-1], offs)):
            if hi > lo:
                v64[lo:hi] = G.reference(ops[0][lo:hi], ops[1][lo:hi], R.FA, ops[2][e], ops[3][e], R.FB, ops[4][e])[1]
    assert torch.equal(v64.float().double(), v64)
    return ops, v64


def gates_are_spread(v64):
    g = R.deinterleave(v64)[0]
    assert float((g.abs() <= 3).double().mean()) >= 0.5 and float(g.max()) > 8 and float(g.min()) < -8


@pytest.mark.parametrize("act", R.ACTS)
def test_cpu_glu_matmul_stays_inside_glu_bound(act):
    for M, H, K in R.FWD_SHAPES:
        ops, v64 = fwd_reference(M, H, K)
        gates_are_spread(v64)
        args = (ops[0], ops[1], R.FA, ops[2], ops[3], R.FB, ops[4])
        assert G.same(mx_matmul(*args), v64.float())
        z64 = R.glu64(v64, act)
        for dt in DTS:
            ok, ratio = R.within_glu(mx_glu_matmul(*args, dt, act=act), z64, R.glu_bound(v64, act, dt), dt)
            print(f"{act} {dt} {(M, H, K)}: max err / bound = {ratio:.3f}")
            assert ok
        for fmt in R.FWD_FMTS:
            codes, scales = mx_glu_matmul(*args, act=act, out_fmt=fmt)
            R.codes_agree(codes, scales, fmt, z64, R.glu_bound(v64, act, torch.float32), what=f"cpu forward {act} {(M, H, K)}")


GROUPED = (70, 32, 40, 3, [33, 33, 70])          # T, H, K, E, ends: an empty group and a ragged last one


@pytest.mark.parametrize("act", ("silu", "gelu"))
def test_cpu_grouped_glu_matmul_stays_inside_glu_bound(act):
    T, H, K, E, ends = GROUPED
    ops, v64 = fwd_reference(T, H, K, E, ends)
    args = (ops[0], ops[1], R.FA, ops[2], ops[3], R.FB, torch.tensor(ends, dtype=torch.int32), ops[4])
    z64 = R.glu64(v64, act)
    ok, ratio = R.within_glu(mx_grouped_glu_matmul(*args, act=act), z64, R.glu_bound(v64, act, torch.float32), torch.float32)
    assert ok, ratio
    for fmt in R.FWD_FMTS:
        codes, scales = mx_grouped_glu_matmul(*args, act=act, out_fmt=fmt)
        R.codes_agree(codes, scales, fmt, z64, R.glu_bound(v64, act, torch.float32), what=f"cpu grouped {act}")


def bwd_cases():
    """(T, H, ddt, vdt, narrow, fmt, pairs): every backward input set of the GPU file with each format and pair it is used with"""
    for T, H in R.BWD_SHAPES:
        for ddt, vdt in R.BWD_DTYPES:
            for narrow, fmt, pairs in R.bwd_plan(T):
                yield T, H, ddt, vdt, narrow, fmt, pairs


def sides(ref, tol, pairs):
    return [(ref, tol)] * ("row" in pairs) + [(ref.t(), tol.t())] * ("col" in pairs)


@pytest.mark.parametrize("act", R.ACTS)
def test_cpu_backward_quantizer_agrees_with_float64_codes(act):
    for T, H, ddt, vdt, narrow, fmt, pairs in bwd_cases():
        if (ddt, vdt) != R.BWD_DTYPES[1] or T == 144:
            continue
        dh, v = R.bwd_inputs(T, H, ddt, vdt, narrow)
        ref, tol = R.dv64(dh, v, act)
        rc, rs, cc, cs = mx_glu_backward_quantize(dh, v, act=act, row_fmt=fmt, col_fmt=fmt)
        if "row" in pairs:
            R.codes_agree(rc, rs, fmt, ref, tol, what=f"cpu backward row {act} {(T, H)}")
        if "col" in pairs:
            R.codes_agree(cc, cs, fmt, ref.t(), tol.t(), what=f"cpu backward col {act} {(T, H)}")


# ---- the caps are a condition ---------------------------------------------------------------------------------------------------------
def test_every_input_set_stays_within_the_exemption_caps():
    """from the reference alone, no kernel and no CPU path: each input set of tests/test_mx_glu_f64_gpu.py, with each format and pair
    it is used with, exempts at most CAP of its elements and of its blocks.  E5M2, and the col pair where a block along T holds one
    element, meet it only with the narrowed gates (mx_glu_ref.bwd_inputs says why): both are asserted to miss it with the wide ones"""
    worst = 0.0
    for act in R.ACTS:
        for T, H, ddt, vdt, narrow, fmt, pairs in bwd_cases():
            dh, v = R.bwd_inputs(T, H, ddt, vdt, narrow)
            for r, t in sides(*R.dv64(dh, v, act), pairs):
                shares = R.exempt_shares(fmt, r, t)
                worst = max(worst, *shares)
                assert max(shares) <= R.CAP, (act, T, H, ddt, vdt, fmt, pairs, shares)
        cases = [fwd_reference(M, H, K)[1] for M, H, K in R.FWD_SHAPES] + [fwd_reference(*GROUPED[:4], GROUPED[4])[1]]
        for v64 in cases:
            for fmt in R.FWD_FMTS:
                shares = R.exempt_shares(fmt, R.glu64(v64, act), R.glu_bound(v64, act, torch.float32))
                worst = max(worst, *shares)
                assert max(shares) <= R.CAP, (act, tuple(v64.shape), fmt, shares)
    print(f"largest exempt share of any case: {worst:.4%}")
    # the narrowing is needed, not a convenience: the wide gates miss the cap for E5M2, and for a one-element block in any format
    dh, v = R.bwd_inputs(144, 96)
    assert R.exempt_shares("mxfp8_e5m2", *R.dv64(dh, v, "gelu"))[0] > R.CAP
    for T, H in ((33, 32), (1, 32)):
        ref, tol = R.dv64(*R.bwd_inputs(T, H), "gelu")
        assert all(max(R.exempt_shares(f, ref.t(), tol.t())) > R.CAP for f in R.FWD_FMTS), (T, H)


# ---- the bound does not hide a wrong kernel -------------------------------------------------------------------------------------------
# (mutation, act, reaches z, reaches dv)
MUTATIONS = [("tanh", "gelu", True, True), ("no_term", "silu", False, True), ("beta", "gelu", False, True), ("swap", "silu", True, True),
             ("swap", "gelu", True, True), ("expf", "silu", True, True), ("expf", "gelu", False, True)]
TILE_R, TILE_C = 128, 64


def every_tile(mask):
    R_, C_ = mask.shape
    assert R_ % TILE_R == 0 and C_ % TILE_C == 0
    return bool(mask.reshape(R_ // TILE_R, TILE_R, C_ // TILE_C, TILE_C).any(3).any(1).all())


def wrong_elements(codes, scales, fmt, ref, tol):
    m = R.codes_compare(codes, scales, fmt, ref, tol)
    return m["wrong"].reshape(ref.shape[0], -1)[:, :ref.shape[1]]


@pytest.mark.parametrize("mutation,act,in_z,in_dv", [(None, a, False, False) for a in R.ACTS] + MUTATIONS)
def test_the_bounds_do_not_hide_a_wrong_kernel(mutation, act, in_z, in_dv):
    """a mutated float32 evaluation stands in for a wrong kernel: wherever the mutation reaches, every tile of 128 x 64 of the float
    output holds a value outside glu_bound / dv_bound, and every such tile of the E2M3 and E4M3 codes, along either axis, a non-exempt
    mismatch.  The unmutated evaluation passes all of it"""
    T, H = 256, 64
    gen = torch.Generator().manual_seed(77)
    sign = lambda: torch.where(torch.rand(T, H, generator=gen) < 0.5, -1.0, 1.0)
    g = torch.rand(T, H, generator=gen) * 6 - 3          # where both functions bend
    # up and dh of one binade: the elements of a block are of one size, so the three mantissa bits of both formats resolve them
    dh, v = sign() * (1 + torch.rand(T, H, generator=gen)), R.interleave(g, sign() * (1 + torch.rand(T, H, generator=gen)))
    z, dv = f32_glu(dh, v, act, mutation)
    z64, zb = R.glu64(v, act), R.glu_bound(v, act, torch.float32)
    dv64, db = R.dv64(dh, v, act)
    for name, got, ref, tol, reached in (("z", z, z64, zb, in_z), ("dv", dv, dv64, db, in_dv)):
        outside = (got.double() - ref).abs() > tol
        print(mutation, act, name, "outside the bound:", int(outside.sum()), "of", outside.numel())
        assert every_tile(outside) if reached else not bool(outside.any()), (name, "float")
        for fmt in ("mxfp6_e2m3", "mxfp8_e4m3"):
            if name == "z":
                _, codes, scales = quantize_with_mx(got, fmt, -1, return_codes=True)
                wrong = [wrong_elements(codes, scales, fmt, ref, tol)]
            else:
                rc, rs, cc, cs = mx_quantize_2way(got, fmt, fmt)
                wrong = [wrong_elements(rc, rs, fmt, ref, tol), wrong_elements(cc, cs, fmt, ref.t(), tol.t()).t()]
            for w in wrong:
                print(mutation, act, name, fmt, "non-exempt mismatches:", int(w.sum()))
                assert every_tile(w) if reached else not bool(w.any()), (name, fmt)


# ---- one training step on two devices -------------------------------------------------------------------------------------------------
def linear_case(act):
    """x [33, 40], W [64, 40] (H = 32), bias, dh, and the codes both devices share; the formats are mx_glu_linear's defaults"""
    gen = torch.Generator().manual_seed(5 + len(act))
    x, w = torch.randn(33, 40, generator=gen), torch.randn(64, 40, generator=gen) / 40 ** 0.5
    bias, dh = torch.randn(64, generator=gen) / 4, torch.randn(33, 32, generator=gen)
    fmts = ("mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2")
    return x, w, bias, dh, fmts, mx_quantize_2way(x, fmts[0], fmts[0]), mx_quantize_2way(w, fmts[1], fmts[1])


def cpu_step(x, w, bias, dh, act):
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = mx_glu_linear(x, w, bias, act=act)
    y.backward(dh)
    return y.detach(), x.grad, w.grad


@pytest.mark.parametrize("act,mutation", [("silu", "no_term"), ("gelu", "beta")])
def test_linear_step_bounds_hold_for_an_emulated_device_and_catch_a_wrong_one(act, mutation):
    """mx_glu_ref.linear_step_bounds without a GPU: device A is mx_gemm_ref.model_emulate (the instruction's measured accumulation, in
    float64) for the three products with the float32 epilogue of f32_glu and the CPU quantizer between them, device B the CPU path of
    ``mx_glu_linear``.  A stays inside the bounds; with a mutated derivative in front of its quantizer dx and dw leave them"""
    x, w, bias, dh, fmts, xq, wq = linear_case(act)
    fx, fw, fg = fmts
    y_b, dx_b, dw_b = cpu_step(x, w, bias, dh, act)
    v_b = mx_matmul(xq[0], xq[1], fx, wq[0], wq[1], fw, bias)
    v_a = G.model_emulate(xq[0], xq[1], fx, wq[0], wq[1], fw, bias).float()
    assert not torch.equal(v_a, v_b) and float(R.deinterleave(v_b)[0].abs().max()) <= 8

    def device_a(mut):
        z, dv = f32_glu(dh, v_a, act, mut)
        codes = mx_quantize_2way(dv, fg, fg)
        return z, G.model_emulate(codes[0], codes[1], fg, wq[2], wq[3], fw).float(), G.model_emulate(codes[2], codes[3], fg, xq[2], xq[3], fx).float(), codes

    y_a, dx_a, dw_a, codes = device_a(None)
    bounds = R.linear_step_bounds(xq, wq, fmts, bias, dh, act, v_a, v_b, codes)
    for name, a, b, B in zip(("y", "dx", "dw"), (y_a, dx_a, dw_a), (y_b, dx_b, dw_b), bounds):
        err = (a.double() - b.double()).abs()
        print(f"{act} {name}: max err / bound = {float((err / B.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= B).all()), name
    _, dx_m, dw_m, codes_m = device_a(mutation)
    bounds = R.linear_step_bounds(xq, wq, fmts, bias, dh, act, v_a, v_b, codes_m)
    assert bool(((dx_m.double() - dx_b.double()).abs() > bounds[1]).any()) and bool(((dw_m.double() - dw_b.double()).abs() > bounds[2]).any())
