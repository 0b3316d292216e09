"""The gated (GLU) MX kernels on the GPU against float64 (tests/mx_glu_ref.py): no ATen ``silu`` / ``gelu`` anywhere.  The float outputs
of ``mx_glu_matmul`` / ``mx_grouped_glu_matmul`` stay inside ``glu_bound`` of ``act64(g) * u`` on the kernel's own pre-activations
(which are asserted to be ``mx_matmul``'s bit for bit, and, the operands being of the exact class, the float64 product itself);
the emitted codes are the quantizer's codes of the kernel's own float32 output and pass ``codes_agree`` against the float64 value;
``mx_glu_backward_quantize`` passes ``codes_agree`` against the float64 ``dv`` both ways; one ``mx_glu_linear`` step agrees with the
CPU's under ``linear_step_bounds``.  The input sets are mx_glu_ref's, whose
exemption caps tests/test_mx_glu_f64.py asserts from the reference alone.  ``pytest -s`` prints max(err / bound) and the exempt
shares."""
import pytest
import torch

import mx_gemm_ref as G
import mx_glu_ref as R
import qsparse_amd as qs
from qsparse_amd import (_hip, mx_glu_backward_quantize, mx_glu_linear, mx_glu_matmul, mx_grouped_glu_matmul, mx_grouped_matmul, mx_matmul,
                         mx_quantize_2way, quantize_with_mx)
from test_mx_glu_gpu import BAD_ROWS, ROWS, special_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = (torch.float32, torch.bfloat16, torch.float16)
GATED = ("silu", "gelu")
GEMM_VEC, GEMM_PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN
Q2_VEC, Q2_PLAIN = _hip.MX_Q2_ROUTE_TILE_VEC, _hip.MX_Q2_ROUTE_TILE_PLAIN
GROUPED = (70, 32, 40, 3, [33, 33, 70])          # T, H, K, E, ends: an empty group and a ragged last one


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def dense_args(M, H, K):
    ops = R.fwd_operands(M, H, K)
    v64 = G.reference(ops[0], ops[1], R.FA, ops[2], ops[3], R.FB, ops[4])[1]
    dev = tuple(t.to(DEV) for t in ops)
    return (dev[0], dev[1], R.FA, dev[2], dev[3], R.FB, dev[4]), v64


def grouped_args():
    T, H, K, E, ends = GROUPED
    ops = R.fwd_operands(T, H, K, E)
    v64 = torch.zeros(T, 2 * H, dtype=torch.float64)
    for e, (lo, hi) in enumerate(zip([0] + ends[:-1], ends)):
        if hi > lo:
            v64[lo:hi] = G.reference(ops[0][lo:hi], ops[1][lo:hi], R.FA, ops[2][e], ops[3][e], R.FB, ops[4][e])[1]
    dev = tuple(t.to(DEV) for t in ops)
    return (dev[0], dev[1], R.FA, dev[2], dev[3], R.FB, torch.tensor(ends, dtype=torch.int32, device=DEV), dev[4]), v64


def check_float(y, v, act, dt, what):
    ok, ratio = R.within_glu(y, R.glu64(v, act), R.glu_bound(v, act, dt), dt)
    print(f"{what} {act} {dt}: max err / bound = {ratio:.3f}")
    assert ok, (what, act, dt, ratio)
    return ratio


def check_codes(call, v, act, what, fmts=R.FWD_FMTS, against_float64=True):
    """`call(out_fmt=...)`: the codes are the quantizer's of the kernel's own float32 output, and agree with float64"""
    y32 = call()
    for fmt in fmts:
        codes, scales = call(out_fmt=fmt)
        _, want_c, want_s = quantize_with_mx(y32, fmt, -1, return_codes=True)
        assert torch.equal(codes, want_c) and torch.equal(scales, want_s), (what, act, fmt)
        if against_float64:
            R.codes_agree(codes, scales, fmt, R.glu64(v, act), R.glu_bound(v, act, torch.float32), what=f"{what} {act}")


# ---- forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,K", R.FWD_SHAPES)
@pytest.mark.parametrize("act", GATED)
def test_dense_forward_against_float64(act, M, H, K):
    args, v64 = dense_args(M, H, K)
    g = R.deinterleave(v64)[0]
    assert float((g.abs() <= 3).double().mean()) >= 0.5 and float(g.max()) > 8 and float(g.min()) < -8
    for dt in DTS:
        y, v = mx_glu_matmul(*args, dt, act=act, preact_dtype=torch.float32)
        assert _hip.mx_glu_last_route == (GEMM_VEC if K % 16 == 0 else GEMM_PLAIN)
        assert G.same(v, mx_matmul(*args)) and G.same(v.cpu(), v64.float()), "v is mx_matmul's, and the exact product"
        check_float(y, v, act, dt, f"dense {(M, H, K)}")
    check_codes(lambda **kw: mx_glu_matmul(*args, act=act, **kw), v64, act, f"dense {(M, H, K)}")


@pytest.mark.parametrize("fa", sorted(ROWS))
@pytest.mark.parametrize("act", GATED)
def test_special_rows_against_float64(fa, act):
    """the rows of tests/test_mx_glu_gpu.py: gates of +-0, +-1, +-448 under scales 2^0, 2^7 (silu(-57344) is -0), 2^-20 and 2^100 (a
    product beyond float32: Inf), a zero row, a 0xFF scale byte, NaN / Inf codes.  What is not finite is compared by class"""
    ops = special_case(fa)
    args = (ops[0], ops[1], fa, ops[2], ops[3], "mxfp8_e4m3")
    for dt in DTS:
        y, v = mx_glu_matmul(*args, None, dt, act=act, preact_dtype=torch.float32)
        assert G.same(v, mx_matmul(*args))
        assert not v[list(BAD_ROWS)].isfinite().any() and y[:BAD_ROWS[0]].isinf().any() and torch.signbit(y[y == 0]).any()
        check_float(y, v, act, dt, f"special {fa}")
    check_codes(lambda **kw: mx_glu_matmul(*args, act=act, **kw), None, act, f"special {fa}", fmts=G.FMTS, against_float64=False)


@pytest.mark.parametrize("act", GATED)
def test_grouped_forward_against_float64(act):
    args, v64 = grouped_args()
    for dt in DTS:
        y, v = mx_grouped_glu_matmul(*args, dt, act=act, preact_dtype=torch.float32)
        assert G.same(v, mx_grouped_matmul(*args)) and G.same(v.cpu(), v64.float())
        check_float(y, v, act, dt, "grouped")
    check_codes(lambda **kw: mx_grouped_glu_matmul(*args, act=act, **kw), v64, act, "grouped")


# ---- the backward quantizer --------------------------------------------------------------------------------------------------------
def agree_both_ways(got, fmt, ref, tol, what):
    if got[0] is not None:
        R.codes_agree(got[0], got[1], fmt, ref, tol, what=what + " row")
    if got[2] is not None:
        R.codes_agree(got[2], got[3], fmt, ref.t(), tol.t(), what=what + " col")


@pytest.mark.parametrize("ddt,vdt", R.BWD_DTYPES)
@pytest.mark.parametrize("T,H", R.BWD_SHAPES)
@pytest.mark.parametrize("act", R.ACTS)
def test_backward_quantizer_against_float64(act, T, H, ddt, vdt):
    """every format of mx_glu_ref.bwd_plan on the input set and the pairs it names: both pairs in one launch, then each pair alone"""
    route = Q2_VEC if T % 16 == 0 else Q2_PLAIN
    sets = {}
    for narrow, fmt, pairs in R.bwd_plan(T):
        if narrow not in sets:
            dh, v = R.bwd_inputs(T, H, ddt, vdt, narrow)
            sets[narrow] = (dh.to(DEV), v.to(DEV)) + R.dv64(dh, v, act)
        dh, v, ref, tol = sets[narrow]
        what = f"backward {act} {(T, H)} {ddt} {vdt}"
        both = mx_glu_backward_quantize(dh, v, act=act, row_fmt=fmt, col_fmt=fmt)
        assert _hip.mx_glu_bwd_last_route == route
        row = mx_glu_backward_quantize(dh, v, act=act, row_fmt=fmt)
        assert _hip.mx_glu_bwd_last_route == Q2_VEC and row[2] is None and row[3] is None           # (no col pair: T % 16 does not matter)
        col = mx_glu_backward_quantize(dh, v, act=act, col_fmt=fmt)
        assert _hip.mx_glu_bwd_last_route == route and col[0] is None and col[1] is None
        for got, name in ((both, ""), (row, " alone"), (col, " alone")):
            if "row" in pairs and got[0] is not None:
                R.codes_agree(got[0], got[1], fmt, ref, tol, what=what + name + " row")
            if "col" in pairs and got[2] is not None:
                R.codes_agree(got[2], got[3], fmt, ref.t(), tol.t(), what=what + name + " col")


@pytest.mark.parametrize("act", GATED)
def test_backward_quantizer_a_base_one_element_off(act):
    """the VEC shape with v one float32 element past a 16-byte boundary: PLAIN.  The input set is (144, 96) in (bfloat16, float32), one of
    those whose caps tests/test_mx_glu_f64.py asserts"""
    T, H = 144, 96
    ddt, vdt = R.BWD_DTYPES[1]
    dh, v = R.bwd_inputs(T, H, ddt, vdt)
    ref, tol = R.dv64(dh, v, act)
    raw = torch.empty(T * 2 * H + 1, dtype=vdt, device=DEV)
    v1 = raw[1:].view(T, 2 * H)
    v1.copy_(v)
    assert v1.data_ptr() % 16 == 4
    for fmt in R.FWD_FMTS:
        got = mx_glu_backward_quantize(dh.to(DEV), v1, act=act, row_fmt=fmt, col_fmt=fmt)
        assert _hip.mx_glu_bwd_last_route == Q2_PLAIN
        agree_both_ways(got, fmt, ref, tol, f"backward {act} off by one")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", GATED)
def test_one_mx_glu_linear_step_against_the_cpu(act):
    """x [33, 40] -> H = 32: y, dx and dw of one step on the GPU against the same call on the CPU, under
    mx_glu_ref.linear_step_bounds, whose docstring derives them: the products' model bound, the activation's bounds on either
    device's own pre-activations, and the distance the bound leaves between the two devices' quantized dv.  The GPU's v and dv codes
    that the bound needs come from the public calls the step is made of"""
    gen = torch.Generator().manual_seed(5 + len(act))
    x, w = torch.randn(33, 40, generator=gen), torch.randn(64, 40, generator=gen) / 40 ** 0.5
    bias, dh = torch.randn(64, generator=gen) / 4, torch.randn(33, 32, generator=gen)
    fmts = fx, fw, fg = ("mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2")
    results = {}
    for dev in ("cpu", DEV):
        xl, wl = x.to(dev).clone().requires_grad_(True), w.to(dev).clone().requires_grad_(True)
        y = mx_glu_linear(xl, wl, bias.to(dev), act=act)
        y.backward(dh.to(dev))
        results[dev] = (y.detach().cpu(), xl.grad.cpu(), wl.grad.cpu())
    xq, wq = mx_quantize_2way(x, fx, fx), mx_quantize_2way(w, fw, fw)
    xg, wg = mx_quantize_2way(x.to(DEV), fx, fx), mx_quantize_2way(w.to(DEV), fw, fw)
    assert all(torch.equal(a, b.cpu()) for a, b in zip(xq + wq, xg + wg)), "the operands are the same bits on both devices"
    v_b = mx_matmul(xq[0], xq[1], fx, wq[0], wq[1], fw, bias)
    v_a = mx_glu_matmul(xg[0], xg[1], fx, wg[0], wg[1], fw, bias.to(DEV), act=act, preact_dtype=torch.float32)[1]
    assert float(R.deinterleave(v_b)[0].abs().max()) <= 8
    codes_a = mx_glu_backward_quantize(dh.to(DEV), v_a, act=act, row_fmt=fg, col_fmt=fg)
    bounds = R.linear_step_bounds(xq, wq, fmts, bias, dh, act, v_a.cpu(), v_b, codes_a)
    for name, a, b, B in zip(("y", "dx", "dw"), results[DEV], results["cpu"], bounds):
        err = (a.double() - b.double()).abs()
        print(f"step {act} {name}: max err / bound = {float((err / B.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= B).all()), (act, name)
