"""``mx_norm_backward`` on the CPU: against the definition restated in ``mx_norm_bwd_ref.py`` bit for bit, against float64 within the
margins of ``mx_norm_ref.norm_backward_margins``, special values, ``mx_norm_linear(norm_backward="fused")`` / ``MXTrainNormLinear`` and
the C ABI's checks (no GPU needed: everything refused is refused before a launch).  The GPU twins are in ``test_mx_norm_bwd_gpu.py``;
the checks that run on both are written once, on a device argument, and imported there."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn as nn

import mx_norm_bwd_ref as BR
import mx_norm_ref as NR
import qsparse_amd as qs
import test_mx_norm as T
from mx_norm_ref import DTS, EPS, NORMS, norm_backward_margins, norm_backward_ref, same
from qsparse_amd import MXTrainNormLinear, _hip, mx_linear, mx_norm_backward, mx_norm_linear, mx_norm_quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dx", "dweight", "dbias")


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def to(dev, ts):
    return [t if t is None else t.to(dev) for t in ts]


def run(dev, case, norm, **kw):
    """mx_norm_backward of a case of mx_norm_bwd_ref on `dev`, results back on the CPU"""
    dxhat, x, rstd, mean, w = to(dev, case)
    return to("cpu", mx_norm_backward(dxhat, x, rstd, mean, w, norm=norm, **kw))


def rounded(ref, dtype):
    """the reference's (float32 dx, dweight, dbias) as the function returns them: dx rounded once to x's dtype"""
    return (ref[0].to(dtype), ref[1], ref[2])


# ---- test 1: the CPU path against the definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_cpu_path_is_the_definition(norm, dtype):
    for R, C in BR.SHAPES:
        for has_w in (True, False):
            got = run("cpu", BR.case(R, C, dtype, norm, has_w), norm)
            want = rounded(BR.reference(R, C, dtype, norm, has_w), dtype)
            for name, a, r in zip(NAMES, got, want):
                assert same(a, r), (name, R, C, has_w)


def test_order_differs_from_torchs_and_is_a_function_of_the_shape():
    """the fixed order is not torch's: at a shape with more than one tile and pass the last bits differ from .sum(0) / .mean(-1); and
    the column sum of a row tile does not depend on the columns around it"""
    R, C = 300, 520
    case = BR.case(R, C, torch.float32, "layer")
    dx, dw, db = run("cpu", case, "layer")
    tdx, tdw, tdb = norm_backward_ref(*case, "layer")
    assert not same(dx, tdx) and not same(dw, tdw) and not same(db, tdb)
    dxhat, x, rstd, mean, w = case
    part = mx_norm_backward(dxhat[:, 64:100].contiguous(), x[:, 64:100].contiguous(), rstd, mean, None, norm="layer", need_dx=False)
    assert part[0] is None and same(part[2], db[64:100])


def test_leading_dimensions_and_needs():
    dxhat, x, rstd, mean, w = BR.case(300, 520, torch.bfloat16, "layer")
    flat = mx_norm_backward(dxhat, x, rstd, mean, w, norm="layer")
    lead = mx_norm_backward(dxhat.view(3, 100, 520), x.view(3, 100, 520), rstd.view(3, 100), mean.view(3, 100), w, norm="layer")
    assert lead[0].shape == (3, 100, 520) and lead[0].dtype == torch.bfloat16 and lead[1].shape == lead[2].shape == (520,)
    assert all(same(a.reshape(r.shape), r) for a, r in zip(lead, flat))
    check_every_subset("cpu", (300, 520, torch.bfloat16, "layer"))
    empty = mx_norm_backward(torch.zeros(0, 40), torch.zeros(0, 40), torch.zeros(0), None, None)
    assert empty[0].shape == (0, 40) and same(empty[1], torch.zeros(40)) and same(empty[2], torch.zeros(40))


def check_every_subset(dev, key):
    """every subset of need_*: what is not asked for is None, what is asked for does not change with the subset"""
    case = BR.case(*key)
    full = run(dev, case, key[3])
    for bits in range(8):
        needs = [bool(bits & 1), bool(bits & 2), bool(bits & 4)]
        got = run(dev, case, key[3], need_dx=needs[0], need_dweight=needs[1], need_dbias=needs[2])
        for name, need, a, r in zip(NAMES, needs, got, full):
            assert (a is None) == (not need), (name, bits)
            assert a is None or same(a, r), (name, bits)


def test_refusals():
    dxhat, x, rstd, mean, w = BR.case(129, 96, torch.float32, "layer")
    with pytest.raises(ValueError, match="unknown norm"):
        mx_norm_backward(dxhat, x, rstd, mean, w, norm="batch")
    with pytest.raises(ValueError, match="needs mean"):
        mx_norm_backward(dxhat, x, rstd, None, w, norm="layer")
    with pytest.raises(ValueError, match="dxhat has shape"):
        mx_norm_backward(dxhat[:, :64], x, rstd, mean, w, norm="layer")
    with pytest.raises(ValueError, match="rstd has shape"):
        mx_norm_backward(dxhat, x, rstd[:-1], mean, w, norm="layer")
    with pytest.raises(TypeError, match="rstd must be float32"):
        mx_norm_backward(dxhat, x, rstd.double(), mean, w, norm="layer")
    with pytest.raises(TypeError, match="dxhat must be one of"):
        mx_norm_backward(dxhat.double(), x, rstd, mean, w, norm="layer")
    with pytest.raises(ValueError, match="expected \\(96,\\)"):
        mx_norm_backward(dxhat, x, rstd, mean, w[:-1], norm="layer")
    with pytest.raises(ValueError, match="x is on cpu but rstd on meta"):
        mx_norm_backward(dxhat, x, rstd.to("meta"), mean, w, norm="layer")
    with pytest.raises(ValueError, match="unknown norm_backward"):
        mx_norm_linear(x, None, None, torch.randn(8, 96), norm_backward="aten")
    with pytest.raises(ValueError, match="unknown norm_backward"):
        MXTrainNormLinear(96, 8, norm_backward="hip")
    with pytest.raises(ValueError, match="unknown norm_backward"):
        MXTrainNormLinear.from_float(nn.RMSNorm(96), nn.Linear(96, 8), norm_backward=None)


# ---- test 2: against float64 ---------------------------------------------------------------------------------------------------------
def check_against_float64(dev):
    """|result - float64| <= norm_backward_margins, the bound of DESIGN.md 3r that holds for ANY order of the sums.  The margin of dx
    bounds the float32 value in front of its one rounding to x's dtype: with a float32 x that is the function's dx itself; with a
    two-byte x the bound is checked on the reference's float32 dx and the function's dx is that value rounded once, bit for bit.
    The column sums are float32 throughout.  Worst error / margin, the same on the CPU and on the GPU: dx 0.32, dweight 0.14,
    dbias 0.01 (printed)"""
    worst = {"dx": 0.0, "dweight": 0.0, "dbias": 0.0}
    for norm in NORMS:
        for R, C in BR.SHAPES:
            for dtype in DTS:
                case = BR.case(R, C, dtype, norm)
                got = run(dev, case, norm)
                if dtype != torch.float32:
                    ref = BR.reference(R, C, dtype, norm)
                    assert same(got[0], ref[0].to(dtype)), (norm, R, C, dtype)
                    got = (ref[0],) + tuple(got[1:])
                want = norm_backward_ref(*case, norm, torch.float64)
                margins = norm_backward_margins(*case, norm)
                for name, a, r, m in zip(NAMES, got, want, margins):
                    err = (a.double() - r).abs()
                    worst[name] = max(worst[name], float((err / m.clamp_min(1e-300)).max()))
                    assert bool((err <= m).all()), (name, norm, R, C, dtype, float((err / m.clamp_min(1e-300)).max()))
    print(f"{dev}: worst error / margin: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_against_float64_cpu():
    check_against_float64("cpu")


# ---- test 4: special values ------------------------------------------------------------------------------------------------------------
def special_case(dtype, norm, R=140, C=96):
    """a NaN row and an Inf row of x (their rstd is NaN, as the forward writes it), the other rows as usual"""
    dxhat, x, _, _, w = BR.case(R, C, dtype, norm)
    x = x.clone()
    x[5, 40] = float("nan")
    x[133, 70] = float("inf")
    rstd, mean = mx_norm_quantize(x, w, norm=norm, eps=EPS, return_stats=True)[-2:]
    return dxhat, x, rstd, mean, w


def check_special_values(dev, dtype, norm):
    case = special_case(dtype, norm)
    dx, dw, db = run(dev, case, norm)
    bad = torch.zeros(140, dtype=torch.bool)
    bad[5] = bad[133] = True
    assert bool(dx[bad].isnan().all()) and bool(dw.isnan().all()) and bool(db.isfinite().all())
    clean = BR.case(140, 96, dtype, norm)
    assert same(dx[~bad], run(dev, clean, norm)[0][~bad])                   # the other rows are untouched
    want = rounded(BR.ref_backward(*case), dtype)
    assert all(same(a, r) for a, r in zip((dx, dw, db), want))
    zero = (torch.zeros_like(clean[0]),) + tuple(clean[1:])
    for a in run(dev, zero, norm):
        assert bool((a == 0).all())


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("dtype", DTS, ids=str)
def test_special_values_cpu(dtype, norm):
    check_special_values("cpu", dtype, norm)


def f16_max_case(norm, R=40, C=128):
    dxhat, x, _, _, w = BR.case(R, C, torch.float16, norm)
    x = x.clone()
    x[3] = 65504.0
    x[4, ::2] = 65504.0
    x[4, 1::2] = -65504.0
    rstd, mean = mx_norm_quantize(x, w, norm=norm, eps=EPS, return_stats=True)[-2:]
    return dxhat, x, rstd, mean, w


@pytest.mark.parametrize("norm", NORMS)
def test_f16_row_of_65504_cpu(norm):
    case = f16_max_case(norm)
    got = run("cpu", case, norm)
    assert all(same(a, r) for a, r in zip(got, rounded(BR.ref_backward(*case), torch.float16)))
    assert bool(got[0].isfinite().all()) and bool(got[1].isfinite().all())


# ---- test 5: mx_norm_linear(norm_backward="fused") ---------------------------------------------------------------------------------------
def check_fused_norm_linear(dev, shape, N, norm):
    """out, dW, db are "torch"'s bit for bit; dx, d norm_weight, d norm_bias are mx_norm_backward on mx_linear's float32 input gradient,
    bit for bit, and within the margins of float64"""
    x, nw, nb, W, b, dy = T._train_case(dev, shape, N, norm, 6)
    K = shape[-1]
    res = {}
    for mode in ("torch", "fused"):
        leaves = [t.clone().requires_grad_(True) for t in (x, nw, W, b)] + [None if nb is None else nb.clone().requires_grad_(True)]
        xg, nwg, Wg, bg, nbg = leaves
        out = mx_norm_linear(xg, nwg, nbg, Wg, bg, norm=norm, eps=EPS, norm_backward=mode)
        out.backward(dy)
        res[mode] = (out.detach(), Wg.grad, bg.grad, xg.grad, nwg.grad, None if nbg is None else nbg.grad)
    assert all(same(a, r) for a, r in zip(res["fused"][:3], res["torch"][:3]))

    y = NR.ref_y(x.reshape(-1, K).cpu(), nw.cpu(), None if nb is None else nb.cpu(), norm)[0].to(dev)
    yr = y.reshape(shape).requires_grad_(True)
    mx_linear(yr, W.clone().requires_grad_(True), b.clone().requires_grad_(True)).backward(dy)
    dxhat = yr.grad.reshape(-1, K)                                        # mx_linear's input gradient, float32
    x2 = x.reshape(-1, K)
    rstd, mean = mx_norm_quantize(x2, nw, nb, norm=norm, eps=EPS, return_stats=True)[-2:]
    dx, dw, db = mx_norm_backward(dxhat, x2, rstd, mean, nw, norm=norm)
    got = res["fused"][3:]
    assert same(got[0], dx.reshape(shape)) and same(got[1], dw) and (nb is None or same(got[2], db))
    want = norm_backward_ref(dxhat, x2, rstd, mean, nw, norm, torch.float64)
    margins = norm_backward_margins(dxhat, x2, rstd, mean, nw, norm)
    for name, a, r, m in zip(NAMES, (dx, dw, db), want, margins):
        err = (a.double() - r).abs()
        print(f"{norm} {shape}: {name} worst error / margin = {float((err / m.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= m).all()), name


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape,N", [((2, 33, 96), 64), ((129, 128), 32)])
def test_fused_norm_linear_cpu(shape, N, norm):
    check_fused_norm_linear("cpu", shape, N, norm)


def check_needs_reach_the_call(dev, monkeypatch):
    """the need_* flags of the fused backward are needs_input_grad's; nobody asking for a norm gradient means no call"""
    import qsparse_amd.mx_norm as M
    x, nw, nb, W, b, dy = T._train_case(dev, (40, 64), 32, "layer", 7)
    calls = []
    real = M.mx_norm_backward
    monkeypatch.setattr(M, "mx_norm_backward",
                        lambda *a, **k: calls.append((k["need_dx"], k["need_dweight"], k["need_dbias"])) or real(*a, **k))
    for req in ((True, False, False), (False, True, False), (False, False, True), (True, True, True), (False, False, False)):
        xg, nwg, nbg = [t.clone().requires_grad_(r) for t, r in zip((x, nw, nb), req)]
        Wg = W.clone().requires_grad_(True)
        mx_norm_linear(xg, nwg, nbg, Wg, b, norm="layer", norm_backward="fused").backward(dy)
        assert [t.grad is not None for t in (xg, nwg, nbg)] == list(req) and Wg.grad is not None
    assert calls == [(True, False, False), (False, True, False), (False, False, True), (True, True, True)]
    del calls[:]
    mx_norm_linear(x.clone().requires_grad_(True), nw, nb, W, b, norm="layer").backward(dy)          # the default does not call it
    assert calls == []


def test_needs_reach_the_call_cpu(monkeypatch):
    check_needs_reach_the_call("cpu", monkeypatch)


def check_fused_layer(dev):
    """MXTrainNormLinear.from_float(..., norm_backward="fused") for the four norm modules of check_layer: the functional's gradients"""
    torch.manual_seed(8)
    for fnorm in (nn.RMSNorm(96, eps=1e-5), nn.LayerNorm(96), nn.LayerNorm(96, bias=False), nn.RMSNorm(96, elementwise_affine=False)):
        fnorm, lin = fnorm.to(dev), nn.Linear(96, 64).to(dev)
        for p in fnorm.parameters():
            nn.init.normal_(p, 1.0, 0.25)
        layer = MXTrainNormLinear.from_float(fnorm, lin, norm_backward="fused")
        assert layer.norm_backward == "fused" and "norm_backward='fused'" in repr(layer)
        assert "norm_backward" not in repr(MXTrainNormLinear.from_float(fnorm, lin))
        x, dy = torch.randn(2, 33, 96).to(dev), torch.randn(2, 33, 64).to(dev)
        xg = x.clone().requires_grad_(True)
        layer(xg).backward(dy)
        got = [xg.grad] + [p.grad.clone() for p in layer.parameters()]
        for p in layer.parameters():
            p.grad = None
        xr = x.clone().requires_grad_(True)
        eps = float(torch.finfo(x.dtype).eps) if layer.eps is None else layer.eps          # (nn.RMSNorm's rule for eps=None)
        mx_norm_linear(xr, layer.norm_weight, layer.norm_bias, layer.weight, layer.bias, norm=layer.norm, eps=eps,
                       norm_backward="fused").backward(dy)
        want = [xr.grad] + [p.grad for p in layer.parameters()]
        assert len(got) == len(want) and all(same(a, r) for a, r in zip(got, want))


def test_fused_layer_cpu():
    check_fused_layer("cpu")


# ---- test 7: the C ABI without a GPU ---------------------------------------------------------------------------------------------------
def _args(**kw):
    a = _hip.MxNormBwdArgs()
    a.struct_size = ctypes.sizeof(a)
    a.mode, a.xdt, a.gdt = 1, _hip.F32, _hip.F32
    a.dxhat, a.x, a.weight, a.rstd, a.mean = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.dx, a.dweight, a.dbias = 0x6000, 0x7000, 0x8000
    a.workspace, a.workspace_bytes = 0x10000, 1 << 40
    a.R, a.C = 129, 96
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_descriptor_checks_in_the_documented_order():
    """QS_ERR_ARG (-2) before QS_ERR_DTYPE (-1) before QS_ERR_ALIGN (-3) before QS_ERR_WORKSPACE (-4); the route of what is accepted.
    Only the route export is called on descriptors that would launch: nothing is enqueued here"""
    lib = _hip.load()
    route = lambda a: lib.qs_mx_norm_bwd_route(ctypes.byref(a))
    assert lib.qs_mx_norm_bwd_v(None) == -2 and lib.qs_mx_norm_bwd_route(None) == -2
    short = _args(struct_size=2)
    assert lib.qs_mx_norm_bwd_v(ctypes.byref(short)) == -2 and route(short) == -2
    assert route(_args()) == _hip.MX_NORM_BWD_ROUTE_VEC
    for bad in (dict(mode=2), dict(dxhat=None), dict(x=None), dict(rstd=None), dict(mean=None), dict(dx=None, dweight=None, dbias=None),
                dict(R=-1), dict(C=-1)):
        a = _args(xdt=7, workspace=None, **bad)                     # a later failure as well: the earlier check answers
        assert route(a) == -2 and lib.qs_mx_norm_bwd_v(ctypes.byref(a)) == -2, bad
    assert route(_args(mode=0, mean=None)) == _hip.MX_NORM_BWD_ROUTE_VEC                # rms mode does not look at mean
    for bad in (dict(xdt=7), dict(gdt=-1)):
        a = _args(x=0x2001, workspace_bytes=0, **bad)
        assert route(a) == -1 and lib.qs_mx_norm_bwd_v(ctypes.byref(a)) == -1, bad
    for bad in (dict(x=0x2002), dict(dx=0x6002), dict(dxhat=0x1002), dict(weight=0x3002), dict(rstd=0x4001), dict(mean=0x5002),
                dict(dweight=0x7002), dict(dbias=0x8003), dict(workspace=0x10008), dict(xdt=_hip.BF16, x=0x2001),
                dict(gdt=_hip.F16, dxhat=0x1001)):
        a = _args(workspace_bytes=0, **bad)
        assert route(a) == -3 and lib.qs_mx_norm_bwd_v(ctypes.byref(a)) == -3, bad
    assert route(_args(xdt=_hip.BF16, x=0x2002, dx=0x6002)) == _hip.MX_NORM_BWD_ROUTE_PLAIN      # element-aligned: accepted, PLAIN
    assert route(_args(weight=0x3004)) == _hip.MX_NORM_BWD_ROUTE_PLAIN and route(_args(C=100)) == _hip.MX_NORM_BWD_ROUTE_PLAIN
    assert route(_args(weight=None)) == _hip.MX_NORM_BWD_ROUTE_VEC
    assert route(_args(R=1 << 40, C=1 << 40)) == -2                                     # R * C beyond 64 bits
    # an empty tensor: accepted, nothing to do, no workspace needed
    for empty in (dict(R=0), dict(C=0)):
        a = _args(workspace=None, workspace_bytes=0, **empty)
        assert route(a) == 0 and lib.qs_mx_norm_bwd_v(ctypes.byref(a)) == 0
    need = _hip.mx_norm_bwd_plan(129, 96, "layer", True, True)
    for bad in (dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace_bytes=0)):
        a = _args(**bad)
        assert route(a) == -4 and lib.qs_mx_norm_bwd_v(ctypes.byref(a)) == -4, bad
    assert route(_args(workspace_bytes=need)) == _hip.MX_NORM_BWD_ROUTE_VEC
    only_dx = _hip.mx_norm_bwd_plan(129, 96, "layer", True, False)
    assert route(_args(dweight=None, dbias=None, workspace_bytes=only_dx)) == _hip.MX_NORM_BWD_ROUTE_VEC
    assert route(_args(dweight=None, workspace_bytes=only_dx)) == -4                     # dbias alone needs the partial sums too


def test_plan_matches_the_layout():
    """up16(4 R) for c1, once more for c2 in layer mode, with dx; 2 up16(4 ceil(R / 128) C) with a column sum; 0 for an empty tensor"""
    up16 = lambda n: (n + 15) // 16 * 16
    for R, C in BR.SHAPES + ((8192, 4096), (50432, 768)):
        T_ = (R + 127) // 128
        for norm in NORMS:
            for need_dx in (False, True):
                for need_cols in (False, True):
                    want = need_dx * up16(4 * R) * (2 if norm == "layer" else 1) + need_cols * 2 * up16(4 * T_ * C)
                    assert _hip.mx_norm_bwd_plan(R, C, norm, need_dx, need_cols) == want, (R, C, norm, need_dx, need_cols)
    assert _hip.mx_norm_bwd_plan(0, 96, "rms", True, True) == 0 and _hip.mx_norm_bwd_plan(96, 0, "layer", True, True) == 0
    lib = _hip.load()
    n = ctypes.c_uint64(0)
    assert lib.qs_mx_norm_bwd_plan(-1, 4, 0, 1, 1, ctypes.byref(n)) == -2 and lib.qs_mx_norm_bwd_plan(4, 4, 2, 1, 1, ctypes.byref(n)) == -2
    assert lib.qs_mx_norm_bwd_plan(4, 4, 0, 1, 1, None) == -2 and lib.qs_mx_norm_bwd_plan(1 << 40, 1 << 40, 0, 1, 1, ctypes.byref(n)) == -2


def test_descriptor_struct_has_the_headers_layout(tmp_path):
    """the ctypes mirror of qs_mx_norm_bwd_args against `sizeof` / `offsetof` of the header itself (gcc: the header is plain C)"""
    ct, cname = _hip.MxNormBwdArgs, "qs_mx_norm_bwd_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "qsparse_hip.h")}"', 'int main(void) {',
             f'printf("%zu", sizeof({cname}));']
    lines += [f'printf(" %zu", offsetof({cname}, {fname}));' for fname, _ in ct._fields_]
    lines += ['printf("\\n");', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    size, *offsets = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(ct)
    assert [int(o) for o in offsets] == [getattr(ct, f).offset for f, _ in ct._fields_]
    assert ct._fields_[0][0] == "struct_size"
