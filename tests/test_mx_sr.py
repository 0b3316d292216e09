"""Stochastic rounding of the MX quantizers, CPU side: the Philox known answers, the package's CPU path against the independent
reference tests/mx_sr_ref.py (bit for bit), the properties the definition promises (grid values fixed, the stream and step rules,
unbiasedness), ``mx_linear`` with stochastically rounded gradient operands, and the rounding operands of the two C descriptors
(layout, validation, routes; the v27 struct_size and the v27 alias symbols) -- none of which needs a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import mx_ref as R
import mx_sr_ref as S
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_gemm import MXTrainLinear, mx_linear, mx_matmul, mx_quantize_2way
from qsparse_amd.quantize import _mx_sr_words, _philox4x32_10, quantize_with_mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = list(R.FORMATS)
SHAPES = [((5, 45), -1), ((4, 64), -1), ((3, 40, 5), 1)]
# sizeof(qs_mx_quant_args) / sizeof(qs_mx_quant2_args) as ABI v27 had them: where the fields appended in v28 begin
V27_SIZE_1, V27_SIZE_2 = _hip.MxQuantArgs.rounding.offset, _hip.MxQuant2Args.rounding.offset


def randn(shape, dtype, seed=0, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.exp(torch.randn((shape[0],) + (1,) * (len(shape) - 1), generator=g) * spread)).to(dtype)


def sr(x, fmt, dim=-1, seed=0, step=None, stream=0):
    return quantize_with_mx(x, fmt, dim, True, "stochastic", seed, None if step is None else torch.tensor([step]), stream)


def test_philox_known_answers():
    for ctr, key, out in S.KNOWN_ANSWERS:
        assert tuple(int(v[0]) for v in S.philox(ctr, key)) == out
        t = lambda v: torch.tensor([v], dtype=torch.int64)
        assert tuple(int(v) for v in _philox4x32_10(*[t(c) for c in ctr], key[0], key[1])) == out
    # the words of a tensor: index, stream, key and base as the definition places them, across a carry of the counter's high word
    for seed, step, stream, base in ((0, 0, 0, 0), (5, 2 ** 63, 1, 2 ** 34 - 8), (2 ** 64 - 1, 3, 7, 2 ** 40 + 4)):
        w = _mx_sr_words((3, 7), seed, torch.tensor([step - 2 ** 64 if step >= 2 ** 63 else step]), stream, base)
        assert w.shape == (3, 7) and (w.reshape(-1).numpy().astype(np.uint64) == S.words(21, seed, step, stream, base)).all()


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_cpu_path_equals_the_reference(fmt, dtype):
    for i, (shape, dim) in enumerate(SHAPES):
        x = randn(shape, dtype, seed=i)
        if shape == (4, 64):
            x[0, :32] = 0                                                      # a zero block
            x[1, 3], x[2, 40] = float("nan"), float("inf")                     # a NaN and an Inf block
            x[3, 33], x[3, 35] = -0.0, -1e-6
            if dtype == torch.float32:
                x[0, 32:] = torch.tensor([1e-40, -3e-42] * 16)                 # a block of float32 subnormals
                x[3, :3] = torch.tensor([2e-39, -1e-45, 1.0])                  # ... and subnormals far below a block's grid
        got = sr(x, fmt, dim, seed=7 + i, step=3, stream=i)
        want = S.reference(x, fmt, dim, torch.float32, 7 + i, 3, i)
        assert all(R.same(a, b) for a, b in zip(got, want)), (shape, fmt, dtype)
        if shape == (4, 64):
            y, c, s = got
            assert s[1, 0] == 255 and s[2, 1] == 255 and y[1, :32].isnan().all() and not c[1, :32].any()
            assert s[0, 0] == 0 and not y[0, :32].any()
            assert torch.signbit(y[3, 33]) and y[3, 33] == 0                   # -0.0 stays -0.0
        assert not torch.equal(got[1], quantize_with_mx(x, fmt, dim, True)[1])  # (not the nearest mode's codes)
    with pytest.raises(ValueError, match="unknown rounding"):
        quantize_with_mx(x, fmt, rounding="up")
    with pytest.raises(TypeError, match="one-element int64"):
        quantize_with_mx(x, fmt, rounding="stochastic", step=torch.zeros(1))
    # the backward stays straight-through
    xg = randn((4, 64), torch.float32).requires_grad_(True)
    y = quantize_with_mx(xg, fmt, rounding="stochastic", seed=1)
    gy = torch.randn(4, 64)
    y.backward(gy)
    assert torch.equal(xg.grad, gy)


@pytest.mark.parametrize("fmt", FMTS)
def test_grid_values_are_fixed_points(fmt):
    """every value of the format times a power of two comes back unchanged, whatever the word"""
    g, _ = R.grid(fmt)
    g = g.float()
    g = torch.cat([g, -g, g.new_zeros((-2 * len(g)) % 32)])                    # whole blocks; each holds the largest normal or zeros
    g = g[torch.randperm(len(g), generator=torch.Generator().manual_seed(0))]
    top = R.FORMATS[fmt][4]
    for k in (-20, 0, 9):
        x = (g * 2.0 ** k).reshape(-1, 32)
        x[:, 0] = top * 2.0 ** k                                               # pin every block's scale to 2^k
        for seed in (0, 1, 2 ** 40 + 17):
            y, c, s = sr(x, fmt, -1, seed)
            assert R.same(y, x), (fmt, k, seed)
            assert torch.equal(c, R.reference(x, fmt)[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_way_pairs_are_the_one_way_call_at_streams_0_and_1(dtype):
    for i, shape in enumerate(((33, 31), (64, 96), (70, 45), (1, 33))):
        x = randn(shape, dtype, seed=i)
        fr, fc = FMTS[i], FMTS[(i + 2) % 5]
        step = torch.tensor([i])
        rc, rs, cc, cs = mx_quantize_2way(x, fr, fc, "stochastic", 42, step)
        _, c, s = sr(x, fr, -1, 42, i, 0)
        assert torch.equal(rc, c) and torch.equal(rs, s)
        _, c, s = sr(x.t().contiguous(), fc, -1, 42, i, 1)
        assert torch.equal(cc, c) and torch.equal(cs, s)
        _, c, s = S.reference(x.t().contiguous(), fc, -1, torch.float32, 42, i, 1)
        assert torch.equal(cc, c) and torch.equal(cs, s)
        assert int(step) == i                                                  # the quantizer reads the counter, nothing more
        only = mx_quantize_2way(x, None, fc, "stochastic", 42, step)
        assert only[0] is None and torch.equal(only[2], cc)
    with pytest.raises(ValueError, match="unknown rounding"):
        mx_quantize_2way(x, fr, None, "random")
    assert torch.equal(mx_quantize_2way(x, fr, fc, "nearest", 5)[2], mx_quantize_2way(x, fr, fc)[2])


def test_step_is_added_to_the_seed():
    x = randn((8, 64), torch.float32)
    for fmt in ("mxfp4_e2m1", "mxfp8_e4m3"):
        a = sr(x, fmt, -1, seed=100, step=23)
        assert all(torch.equal(p, q) for p, q in zip(a, sr(x, fmt, -1, seed=123)))
        assert all(torch.equal(p, q) for p, q in zip(a, sr(x, fmt, -1, seed=2 ** 64 + 122, step=1)))        # mod 2^64
        assert all(torch.equal(p, q) for p, q in zip(sr(x, fmt, -1, seed=5, step=-5), sr(x, fmt, -1, seed=0)))
        b = sr(x, fmt, -1, seed=100, step=24)
        assert not torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])         # other codes, the same scales
        assert not torch.equal(a[1], sr(x, fmt, -1, seed=100, step=23, stream=1)[1])


@pytest.mark.parametrize("fmt", FMTS)
def test_mean_over_steps_is_unbiased_where_nearest_rounding_is_not(fmt):
    """2048 elements, S = 256 steps.  Each y_t - x is a two-point variable on a grid step d with mean zero: variance at most d^2 / 4,
    so the mean over S independent steps has standard deviation at most d / (2 sqrt(S)).  Bound: six of those, for every element that
    is not clamped (above the largest normal the error is the clamp's).  Nearest rounding, whose error is the same at every step,
    must break that bound on the same input -- which is what shows that this test can fail.

    Largest |mean - x| in units of d / (2 sqrt(S)) over the five formats when this was written: 2.8 - 4.4 (nearest mode: 16.0)."""
    ebits, mbits, bias, emax, top = R.FORMATS[fmt]
    x = randn((64, 32), torch.float32, seed=5)
    S_ = 256
    acc = torch.zeros(x.shape, dtype=torch.float64)
    for t in range(S_):
        y, c, s = sr(x, fmt, -1, seed=2024, step=t)
        acc += y.double()
    X = R.expand_scale(s, 32, 1)
    v = x.double() / X
    ex = torch.frexp(v.abs().clamp(min=2.0 ** -300))[1] - 1
    d = torch.pow(torch.tensor(2.0, dtype=torch.float64), (ex.clamp(min=1 - bias) - mbits).double()) * X
    free = v.abs() <= top
    assert int(free.sum()) >= 1843                                             # (nine in ten: the bound is not checked on a remnant)
    bound = 6 * d / (2 * S_ ** 0.5)
    ratio = ((acc / S_ - x.double()).abs() / bound)[free].max()
    nearest = ((quantize_with_mx(x, fmt).double() - x.double()).abs() / bound)[free].max()
    print(fmt, "largest |mean - x| / (d / (2 sqrt(S))): stochastic", float(ratio) * 6, "nearest", float(nearest) * 6)
    assert ratio <= 1, float(ratio)
    assert nearest > 1, float(nearest)


def test_mx_linear_rounds_the_two_forms_of_dy_and_nothing_else():
    g = torch.Generator().manual_seed(7)
    K, N, fx, fw, fg = 70, 40, "mxfp8_e4m3", "mxfp6_e2m3", "mxfp4_e2m1"
    w, b = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    x, dy = torch.randn(2, 5, K, generator=g) * 2, torch.randn(2, 5, N, generator=g) / N
    x2, dy2 = x.reshape(-1, K), dy.reshape(-1, N)
    q = lambda t, f: R.reference(t, f, -1)[1:]

    def run(*extra):
        xg, wg, bg = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = mx_linear(xg, wg, bg, fx, fw, fg, *extra)
        y.backward(dy)
        return y.detach(), xg.grad, wg.grad, bg.grad

    step = torch.tensor([10])
    y, dx, dw, db = run("stochastic", 77, step)
    assert int(step) == 11                                                     # one backward, one step
    g_row = S.reference(dy2, fg, -1, torch.float32, 77, 10, 0)[1:]
    g_col = S.reference(dy2.t().contiguous(), fg, -1, torch.float32, 77, 10, 1)[1:]
    assert torch.equal(dx.reshape(-1, K), mx_matmul(*g_row, fg, *q(w.t().contiguous(), fw), fw))
    assert torch.equal(dw, mx_matmul(*g_col, fg, *q(x2.t().contiguous(), fx), fx))
    yn, dxn, dwn, dbn = run()
    assert torch.equal(y, yn) and torch.equal(db, dbn)                         # x and W stay nearest-even; the bias gradient is exact
    assert not torch.equal(dx, dxn) and not torch.equal(dw, dwn)
    y2, dx2, dw2, _ = run("stochastic", 77, step)
    assert int(step) == 12 and torch.equal(y2, y) and not torch.equal(dx2, dx) and not torch.equal(dw2, dw)
    y3, dx3, dw3, _ = run("stochastic", 77 + 10)                               # no counter: the seed alone
    assert torch.equal(dx3, dx) and torch.equal(dw3, dw)
    # nearest mode, asked for by name, is the call as it was
    yq, dxq, dwq, _ = run("nearest", 5, step)
    assert int(step) == 12 and torch.equal(yq, yn) and torch.equal(dxq, dxn) and torch.equal(dwq, dwn)
    assert torch.equal(dxn.reshape(-1, K), mx_matmul(*q(dy2, fg), fg, *q(w.t().contiguous(), fw), fw))
    assert torch.equal(dwn, mx_matmul(*q(dy2.t().contiguous(), fg), fg, *q(x2.t().contiguous(), fx), fx))
    # a first layer (no input gradient) still advances the counter once; a pass that quantizes no gradient does not
    wg = w.clone().requires_grad_(True)
    mx_linear(x, wg, None, fx, fw, fg, "stochastic", 77, step).backward(dy)
    assert int(step) == 13
    bg = b.clone().requires_grad_(True)
    mx_linear(x, w, bg, fx, fw, fg, "stochastic", 77, step).backward(dy)
    assert int(step) == 13
    with pytest.raises(ValueError, match="unknown rounding"):
        mx_linear(x, w, grad_rounding="sr")
    with pytest.raises(TypeError, match="one-element int64"):
        mx_linear(x, w, grad_rounding="stochastic", step=3)


def test_mxtrainlinear_owns_seed_and_step_only_in_stochastic_mode():
    torch.manual_seed(3)
    a = MXTrainLinear(64, 32, grad_fmt="mxfp4_e2m1", grad_rounding="stochastic")
    b = MXTrainLinear(64, 32, grad_fmt="mxfp4_e2m1", grad_rounding="stochastic")
    assert a.sr_seed != b.sr_seed and 0 <= a.sr_seed < 2 ** 62                 # layers do not share their noise
    torch.manual_seed(3)
    a2 = MXTrainLinear(64, 32, grad_fmt="mxfp4_e2m1", grad_rounding="stochastic")
    assert a2.sr_seed == a.sr_seed and torch.equal(a2.weight, a.weight)        # torch.manual_seed reproduces a model
    assert a.sr_step.dtype == torch.int64 and a.sr_step.shape == (1,) and int(a.sr_step) == 0
    assert list(a.state_dict()) == ["weight", "bias"] and "grad_rounding='stochastic'" in repr(a)
    x, gy = torch.randn(6, 64), torch.randn(6, 32)
    a(x).backward(gy)
    a2(x).backward(gy)
    assert int(a.sr_step) == 1 and torch.equal(a.weight.grad, a2.weight.grad)
    g1 = a.weight.grad.clone()
    a.weight.grad = None
    a(x).backward(gy)
    assert int(a.sr_step) == 2 and not torch.equal(a.weight.grad, g1)
    lin = torch.nn.Linear(64, 32)
    c = MXTrainLinear.from_linear(lin, grad_fmt="mxfp6_e3m2", grad_rounding="stochastic", seed=5)
    assert c.sr_seed == 5 and c.weight is lin.weight and c.sr_step.device.type == "cpu" and list(c.state_dict()) == ["weight", "bias"]
    c(x).backward(gy)
    assert int(c.sr_step) == 1
    n = MXTrainLinear(64, 32)
    assert n.grad_rounding == "nearest" and not hasattr(n, "sr_seed") and not hasattr(n, "sr_step") and not list(n.buffers())
    assert "grad_rounding" not in repr(n)
    with pytest.raises(ValueError, match="unknown rounding"):
        MXTrainLinear(4, 4, grad_rounding="sr")
    assert qs.quantize_with_mx is quantize_with_mx


def _layout(tmp_path, cname, ct):
    """sizeof and every offsetof of the header's `cname` by gcc, against the ctypes struct `ct`; returns the field names"""
    fields = [f for f, _ in ct._fields_]
    src = tmp_path / f"{cname}.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu", sizeof(%s));\n%s\nreturn 0; }\n'
                   % (os.path.join(ROOT, "include", "qsparse_hip.h"), cname, "\n".join(f'printf(" %zu", offsetof({cname}, {f}));' for f in fields)))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / cname), str(src)], check=True)
    size, *offs = subprocess.run([str(tmp_path / cname)], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(ct) and [int(o) for o in offs] == [getattr(ct, f).offset for f in fields], cname
    return fields, dict(zip(fields, map(int, offs)))


def test_descriptors_extend_their_predecessors_and_match_the_header(tmp_path):
    one, off1 = _layout(tmp_path, "qs_mx_quant_args", _hip.MxQuantArgs)
    two, off2 = _layout(tmp_path, "qs_mx_quant2_args", _hip.MxQuant2Args)
    # the v27 type names are the same structs: same size, same offsets
    assert _layout(tmp_path, "qs_mx_quant_sr_args", _hip.MxQuantArgs) == (one, off1)
    assert _layout(tmp_path, "qs_mx_quant2_sr_args", _hip.MxQuant2Args) == (two, off2)
    assert one[-5:] == ["rounding", "rng_stream", "seed", "step", "index_base"] and one[-6] == "stream"
    assert two[-5:] == ["rounding", "reserved0", "seed", "step", "index_base"] and two[-6] == "stream"
    # the appended fields begin where the v27 structs ended (8-byte aligned, so nothing moves): sizeof as gcc laid v27 out
    assert (off1["rounding"], off2["rounding"]) == (V27_SIZE_1, V27_SIZE_2) == (80, 88)
    lib = _hip.load()
    assert lib.qs_version() == _hip.ABI_VERSION == 28                          # fields were appended: the version was raised
    for name in ("qs_mx_quant_sr_v", "qs_mx_quant_sr_route", "qs_mx_quant2_sr_v", "qs_mx_quant2_sr_route"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)


def _entry_points(lib):
    """(run, route) of the one-way and of the two-way call: the entry points and their v27 aliases"""
    return (((lib.qs_mx_quant_fwd_v, lib.qs_mx_quant_route), (lib.qs_mx_quant2_v, lib.qs_mx_quant2_route)),
            ((lib.qs_mx_quant_sr_v, lib.qs_mx_quant_sr_route), (lib.qs_mx_quant2_sr_v, lib.qs_mx_quant2_sr_route)))


def test_stochastic_entry_points_validate_without_a_gpu():
    """the whole table by the entry points and again by their v27 aliases: the same answers"""
    for (v1, r1), (v2, r2) in _entry_points(_hip.load()):
        _validation_table(v1, r1, v2, r2)


def _validation_table(v1, r1, v2, r2):
    for fn in (v1, r1, v2, r2):
        assert fn(None) == -2
    for ct, fns in ((_hip.MxQuantArgs, (v1, r1)), (_hip.MxQuant2Args, (v2, r2))):
        short = ct()
        short.struct_size = 2
        assert [fn(ctypes.byref(short)) for fn in fns] == [-2, -2]             # too short to carry its own size
    a = _hip.MxQuantArgs()
    a.struct_size = ctypes.sizeof(a)
    a.x, a.y, a.codes, a.scales, a.outer, a.n, a.inner = 4096, 8192, 16384, 32768, 4, 64, 1
    b = _hip.MxQuant2Args()
    b.struct_size = ctypes.sizeof(b)
    b.x, b.R, b.C, b.row_codes, b.row_scales, b.col_codes, b.col_scales = 4096, 64, 64, 8192, 16384, 32768, 65536
    for d, v, r, ok in ((a, v1, r1, _hip.MX_ROUTE_INNER_VEC), (b, v2, r2, _hip.MX_Q2_ROUTE_TILE_VEC)):
        call = lambda: (v(ctypes.byref(d)), r(ctypes.byref(d)))
        for rounding in (0, 1):
            d.rounding = rounding
            assert r(ctypes.byref(d)) == ok                                    # (a route: nothing is enqueued)
            d.step = 4100
            assert call() == (-2, -2)                                          # step off its 8-byte alignment, in either mode
            d.step = 4104
            assert r(ctypes.byref(d)) == ok
            d.index_base = 6
            assert call() == (-2, -2)                                          # index_base % 4
            d.index_base = 2 ** 63 + 4
            assert r(ctypes.byref(d)) == ok
            d.step, d.index_base = None, 0
        for rounding in (2, -1):
            d.rounding = rounding
            assert call() == (-2, -2)                                          # unknown rounding
        # ... which answers before the other checks do
        d.rounding, d.xdt = 2, 7
        assert call() == (-2, -2)
        d.rounding = 1
        # the other checks still answer
        assert call() == (-1, -1)
        d.xdt, d.x = 0, 4098
        assert call() == (-3, -3)
        d.x = None
        assert call() == (-2, -2)
        d.x = 4096
    a.outer = 0
    assert (v1(ctypes.byref(a)), r1(ctypes.byref(a))) == (0, 0)                # empty: nothing enqueued
    b.C = 0
    assert (v2(ctypes.byref(b)), r2(ctypes.byref(b))) == (0, 0)
    # a caller that knows the v27 fields only (its struct_size): the rounding operands read as zero, which is nearest mode --
    # whatever lies behind the struct it passed
    a.outer, a.rounding, a.step, a.index_base = 4, 9, 4100, 6
    a.struct_size = V27_SIZE_1
    assert r1(ctypes.byref(a)) == _hip.MX_ROUTE_INNER_VEC
    b.C, b.rounding, b.step, b.index_base = 64, 9, 4100, 6
    b.struct_size = V27_SIZE_2
    assert r2(ctypes.byref(b)) == _hip.MX_Q2_ROUTE_TILE_VEC


def test_routes_are_the_predecessors_in_both_modes():
    """the route of a v27-sized descriptor ("old") is the route of the full one ("new") in either mode, by either symbol"""
    lib = _hip.load()
    # two-way: the operands tests/test_mx_train.py walks -- R, C, xdt, x, row pair, col pair
    P = (16384, 8192, 65536, 32768)
    cases = [(64, 64, 1, 4096, P[:2], P[2:]), (64, 68, 1, 4096, P[:2], P[2:]), (64, 68, 0, 4096, P[:2], P[2:]),
             (64, 66, 0, 4096, P[:2], P[2:]), (72, 64, 2, 4096, P[:2], P[2:]), (72, 64, 2, 4096, P[:2], (None, None)),
             (80, 64, 2, 4096, P[:2], P[2:]), (80, 64, 2, 4096, P[:2], (65540, 32768)), (80, 64, 2, 4098, P[:2], P[2:]),
             (80, 64, 2, 4096, (16385, 8193), (65536, 32769)), (80, 64, 2, 4096, (None, None), P[2:]), (0, 64, 1, 4096, P[:2], P[2:]),
             (64, 64, 0, 4098, P[:2], P[2:]), (64, 64, 7, 4096, P[:2], P[2:]), (64, 64, 1, 4096, (16384, None), P[2:])]
    seen = set()
    for R_, C, xdt, x, row, col in cases:
        old, new = _hip.MxQuant2Args(), _hip.MxQuant2Args()
        for d, size in ((old, V27_SIZE_2), (new, ctypes.sizeof(new))):
            d.struct_size = size
            d.R, d.C, d.xdt, d.x, d.row_format, d.col_format = R_, C, xdt, x, 4, 1
            (d.row_codes, d.row_scales), (d.col_codes, d.col_scales) = row, col
        want = lib.qs_mx_quant2_route(ctypes.byref(old))
        seen.add(want)
        for rounding in (0, 1):
            new.rounding, new.seed, new.index_base = rounding, 99, 8
            for route in (lib.qs_mx_quant2_route, lib.qs_mx_quant2_sr_route):
                assert route(ctypes.byref(new)) == want, (R_, C, xdt, x, row, col, rounding)
    assert {_hip.MX_Q2_ROUTE_TILE_VEC, _hip.MX_Q2_ROUTE_TILE_PLAIN, 0, -1, -2, -3} <= seen
    # one-way: outer, n, inner, xdt, x, y, codes
    seen = set()
    for outer, n, inner, xdt, x, y, codes in ((4, 64, 1, 0, 4096, 8192, 16384), (4, 64, 1, 1, 4096, 8192, None), (4, 45, 1, 0, 4096, 8192, 16384),
                                              (4, 64, 1, 0, 4100, 8192, 16384), (4, 64, 1, 0, 4096, 8192, 16388), (3, 40, 5, 2, 4096, 8192, 16384),
                                              (0, 64, 1, 0, 4096, 8192, 16384), (4, 64, 1, 0, 4098, 8192, 16384), (4, 64, 1, 5, 4096, 8192, 16384)):
        old, new = _hip.MxQuantArgs(), _hip.MxQuantArgs()
        for d, size in ((old, V27_SIZE_1), (new, ctypes.sizeof(new))):
            d.struct_size = size
            d.outer, d.n, d.inner, d.xdt, d.ydt, d.x, d.y, d.codes, d.scales, d.format = outer, n, inner, xdt, 0, x, y, codes, 32768 if codes else None, 2
        want = lib.qs_mx_quant_route(ctypes.byref(old))
        seen.add(want)
        for rounding in (0, 1):
            new.rounding, new.rng_stream = rounding, 1
            for route in (lib.qs_mx_quant_route, lib.qs_mx_quant_sr_route):
                assert route(ctypes.byref(new)) == want, (outer, n, inner, xdt, x, y, codes, rounding)
    assert {_hip.MX_ROUTE_INNER_VEC, _hip.MX_ROUTE_INNER_PLAIN, _hip.MX_ROUTE_STRIDED, 0, -1, -3} <= seen
