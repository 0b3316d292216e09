"""MX block-scaled quantizers (OCP microscaling: FP8 / FP6 / FP4 elements, one E8M0 scale per block of 32) on the CPU: the
package's ATen path against the float64 reference of tests/mx_ref.py, bit for bit, and the layers built on it."""
import copy
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn as nn

import mx_ref as R
import qsparse_amd as qs
from qsparse_amd import quantize as Q
from qsparse_amd.quantize import MXQuantization, MXQuantizer, quantize_with_mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = list(R.FORMATS)


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def check(x, fmt, dim=-1, what=""):
    """package result (y, codes, scales) == reference, and y alone == the first of them"""
    ry, rc, rs = R.reference(x, fmt, dim)
    y, c, s = quantize_with_mx(x, fmt, dim, return_codes=True)
    assert R.same(y, ry), (fmt, dim, what, "y")
    assert R.same(c, rc), (fmt, dim, what, "codes")
    assert R.same(s, rs), (fmt, dim, what, "scales")
    assert R.same(quantize_with_mx(x, fmt, dim), ry), (fmt, dim, what, "y without codes")
    return y, c, s


def randn(shape, dtype, seed=0, spread=4.0):
    g = torch.Generator().manual_seed(seed)
    lead = (shape[0],) + (1,) * (len(shape) - 1)
    return (torch.randn(shape, generator=g) * torch.exp(torch.randn(lead, generator=g) * spread)).to(dtype)


def test_reference_definitions_agree_and_grids_have_the_expected_sizes():
    assert [len(R.grid(f)[0]) for f in FMTS] == [127, 124, 32, 32, 8]          # magnitudes, zero included
    x = randn((64, 96), torch.float32, spread=8.0)
    for fmt in R.FP8:
        assert all(R.same(a, b) for a, b in zip(R.ref_grid(x, fmt), R.ref_cast(x, fmt)))


# shapes with and without a partial last block: a line below 32, the conv stem's 3 input channels
SHAPES = [(4, 64), (5, 100), (3, 31), (2, 33), (6, 3, 5, 5), (2, 40, 3), (33,), (2, 64, 2, 2)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_cpu_path_equals_reference(fmt, dtype):
    for shape in SHAPES:
        for dim in (-1, 1, 0):
            if dim >= len(shape):
                continue
            check(randn(shape, dtype, seed=len(shape) + dim), fmt, dim, shape)
    cl = randn((2, 40, 3, 3), dtype).contiguous(memory_format=torch.channels_last)
    y, _, _ = check(cl, fmt, 1, "channels_last")
    assert y.shape == cl.shape


@pytest.mark.parametrize("fmt", sorted(R.FP8))
def test_bytes_decode_through_aten(fmt):
    x = randn((16, 100), torch.float32, spread=10.0)
    x[3, 5] = float("nan")
    y, c, s = quantize_with_mx(x, fmt, -1, return_codes=True)
    X = R.expand_scale(s, 100, 1)
    finite = ~X.isnan()
    assert bool((~finite).any()) and bool(finite.any())
    dec = c.view(R.FP8[fmt]).float().double() * X
    assert R.same(dec[finite].float(), y[finite])
    blocks = s != 255
    assert torch.equal(s[blocks].view(torch.float8_e8m0fnu).float().double(), torch.pow(2.0, s[blocks].double() - 127))
    assert bool(y[~finite].isnan().all()) and bool((c[~finite] == 0).all())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_exhaustive_two_byte_patterns(fmt, dtype):
    eb, mb, bias, emax, top = R.FORMATS[fmt]
    g, gcode = R.grid(fmt)
    seen = set()
    for x in (R.all_patterns(dtype), R.permuted_finite_patterns(dtype)):
        x = x.reshape(-1, 32)
        _, rc, _ = R.reference(x, fmt)
        seen |= set(rc.reshape(-1).tolist())
        check(x, fmt, -1, "exhaustive")
    sign = 1 << (eb + mb)
    want = set(gcode.tolist()) | {c | sign for c in gcode.tolist()}             # every non-NaN, non-Inf code up to the largest normal
    assert want <= seen, sorted(want - seen)[:8]
    assert seen <= want


@pytest.mark.parametrize("fmt", FMTS)
def test_exact_ties_clamp_zeros_nonfinite_and_exponent_clamps(fmt):
    eb, mb, bias, emax, top = R.FORMATS[fmt]
    m = R.midpoints(fmt)
    for k in (-126, -60, -3, 0, 7, 100, 118):
        blk = torch.zeros(len(m), 32)
        blk[:, 0], blk[:, 1], blk[:, 2] = top, m, -m                            # amax = top * 2^k: X = 2^k, x / X is the midpoint itself
        check(blk * 2.0 ** k, fmt, -1, f"ties at 2^{k}")
    # the clamp region: amax / X above the largest normal (1.9 * 2^emax and the rest of the top binade)
    tops = torch.linspace(1.0, 2.0, 32)[:-1].repeat(4, 1) * 2.0 ** emax * torch.tensor([[1.0], [-1.0], [2.0 ** -20], [2.0 ** 30]])
    tops[0, 0] = 1.9 * 2.0 ** emax
    y, _, _ = check(tops, fmt, -1, "clamp")
    assert float(y[0].max()) == top
    z = torch.zeros(2, 64)
    z[0, ::2] = -0.0
    z[1, 40:] = -0.0
    y, c, s = check(z, fmt, -1, "zeros")
    assert bool((s == 0).all()) and torch.equal(torch.signbit(y), torch.signbit(z))
    for bad in (float("nan"), float("inf"), -float("inf")):
        x = randn((3, 96), torch.float32)
        x[1, 40] = bad
        y, c, s = check(x, fmt, -1, f"one {bad}")
        assert s[1].tolist()[1] == 255 and bool(y[1, 32:64].isnan().all()) and not bool(y[1, :32].isnan().any())
    sub = torch.arange(1, 65).float().reshape(2, 32) * 2.0 ** -149                # float32 subnormals: e clamps at -127
    check(torch.cat([sub, -sub * 2 ** 10, sub * 2 ** 24]), fmt, -1, "subnormal blocks")
    big = torch.cat([torch.full((1, 32), 3.0e38), -torch.arange(1, 33).float().reshape(1, 32) * 1.0e37, randn((1, 32), torch.float32) * 2.0 ** 126])
    check(big, fmt, -1, "near 2^127")


def test_output_dtype_follows_the_existing_rule():
    x = randn((4, 64), torch.bfloat16)
    assert quantize_with_mx(x, "mxfp4_e2m1").dtype == torch.float32
    qs.set_qsparse_options(preserve_dtype=True)
    try:
        for fmt in FMTS:
            y = quantize_with_mx(x, fmt)
            assert y.dtype == torch.bfloat16 and R.same(y, R.reference(x, fmt, -1, torch.bfloat16)[0])
            h = x.to(torch.float16) * 1e3
            assert R.same(quantize_with_mx(h, fmt), R.reference(h, fmt, -1, torch.float16)[0])
    finally:
        qs.set_qsparse_options(preserve_dtype=False)


def test_gradient_is_the_incoming_gradient():
    x = randn((4, 70), torch.float32).requires_grad_(True)
    g = torch.randn(4, 70) * 100
    y = quantize_with_mx(x, "mxfp6_e3m2", 1)
    y.backward(g)
    assert torch.equal(x.grad, g)
    gin = torch.randn(4, 70)
    assert MXQuantization.backward(None, gin)[0] is gin                         # unchanged: the very tensor, no kernel


def test_bits_must_match_the_format_and_arguments_are_checked():
    with pytest.raises(ValueError, match=r"4-bit.*bits=8|bits=8.*4-bit"):
        MXQuantizer("mxfp4_e2m1")(torch.zeros(2, 32), 8, None)
    with pytest.raises(ValueError):
        MXQuantizer("mxfp4_e2m1").optimize(torch.zeros(2, 32), 6, None)
    with pytest.raises(ValueError, match="unknown MX format"):
        MXQuantizer("mxfp5")
    with pytest.raises(IndexError):
        quantize_with_mx(torch.zeros(2, 32), "mxfp8_e4m3", 2)
    with pytest.raises(ValueError):
        quantize_with_mx(torch.zeros(()), "mxfp8_e4m3")
    assert qs.MXQuantizer is MXQuantizer and qs.quantize_with_mx is quantize_with_mx and MXQuantizer.weight_size == 1


@pytest.mark.parametrize("kind", ["linear", "conv"])
def test_weight_and_bias_through_quantize(kind):
    torch.manual_seed(0)
    layer = nn.Linear(70, 12) if kind == "linear" else nn.Conv2d(40, 6, 3)
    x = torch.randn(5, 70) if kind == "linear" else torch.randn(2, 40, 8, 8)
    ql = qs.quantize(copy.deepcopy(layer), bits=4, bias_bits=4, timeout=2, callback=MXQuantizer("mxfp4_e2m1", block_dim=1))
    ql.train()
    w_ref = R.reference(layer.weight, "mxfp4_e2m1", 1)[0]
    b_ref = R.reference(layer.bias, "mxfp4_e2m1", -1)[0]           # (a 1-d bias has no dim 1: its blocks run along its only one)
    for step in range(4):
        out = ql(x)
        if step < 2:
            assert torch.equal(out, layer(x))                      # the timeout machinery: identity until then
    assert R.same(ql.weight.detach(), w_ref) and R.same(ql.bias.detach(), b_ref)
    fwd = nn.functional.linear if kind == "linear" else nn.functional.conv2d
    assert torch.equal(ql(x), fwd(x, w_ref, b_ref))
    ql.zero_grad()
    ql(x).sum().backward()
    plain = copy.deepcopy(layer)
    with torch.no_grad():
        plain.weight.copy_(w_ref), plain.bias.copy_(b_ref)
    plain(x).sum().backward()
    wparam = dict(ql.named_parameters())
    gw = [p.grad for n, p in wparam.items() if p.grad is not None and p.shape == layer.weight.shape]
    assert len(gw) == 1 and torch.equal(gw[0], plain.weight.grad)   # straight through: the gradient of the quantized weight
    bad = qs.quantize(copy.deepcopy(layer), bits=8, timeout=1, callback=MXQuantizer("mxfp4_e2m1", 1)).train()
    bad(x)
    with pytest.raises(ValueError, match="bits=8"):
        bad(x)                                                     # the first quantizing step: 8 bits asked of a 4-bit format


def test_lone_activation_layer_with_timeout_and_state_dict_round_trip():
    act = qs.quantize(bits=8, timeout=3, channelwise=-1, callback=MXQuantizer("mxfp8_e4m3", block_dim=1)).train()
    xs = [randn((4, 48, 5), torch.float32, seed=s) for s in range(6)]
    for s, x in enumerate(xs):
        y = act(x)
        if s < 3:
            assert y is x
        else:
            assert R.same(y, R.reference(x, "mxfp8_e4m3", 1)[0])
    assert int(act._n_updates) == 6 and bool((act.weight == 0).all())          # stateless: the weight is never touched
    act.eval()
    assert R.same(act(xs[0]), R.reference(xs[0], "mxfp8_e4m3", 1)[0]) and int(act._n_updates) == 6
    fresh = qs.quantize(bits=8, timeout=3, channelwise=-1, callback=MXQuantizer("mxfp8_e4m3", block_dim=1))
    fresh(xs[0])                                                                # (lazy init, as the reference requires before loading)
    fresh.load_state_dict(act.state_dict())
    qs.load_extra_state_dict(fresh, qs.extra_state_dict(act))
    fresh.eval()
    assert int(fresh._n_updates) == 6 and R.same(fresh(xs[1]), act(xs[1]))


def _net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(3, 40, 3, padding=1), nn.ReLU(), nn.Conv2d(40, 8, 3, padding=1), nn.ReLU(), nn.Flatten(),
                         nn.Linear(8 * 6 * 6, 10))


def test_convert_export_and_dequantize():
    net = _net()
    conv = qs.convert(net, qs.quantize(bits=6, timeout=1, callback=MXQuantizer("mxfp6_e2m3", block_dim=1)), weight_layers=[nn.Conv2d, nn.Linear])
    conv = qs.convert(conv, qs.quantize(bits=8, timeout=1, channelwise=-1, callback=MXQuantizer("mxfp8_e5m2", block_dim=1)),
                      activation_layers=[nn.ReLU])
    conv.train()
    x = torch.randn(4, 3, 6, 6)
    for _ in range(3):
        conv(x).sum().backward()
    ex = qs.export_integer(conv)
    weights = {p: e for p, e in ex.items() if e.weight is not None}
    acts = {p: e for p, e in ex.items() if e.activation is not None and e.activation.get("operator") == "quantize"}
    assert len(weights) == 3 and len(acts) == 2
    conv.eval()
    mods = dict(conv.named_modules())
    for path, e in weights.items():
        w = e.weight
        assert w.kind == "mx" and w.fmt == "mxfp6_e2m3" and w.block_dim == 1 and w.bits == 6
        assert w.codes.dtype == torch.uint8 and w.block_scale.dtype == torch.uint8 and w.codes.shape == w.values.shape
        n = w.codes.shape[1]
        assert w.block_scale.shape[1] == -(-n // 32) and int(w.codes.max()) < 64
        eff = mods[path].weight.detach()
        assert R.same(w.dequantize(), eff)
        rebuilt = type(w)(kind="mx", bits=6, channel_index=-1, codes=w.codes.clone(), values=torch.empty(0), block_scale=w.block_scale.clone(),
                          fmt=w.fmt, block_dim=1)
        assert R.same(rebuilt.dequantize(), eff)                               # from the two byte tensors alone
    for e in acts.values():
        assert e.activation["quantizer"] == "MXQuantizer" and e.activation["fmt"] == "mxfp8_e5m2" and e.activation["block_dim"] == 1
    kinds = {e.weight.kind for e in qs.export_integer(_scaler_net()).values() if e.weight is not None}
    assert kinds == {"scaler"}                                                 # existing kinds unchanged


def _scaler_net():
    net = qs.convert(_net(), qs.quantize(bits=8, timeout=1), weight_layers=[nn.Conv2d, nn.Linear]).train()
    net(torch.randn(2, 3, 6, 6)), net(torch.randn(2, 3, 6, 6))
    return net


def test_entry_point_is_declared_bound_and_validates_without_a_gpu(tmp_path):
    from qsparse_amd import _hip
    lib = _hip.load()
    assert lib.qs_version() >= 28 and _hip.ABI_VERSION == 28
    assert lib.qs_mx_quant_fwd_v(None) == -2
    a = _hip.MxQuantArgs()
    a.struct_size = ctypes.sizeof(a)
    assert lib.qs_mx_quant_fwd_v(ctypes.byref(a)) == -2                         # no tensors
    a.x, a.y, a.outer, a.n, a.inner, a.format = 16, 32, 1, 64, 1, 5
    assert lib.qs_mx_quant_fwd_v(ctypes.byref(a)) == -2                         # unknown format
    a.format, a.xdt = 4, 7
    assert lib.qs_mx_quant_fwd_v(ctypes.byref(a)) == -1                         # unknown dtype
    a.xdt, a.ydt = 0, 1
    assert lib.qs_mx_quant_fwd_v(ctypes.byref(a)) == -1                         # float32 in, bf16 out
    a.ydt, a.x = 0, 18
    assert lib.qs_mx_quant_fwd_v(ctypes.byref(a)) == -3                         # x not even element-aligned
    a.x, a.n = 16, -1
    assert lib.qs_mx_quant_fwd_v(ctypes.byref(a)) == -2
    a.n = 0
    assert lib.qs_mx_quant_fwd_v(ctypes.byref(a)) == 0                          # an empty tensor: accepted, nothing enqueued
    # the route the launch would take, decided by the launching code itself
    a.n = 64
    assert lib.qs_mx_quant_route(ctypes.byref(a)) == _hip.MX_ROUTE_INNER_VEC
    a.n = 33
    assert lib.qs_mx_quant_route(ctypes.byref(a)) == _hip.MX_ROUTE_INNER_PLAIN
    a.n, a.x = 64, 20
    assert lib.qs_mx_quant_route(ctypes.byref(a)) == _hip.MX_ROUTE_INNER_PLAIN
    a.x, a.inner = 16, 9
    assert lib.qs_mx_quant_route(ctypes.byref(a)) == _hip.MX_ROUTE_STRIDED
    # the ctypes mirror against the header's own layout
    fields = [f for f, _ in _hip.MxQuantArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu", sizeof(qs_mx_quant_args));\n%s\nreturn 0; }\n'
                   % (os.path.join(ROOT, "include", "qsparse_hip.h"), "\n".join(f'printf(" %zu", offsetof(qs_mx_quant_args, {f}));' for f in fields)))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(src)], check=True)
    size, *offs = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(_hip.MxQuantArgs) and [int(o) for o in offs] == [getattr(_hip.MxQuantArgs, f).offset for f in fields]
