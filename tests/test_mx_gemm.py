"""Matrix products on MX codes, CPU side: the ATen path of ``mx_matmul`` against the float64 reference of tests/mx_gemm_ref.py, the
entry point's declaration / binding / validation (no GPU needed for any of it), and ``MXLinear``."""
import copy
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn as nn

import mx_gemm_ref as G
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_gemm import MXLinear, mx_matmul
from qsparse_amd.quantize import MXQuantizer, quantize_with_mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
RAGGED_K = (1, 31, 32, 33, 127, 128, 129, 1000)
BITS = {f: G.WIDTH[f] for f in G.FMTS}


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def exact_case(g, M, N, K, fa, fb):
    ra, rb = G.scale_windows(K, fa, fb)
    G.assert_exact_class(K, fa, fb, ra, rb)
    return G.exact_operand(g, M, K, fa, ra) + G.exact_operand(g, N, K, fb, rb)


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_cpu_path_equals_reference_on_the_exact_class(fa, fb):
    g = torch.Generator().manual_seed(G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    for K in RAGGED_K:
        ac, asc, bc, bsc = exact_case(g, 7, 9, K, fa, fb)
        bias = torch.randint(-64, 64, (9,), generator=g).float()
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            want, y64, _ = G.reference(ac, asc, fa, bc, bsc, fb, None, dt)
            got = mx_matmul(ac, asc, fa, bc, bsc, fb, out_dtype=dt)
            assert got.dtype == dt and G.same(got, want), (K, dt)
        assert G.same(mx_matmul(ac, asc, fa, bc, bsc, fb, bias), G.reference(ac, asc, fa, bc, bsc, fb, bias)[0]), (K, "bias")
    # 0xFF blocks: NaN exactly in the rows / columns that read them, everything else still exact
    ac, asc, bc, bsc = exact_case(g, 6, 8, 100, fa, fb)
    asc[2, 1], bsc[5, 3], bsc[0, 0] = 255, 255, 255
    want, y64, _ = G.reference(ac, asc, fa, bc, bsc, fb)
    nan = torch.zeros(6, 8, dtype=torch.bool)
    nan[2, :], nan[:, 5], nan[:, 0] = True, True, True
    assert torch.equal(y64.isnan(), nan)
    assert G.same(mx_matmul(ac, asc, fa, bc, bsc, fb), want)
    # leading batch dimensions are flattened into M and restored
    ac, asc, bc, bsc = exact_case(g, 24, 5, 70, fa, fb)
    y = mx_matmul(ac.view(2, 3, 4, 70), asc.view(2, 3, 4, 3), fa, bc, bsc, fb)
    assert y.shape == (2, 3, 4, 5) and G.same(y.reshape(24, 5), G.reference(ac, asc, fa, bc, bsc, fb)[0])
    assert mx_matmul(ac[0], asc[0], fa, bc, bsc, fb).shape == (5,)


@pytest.mark.parametrize("fa,fb", [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp8_e5m2", "mxfp6_e3m2"), ("mxfp6_e2m3", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp8_e4m3"),
                                   ("mxfp4_e2m1", "mxfp4_e2m1")])
def test_cpu_path_on_quantizer_inputs_within_the_float64_bound(fa, fb):
    """float64 accumulation in the BLAS's order: |y - y64| <= K 2^-52 S + ulp_ydt(y64)"""
    g = torch.Generator().manual_seed(1)
    for K in (96, 1000):
        x, w, bias = torch.randn(33, K, generator=g), torch.randn(17, K, generator=g) / K ** 0.5, torch.randn(17, generator=g)
        _, ac, asc = quantize_with_mx(x, fa, -1, return_codes=True)
        _, bc, bsc = quantize_with_mx(w, fb, -1, return_codes=True)
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            _, y64, S = G.reference(ac, asc, fa, bc, bsc, fb, bias, dt)
            got = mx_matmul(ac, asc, fa, bc, bsc, fb, bias, dt)
            ok, ratio = G.within(got, y64, K * 2.0 ** -52 * S + G.ulp(y64, dt))
            print(fa, fb, K, dt, "largest |err| / bound", ratio)
            assert ok, (K, dt, ratio)


def test_arguments_are_checked_before_anything_runs():
    g = torch.Generator().manual_seed(0)
    ac, asc = G.exact_operand(g, 4, 64, "mxfp8_e4m3", 1)
    bc, bsc = G.exact_operand(g, 5, 64, "mxfp4_e2m1", 1)
    ok = lambda **kw: mx_matmul(**{**dict(a_codes=ac, a_scales=asc, a_fmt="mxfp8_e4m3", b_codes=bc, b_scales=bsc, b_fmt="mxfp4_e2m1"), **kw})
    assert ok().shape == (4, 5)
    with pytest.raises(ValueError, match="unknown MX format"):
        ok(a_fmt="mxfp5")
    with pytest.raises(TypeError, match="uint8"):
        ok(a_codes=ac.float())
    with pytest.raises(TypeError, match="uint8"):
        ok(b_scales=bsc.int())
    with pytest.raises(ValueError, match="a_scales has shape"):
        ok(a_scales=asc[:, :1])
    with pytest.raises(ValueError, match="disagree on K"):
        ok(b_codes=bc[:, :32].contiguous(), b_scales=bsc[:, :1].contiguous())
    with pytest.raises(ValueError, match=r"\[N, K\]"):
        ok(b_codes=bc.view(1, 5, 64), b_scales=bsc.view(1, 5, 2))
    with pytest.raises(TypeError, match="float32"):
        ok(bias=torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="bias has shape"):
        ok(bias=torch.zeros(4))
    with pytest.raises(TypeError, match="out_dtype"):
        ok(out_dtype=torch.float64)
    with pytest.raises(ValueError, match="K >= 1"):
        ok(a_codes=ac[:, :0], a_scales=asc[:, :0], b_codes=bc[:, :0], b_scales=bsc[:, :0])
    assert qs.mx_matmul is mx_matmul and qs.MXLinear is MXLinear


def test_entry_point_is_declared_bound_and_validates_without_a_gpu(tmp_path):
    lib = _hip.load()
    assert lib.qs_version() == _hip.ABI_VERSION == 28                          # the version this binding needs
    assert "qs_mx_matmul_v" in _hip.SIGNATURES and "qs_mx_matmul_route" in _hip.SIGNATURES
    assert lib.qs_mx_matmul_v(None) == -2 and lib.qs_mx_matmul_route(None) == -2
    a = _hip.MxMatmulArgs()
    a.struct_size = ctypes.sizeof(a)
    assert lib.qs_mx_matmul_v(ctypes.byref(a)) == -2                           # no tensors
    a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.y = 1024, 2048, 4096, 8192, 16384
    a.M, a.N, a.K = 4, 5, 64
    a.a_format = 5
    assert lib.qs_mx_matmul_v(ctypes.byref(a)) == -2                           # unknown format
    a.a_format, a.b_format = 4, -1
    assert lib.qs_mx_matmul_v(ctypes.byref(a)) == -2
    a.b_format, a.ydt = 2, 7
    assert lib.qs_mx_matmul_v(ctypes.byref(a)) == -1                           # unknown dtype
    a.ydt, a.y = 0, 16386
    assert lib.qs_mx_matmul_v(ctypes.byref(a)) == -3                           # y not aligned to a float32
    a.ydt = 1
    assert lib.qs_mx_matmul_route(ctypes.byref(a)) == _hip.MX_GEMM_ROUTE_VEC   # ... but to a bf16
    a.bias = 6
    assert lib.qs_mx_matmul_v(ctypes.byref(a)) == -3                           # bias not aligned to a float32
    a.bias, a.y, a.ydt, a.K = None, 16384, 0, -1
    assert lib.qs_mx_matmul_v(ctypes.byref(a)) == -2
    a.K = 0
    assert lib.qs_mx_matmul_v(ctypes.byref(a)) == -2                           # K >= 1
    a.K, a.M = 64, 0
    assert lib.qs_mx_matmul_v(ctypes.byref(a)) == 0                            # an empty product: accepted, nothing enqueued
    a.M, a.N = 4, 0
    assert lib.qs_mx_matmul_v(ctypes.byref(a)) == 0
    # the route the launch would take, decided by the launching code itself
    a.N = 5
    assert lib.qs_mx_matmul_route(ctypes.byref(a)) == _hip.MX_GEMM_ROUTE_VEC
    a.K = 72
    assert lib.qs_mx_matmul_route(ctypes.byref(a)) == _hip.MX_GEMM_ROUTE_PLAIN     # K % 16 != 0
    a.K, a.a_codes = 64, 1025
    assert lib.qs_mx_matmul_route(ctypes.byref(a)) == _hip.MX_GEMM_ROUTE_PLAIN     # unaligned code base
    a.a_codes, a.b_codes = 1024, 4100
    assert lib.qs_mx_matmul_route(ctypes.byref(a)) == _hip.MX_GEMM_ROUTE_PLAIN
    a.b_codes, a.a_scales, a.b_scales = 4096, 2049, 8193
    assert lib.qs_mx_matmul_route(ctypes.byref(a)) == _hip.MX_GEMM_ROUTE_VEC       # scale bytes: any address
    short = _hip.MxMatmulArgs()
    short.struct_size = 2
    assert lib.qs_mx_matmul_v(ctypes.byref(short)) == -2                       # a descriptor too short to carry its own size
    # the ctypes mirror against the header's own layout
    fields = [f for f, _ in _hip.MxMatmulArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu", sizeof(qs_mx_matmul_args));\n%s\nreturn 0; }\n'
                   % (os.path.join(ROOT, "include", "qsparse_hip.h"), "\n".join(f'printf(" %zu", offsetof(qs_mx_matmul_args, {f}));' for f in fields)))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(src)], check=True)
    size, *offs = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(_hip.MxMatmulArgs) and [int(o) for o in offs] == [getattr(_hip.MxMatmulArgs, f).offset for f in fields]


def _quantized_linear(fmt, K=70, N=12, bias_bits=-1, block_dim=1, seed=0):
    torch.manual_seed(seed)
    layer = qs.quantize(nn.Linear(K, N), bits=BITS[fmt], bias_bits=bias_bits, timeout=1, callback=MXQuantizer(fmt, block_dim=block_dim)).train()
    layer(torch.randn(3, K)), layer(torch.randn(3, K))
    return layer.eval()


@pytest.mark.parametrize("wfmt,afmt", [("mxfp4_e2m1", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp6_e3m2"), ("mxfp8_e4m3", "mxfp4_e2m1"), ("mxfp8_e5m2", "mxfp8_e5m2")])
@pytest.mark.parametrize("bias_bits", [-1, 0])
def test_mxlinear_equals_the_simulated_layer_on_mx_quantized_input(wfmt, afmt, bias_bits):
    """the property: MXLinear.from_quantized(layer, fmt)(x) is the simulated layer's evaluation-mode output on quantize_with_mx(x,
    fmt, -1), up to the two summations: float32 in ATen's order there (K 2^-24 S + ulp), float64 here"""
    layer = _quantized_linear(wfmt, bias_bits=BITS[wfmt] if bias_bits == 0 else -1)
    mxl = MXLinear.from_quantized(layer, afmt)
    assert mxl.weight_fmt == wfmt and mxl.act_fmt == afmt and mxl.weight_codes.shape == (12, 70) and mxl.weight_scales.shape == (12, 3)
    assert mxl.bias.dtype == torch.float32 and torch.equal(mxl.bias, layer.bias.detach())
    x = torch.randn(2, 5, 70, generator=torch.Generator().manual_seed(4)) * 3
    y = mxl(x)
    assert y.shape == (2, 5, 12) and y.dtype == torch.float32 and not y.requires_grad
    xq, ac, asc = quantize_with_mx(x, afmt, -1, return_codes=True)
    with torch.no_grad():
        sim = layer(xq)
    _, y64, S = G.reference(ac.reshape(10, 70), asc.reshape(10, 3), afmt, mxl.weight_codes, mxl.weight_scales, wfmt, mxl.bias)
    bound = 70 * 2.0 ** -52 * S + G.ulp(y64, torch.float32)
    assert G.within(y.reshape(10, 12), y64, bound)[0]
    gpu_bound = 2 * 70 * 2.0 ** -23 * S + 2.0 ** -23 * mxl.bias.abs().double() + G.ulp(y64, torch.float32)     # the bound the GPU tests use
    assert bool(((y.double() - sim.double()).reshape(10, 12).abs() <= gpu_bound).all())
    assert G.within(sim.reshape(10, 12), y64, 70 * 2.0 ** -24 * S + 2.0 ** -23 * mxl.bias.abs().double() + G.ulp(y64, torch.float32))[0]
    # and the weight the simulated layer multiplies with is what the codes decode to
    assert torch.equal(G.values(mxl.weight_codes, mxl.weight_scales, wfmt).float(), layer.weight.detach())


def test_mxlinear_constructors_refusals_and_state_dict():
    layer = _quantized_linear("mxfp6_e3m2")
    ex = qs.export_integer(nn.Sequential(layer))["0"]
    a, b = MXLinear.from_quantized(layer, "mxfp8_e4m3"), MXLinear.from_exported(ex.weight, layer.bias.detach(), "mxfp8_e4m3")
    x = torch.randn(6, 70)
    assert torch.equal(a(x), b(x)) and set(a.state_dict()) == {"weight_codes", "weight_scales", "bias"}
    assert not list(a.parameters()) and "weight_fmt='mxfp6_e3m2'" in repr(a)
    nobias = MXLinear.from_exported(ex.weight, None, "mxfp4_e2m1")
    assert nobias.bias is None and set(nobias.state_dict()) == {"weight_codes", "weight_scales"} and nobias(x).shape == (6, 12)
    # state_dict round trip into a layer built from another weight
    other = MXLinear.from_quantized(_quantized_linear("mxfp6_e3m2", seed=9), "mxfp8_e4m3")
    assert not torch.equal(other(x), a(x))
    other.load_state_dict(copy.deepcopy(a.state_dict()))
    assert torch.equal(other(x), a(x))
    # blocks along N cannot feed the instruction
    along_n = _quantized_linear("mxfp8_e4m3", block_dim=0)
    with pytest.raises(ValueError, match="along K"):
        MXLinear.from_quantized(along_n, "mxfp8_e4m3")
    with pytest.raises(ValueError, match="along K"):
        MXLinear.from_exported(qs.export_integer(nn.Sequential(along_n))["0"].weight, None)
    scaler = qs.quantize(nn.Linear(70, 12), bits=8, timeout=1).train()
    scaler(x), scaler(x)
    with pytest.raises(ValueError, match="MXQuantizer"):
        MXLinear.from_quantized(scaler, "mxfp8_e4m3")
    with pytest.raises(ValueError, match="kind"):
        MXLinear.from_exported(qs.export_integer(nn.Sequential(scaler))["0"].weight, None)
    fresh = qs.quantize(nn.Linear(70, 12), bits=8, timeout=5, callback=MXQuantizer("mxfp8_e4m3", block_dim=1))
    with pytest.raises(ValueError, match="timeout"):
        MXLinear.from_quantized(fresh, "mxfp8_e4m3")
    with pytest.raises(ValueError, match="unknown MX format"):
        MXLinear.from_quantized(layer, "mxfp3")
    # inference only
    with pytest.raises(RuntimeError, match="requires grad"):
        a(x.clone().requires_grad_(True))
    with torch.no_grad():
        assert not a(x.clone().requires_grad_(True)).requires_grad
    assert layer.training is False and _quantized_linear("mxfp6_e3m2").train().training
