"""Deterministic split-K of the MX matrix product, CPU side: the slicing plan and the automatic slice count against the rule as
include/qsparse_hip.h states it (re-derived here), the three entry points' declaration / binding / validation, and the Python
arguments (no GPU needed for any of it)."""
import ctypes
import os
import subprocess

import pytest
import torch

import mx_gemm_ref as G
from qsparse_amd import _hip
from qsparse_amd.mx_gemm import MXTrainLinear, mx_linear, mx_matmul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_ALIGN, ERR_WORKSPACE = -2, -3, -4


def cdiv(a, b):
    return -(-a // b)


def plan_by_the_text(M, N, K, S):
    """(S', workspace bytes) from the header's text: per = ceil(steps / S), S' = ceil(steps / per), S' M N 4 bytes unless S' == 1"""
    steps = cdiv(K, 128)
    per = cdiv(steps, S)
    s = cdiv(steps, per)
    return s, (s * M * N * 4 if s > 1 else 0)


def auto_by_the_text(M, N, K):
    tiles, steps = cdiv(M, 128) * cdiv(N, 128), cdiv(K, 128)
    if steps < 32 or tiles >= 256:
        return 1
    return max(1, min(512 // tiles, steps // 8, 16))


@pytest.mark.parametrize("K,S", [(256, 2), (1000, 3), (400, 4), (129, 2), (130, 8), (16, 4), (1, 1), (1, 7), (128, 2), (129, 1000), (50432, 3),
                                 (50432, 5), (1280, 4), (1281, 4), (128 * 7, 4), (128 * 9, 4), (128 * 10, 6), (128 * 91, 12), (2 ** 20, 16),
                                 (2 ** 20 + 1, 2 ** 31 - 1)])
def test_plan_is_the_headers_slicing(K, S):
    for M, N in ((1, 1), (130, 67), (3072, 768)):
        want = plan_by_the_text(M, N, K, S)
        assert _hip.mx_split_plan(M, N, K, S) == want, (M, N, K, S)
        steps, (s, _) = cdiv(K, 128), want
        per = cdiv(steps, S)
        assert 1 <= s <= min(S, steps) and (s - 1) * per < steps <= s * per        # no slice is empty, together they cover K
        assert _hip.mx_split_plan(M, N, K, s)[0] == s                               # S' asked for again is S' again


def test_plan_refusals_and_empty_products():
    lib = _hip.load()
    plan = lambda *a: lib.qs_mx_matmul_splitk_plan(*a, None, None)
    assert plan(4, 4, 128, 2) == 0                                                  # (both outputs are optional)
    assert plan(-1, 4, 128, 2) == ERR_ARG and plan(4, -1, 128, 2) == ERR_ARG and plan(4, 4, -1, 2) == ERR_ARG
    assert plan(4, 4, 128, -1) == ERR_ARG and plan(4, 4, 0, 1) == ERR_ARG
    assert plan(2 ** 40, 2 ** 40, 128, 1) == ERR_ARG                                # M N beyond 63 bits
    assert plan(2 ** 31, 2 ** 30, 1024, 8) == ERR_ARG and plan(2 ** 31, 2 ** 30, 1024, 1) == 0      # S' M N 4 beyond 64 bits
    assert _hip.mx_split_plan(0, 5, 1000, 3) == (1, 0) and _hip.mx_split_plan(5, 0, 0, 0) == (1, 0)


# the (M, N, K) of tests/test_mx_gemm_gpu.py (SHAPES and the offset-base case), tests/test_mx_gemm_canary_gpu.py (CASES) and
# tests/test_mx_train_gpu.py (ALIGNED, RAGGED, the mixed-dtype case), copied
EXISTING = [(1, 300, 128), (15, 17, 129), (16, 128, 1000), (127, 129, 33), (300, 1, 31), (129, 16, 127), (128, 127, 32), (17, 15, 1),
            (300, 300, 256), (129, 130, 256),
            (128, 128, 128), (1, 1, 16), (129, 127, 144), (37, 301, 400), (5, 3, 1), (130, 67, 129), (17, 129, 31), (64, 64, 256), (200, 9, 1000),
            (512, 576, 640), (530, 522, 542), (10, 48, 96)]


def test_automatic_rule():
    auto = lambda M, N, K: _hip.mx_split_plan(M, N, K, 0)[0]
    for M, N, K in EXISTING:
        # as a layer's three products: forward [M, K] x [N, K], dgrad [M, N] x [K, N], wgrad [N, M] x [K, M]
        for m, n, k in ((M, N, K), (M, K, N), (N, K, M)):
            assert auto(m, n, k) == 1, (m, n, k)
    assert auto(128, 128, 31 * 128) == 1 and auto(128, 128, 31 * 128 + 1) > 1       # steps = 31 | 32
    assert auto(128 * 16, 128 * 16, 128 * 400) == 1                                 # tiles = 256
    assert auto(128 * 16, 128 * 16 - 128, 128 * 400) == 2                           # tiles = 240
    assert auto(3072, 768, 50432) == 3 and auto(768, 3072, 50432) == 3              # the ViT-B MLP weight gradients
    assert auto(128, 128, 4096) == 4
    g = torch.Generator().manual_seed(0)
    for _ in range(2000):
        M, N = (int(torch.randint(1, 5000, (1,), generator=g)) for _ in range(2))
        K = int(torch.randint(1, 200000, (1,), generator=g))
        got = auto(M, N, K)
        assert got == plan_by_the_text(M, N, K, auto_by_the_text(M, N, K))[0] and 1 <= got <= 16, (M, N, K)      # (the plan's S')


def _args(**kw):
    """a well-formed split descriptor on made-up addresses (nothing is ever enqueued here: every call below is refused, or empty)"""
    a = _hip.MxMatmulSplitkArgs()
    a.struct_size = ctypes.sizeof(a)
    a.a_format = a.b_format = 0
    a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.y = 1024, 2048, 4096, 8192, 16384
    a.ydt, a.M, a.N, a.K = 0, 130, 67, 1000
    a.split_k, a.workspace, a.workspace_bytes = 3, 1 << 20, 3 * 130 * 67 * 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_entry_points_are_declared_bound_and_validate_without_a_gpu(tmp_path):
    lib = _hip.load()
    assert lib.qs_version() == _hip.ABI_VERSION == 28                               # symbols were added, the version stays
    for name in ("qs_mx_matmul_splitk_v", "qs_mx_matmul_splitk_route", "qs_mx_matmul_splitk_plan"):
        assert name in _hip.SIGNATURES
    assert lib.qs_mx_matmul_splitk_v(None) == ERR_ARG and lib.qs_mx_matmul_splitk_route(None) == ERR_ARG
    v = lambda **kw: lib.qs_mx_matmul_splitk_v(ctypes.byref(_args(**kw)))
    route = lambda **kw: lib.qs_mx_matmul_splitk_route(ctypes.byref(_args(**kw)))
    short = _hip.MxMatmulSplitkArgs()
    short.struct_size = 2
    assert lib.qs_mx_matmul_splitk_v(ctypes.byref(short)) == ERR_ARG                # too short to carry its own size
    assert v(struct_size=_hip.MxMatmulSplitkArgs.y.offset) == ERR_ARG               # ... or one that ends before y
    assert v(struct_size=_hip.MxMatmulSplitkArgs.split_k.offset) == ERR_ARG         # ... or before split_k (reads as 0)
    blank = _hip.MxMatmulSplitkArgs()
    blank.struct_size = ctypes.sizeof(blank)
    assert lib.qs_mx_matmul_splitk_v(ctypes.byref(blank)) == ERR_ARG
    # the request and the workspace
    assert route() == _hip.MX_GEMM_ROUTE_PLAIN and route(K=1008) == _hip.MX_GEMM_ROUTE_VEC
    assert v(split_k=0) == ERR_ARG and v(split_k=-1) == ERR_ARG and route(split_k=0) == ERR_ARG
    assert v(workspace_bytes=3 * 130 * 67 * 4 - 1) == ERR_WORKSPACE
    assert v(workspace=(1 << 20) + 4) == ERR_ALIGN and v(workspace=(1 << 20) + 8) == ERR_ALIGN
    assert v(workspace=None) == ERR_ARG and route(workspace=None) == ERR_ARG        # S' = 3: refused, nothing enqueued
    # their precedence: NULL, then the alignment, then the size, then the grid of tiles x slices
    assert route(workspace=None, workspace_bytes=0) == ERR_ARG and route(workspace=(1 << 20) + 8, workspace_bytes=0) == ERR_ALIGN
    big = dict(M=46340 * 128, N=46340 * 128, split_k=2)                             # 46340^2 tiles fit a grid, twice as many do not
    assert route(**big, workspace_bytes=2 * (46340 * 128) ** 2 * 4 - 1) == ERR_WORKSPACE
    assert route(**big, workspace_bytes=2 * (46340 * 128) ** 2 * 4) == ERR_ARG and route(**{**big, "split_k": 1}) == _hip.MX_GEMM_ROUTE_PLAIN
    assert route(workspace=None, workspace_bytes=0, K=100) == _hip.MX_GEMM_ROUTE_PLAIN      # S' = 1: no workspace needed
    assert route(workspace=None, workspace_bytes=0, split_k=1) == _hip.MX_GEMM_ROUTE_PLAIN
    assert route(split_k=8, workspace_bytes=8 * 130 * 67 * 4) == _hip.MX_GEMM_ROUTE_PLAIN and v(split_k=8) == ERR_WORKSPACE
    assert route(split_k=9, workspace_bytes=8 * 130 * 67 * 4) == _hip.MX_GEMM_ROUTE_PLAIN                             # per = 1, S' = 8: 9 asks for no more than 8 does
    # every check of qs_mx_matmul_v, unchanged and first
    for null in ("a_codes", "a_scales", "b_codes", "b_scales", "y"):
        assert v(**{null: None}) == ERR_ARG
    assert v(a_format=5) == ERR_ARG and v(b_format=-1) == ERR_ARG and v(ydt=7) == -1 and v(ydt=7, split_k=0) == -1
    assert v(y=16386) == ERR_ALIGN and route(y=16386, ydt=1) == _hip.MX_GEMM_ROUTE_PLAIN and v(bias=6) == ERR_ALIGN
    assert v(M=-1) == ERR_ARG and v(K=0) == ERR_ARG
    assert v(M=0) == 0 and v(N=0, workspace=None) == 0 and v(M=0, split_k=0) == ERR_ARG      # empty: accepted after the checks
    assert route(a_codes=1025) == _hip.MX_GEMM_ROUTE_PLAIN and route(K=1008, b_codes=4097) == _hip.MX_GEMM_ROUTE_PLAIN
    # the ctypes mirror against the header's own layout; the leading fields are qs_mx_matmul_args'
    T = _hip.MxMatmulSplitkArgs
    fields = [f for f, _ in T._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu", sizeof(qs_mx_matmul_splitk_args));\n%s\nreturn 0; }\n'
                   % (os.path.join(ROOT, "include", "qsparse_hip.h"), "\n".join(f'printf(" %zu", offsetof(qs_mx_matmul_splitk_args, {f}));' for f in fields)))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(src)], check=True)
    size, *offs = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(T) and [int(o) for o in offs] == [getattr(T, f).offset for f in fields]
    assert all(getattr(T, f).offset == getattr(_hip.MxMatmulArgs, f).offset for f, _ in _hip.MxMatmulArgs._fields_)


def _exact_ops(M, N, K, fa="mxfp8_e4m3", fb="mxfp6_e2m3", seed=0):
    g = torch.Generator().manual_seed(seed)
    ra, rb = G.scale_windows(K, fa, fb)
    return G.exact_operand(g, M, K, fa, ra) + G.exact_operand(g, N, K, fb, rb), fa, fb


def test_mx_matmul_split_k_argument_on_the_cpu():
    (ac, asc, bc, bsc), fa, fb = _exact_ops(9, 7, 300)
    bias = torch.arange(7.0)
    y1 = mx_matmul(ac, asc, fa, bc, bsc, fb, bias, torch.bfloat16)
    for s in (1, 3, 1000, "auto"):
        assert torch.equal(mx_matmul(ac, asc, fa, bc, bsc, fb, bias, torch.bfloat16, split_k=s), y1)
    for bad in (0, -1, 2 ** 31, "Auto", "", "2"):
        with pytest.raises(ValueError):
            mx_matmul(ac, asc, fa, bc, bsc, fb, split_k=bad)
    for bad in (True, False, 2.0, None, (2,), torch.tensor(2)):
        with pytest.raises(TypeError):
            mx_matmul(ac, asc, fa, bc, bsc, fb, split_k=bad)
    with pytest.raises(TypeError):
        mx_matmul(ac, asc, fa, bc, bsc, fb, None, torch.float32, 2)                 # keyword only


def test_mx_linear_wgrad_split_k_on_the_cpu():
    g = torch.Generator().manual_seed(1)
    x, w, b, dy = torch.randn(40, 24, generator=g), torch.randn(12, 24, generator=g), torch.randn(12, generator=g), torch.randn(40, 12, generator=g)

    def step(**kw):
        xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
        y = mx_linear(xs, ws, bs, **kw)
        y.backward(dy)
        return y.detach(), xs.grad, ws.grad, bs.grad

    base = step()
    for s in (1, 2, "auto"):
        assert all(torch.equal(a, c) for a, c in zip(step(wgrad_split_k=s), base))
    with pytest.raises(ValueError):
        mx_linear(x, w, b, wgrad_split_k=0)
    with pytest.raises(TypeError):
        mx_linear(x, w, b, wgrad_split_k=True)
    layer = MXTrainLinear(24, 12, wgrad_split_k=2)
    assert layer.wgrad_split_k == 2 and "wgrad_split_k=2" in repr(layer) and MXTrainLinear(24, 12).wgrad_split_k == "auto"
    assert "wgrad_split_k" not in repr(MXTrainLinear(24, 12))
    twin = MXTrainLinear.from_linear(torch.nn.Linear(24, 12), wgrad_split_k=4)
    assert twin.wgrad_split_k == 4
    with pytest.raises(ValueError):
        MXTrainLinear(24, 12, wgrad_split_k="no")
    layer(x).sum().backward()
    assert layer.weight.grad is not None
