"""Deterministic split-K of the MX matrix product on the GPU (qs_mx_matmul_splitk_v; include/qsparse_hip.h, "MX matrix product, split
along K").

The definition is a composition: the split result is the ordered float32 sum of what the UNSPLIT kernel gives for each slice of K,
plus the bias, rounded once.  ``test_slice_composition_bit_for_bit`` evaluates exactly that with the unsplit kernel and torch's
float32 adds on the device and asks for the same bits, on random (not exactly summable) operands -- so a partial kernel that
deviates from the unsplit operation sequence, a reduction in another order, a fused multiply-add or a second rounding all show.  The
other tests: the exact class against the float64 CPU reference, the workspace (pre-filled, guarded, no stale reads), 0xFF scale
bytes, training through ``mx_linear(wgrad_split_k=...)`` and graph capture."""
import ctypes

import pytest
import torch

import mx_gemm_ref as G
from mx_guard import guarded as _guarded, intact as _intact
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_gemm import mx_linear, mx_matmul, mx_quantize_2way

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN
PAIRS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp8_e5m2"), ("mxfp6_e3m2", "mxfp6_e3m2")]
# M, N, K, requested S, byte offset of the code bases
CASES = [(128, 128, 256, 2, 0),
         (130, 67, 1000, 3, 0),        # PLAIN; slices of 3 / 3 / 2 steps; last step and last block short
         (37, 301, 400, 4, 0),         # one step per slice
         (5, 3, 129, 2, 0),            # second slice is one code
         (16, 16, 130, 8, 0),          # S' = 2 < S
         (1, 1, 16, 4, 0),             # S' = 1: the unsplit call
         (64, 64, 256, 2, 1)]          # code bases offset by 1 byte (PLAIN)


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def cdiv(a, b):
    return -(-a // b)


def slicing(K, S):
    """(S', [(k0, k1)]) by the header's rule"""
    steps = cdiv(K, 128)
    per = cdiv(steps, S)
    n = cdiv(steps, per)
    return n, [(128 * s * per, min(128 * (s + 1) * per, K)) for s in range(n)]


def random_operand(g, rows, K, fmt):
    """codes drawn from ALL the codes the quantizer can write, scale bytes from a window of 16: nothing exactly summable"""
    t = G.table(fmt)[: 1 << G.WIDTH[fmt]]
    valid = (~t.isnan()).nonzero().reshape(-1)
    codes = valid[torch.randint(0, len(valid), (rows, K), generator=g)].to(torch.uint8)
    scales = torch.randint(119, 135, (rows, cdiv(K, 32)), generator=g).to(torch.uint8)
    return codes, scales


def at_offset(t, off):
    """`t` on the device, its base `off` bytes past a 16-byte boundary"""
    if not off:
        return t.to(DEV)
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    view = flat[off:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == off and view.is_contiguous()
    return view


def on_device(ops, off):
    ac, asc, bc, bsc = ops
    return at_offset(ac, off), asc.to(DEV), at_offset(bc, off), bsc.to(DEV)


def route_of(ac, bc):
    return VEC if ac.shape[1] % 16 == 0 and ac.data_ptr() % 16 == 0 and bc.data_ptr() % 16 == 0 else PLAIN


def split(dev, fa, fb, bias, dt, S, want_slices):
    y = mx_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, bias, dt, split_k=S)
    assert _hip.mx_gemm_last_route == route_of(dev[0], dev[2]) and _hip.mx_gemm_last_split == want_slices
    return y


def partials(dev, fa, fb, ranges):
    ac, asc, bc, bsc = dev
    out = []
    for k0, k1 in ranges:
        a, b = ac[:, k0:k1].contiguous(), bc[:, k0:k1].contiguous()
        sa, sb = asc[:, k0 // 32:cdiv(k1, 32)].contiguous(), bsc[:, k0 // 32:cdiv(k1, 32)].contiguous()
        out.append(mx_matmul(a, sa, fa, b, sb, fb, None, torch.float32, split_k=1))
        assert _hip.mx_gemm_last_route == route_of(a, b) and _hip.mx_gemm_last_split == 1
    return out


def ordered_sum(ps, bias, dt):
    acc = ps[0]
    for p in ps[1:]:
        acc = acc + p                              # float32, ascending s
    if bias is not None:
        acc = acc + bias
    return acc.to(dt)                              # the one rounding


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_slice_composition_bit_for_bit(fa, fb):
    for M, N, K, S, off in CASES:
        g = torch.Generator().manual_seed(M * 1000 + N + K)
        dev = on_device(random_operand(g, M, K, fa) + random_operand(g, N, K, fb), off)
        bias = torch.randn(N, generator=g).to(DEV)
        n, ranges = slicing(K, S)
        ps = partials(dev, fa, fb, ranges)
        assert (route_of(dev[0], dev[2]) == PLAIN) == (K % 16 != 0 or off != 0)
        for dt in (torch.float32, torch.bfloat16):
            for b in (None, bias):
                y = split(dev, fa, fb, b, dt, S, n)
                assert y.dtype == dt and G.same(y, ordered_sum(ps, b, dt)), (fa, fb, M, N, K, S, dt, b is not None)
                if n == 1:                         # S' = 1 is the plain call
                    assert torch.equal(y, mx_matmul(dev[0], dev[1], fa, dev[2], dev[3], fb, b, dt))


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_exact_class_equals_the_cpu_reference(fa, fb):
    """where every summation order is exact the split result is the reference's, whatever the slicing"""
    for M, N, K, S, off in CASES:
        g = torch.Generator().manual_seed(M + N * 1000 + K)
        ra, rb = G.scale_windows(K, fa, fb)
        G.assert_exact_class(K, fa, fb, ra, rb)
        ops = G.exact_operand(g, M, K, fa, ra) + G.exact_operand(g, N, K, fb, rb)
        bias = torch.randint(-16, 16, (N,), generator=g).float()
        dev = on_device(ops, off)
        n = slicing(K, S)[0]
        for dt, b in ((torch.float32, None), (torch.bfloat16, bias), (torch.float32, bias)):
            want = G.reference(*ops[:2], fa, *ops[2:], fb, b, dt)[0]
            y = split(dev, fa, fb, None if b is None else b.to(DEV), dt, S, n)
            assert G.same(y, want), (fa, fb, M, N, K, S, dt)


def _descriptor(fa, fb, ptrs, bias, y, dt, M, N, K, S, ws, ws_bytes):
    a = _hip.MxMatmulSplitkArgs()
    a.struct_size = ctypes.sizeof(a)
    a.a_format, a.b_format = _hip.MX_FORMATS.index(fa), _hip.MX_FORMATS.index(fb)
    a.a_codes, a.a_scales, a.b_codes, a.b_scales = ptrs
    a.bias, a.y, a.ydt = bias, y.data_ptr(), _hip._DT[dt]
    a.M, a.N, a.K = M, N, K
    a.stream = _hip._stream(y)
    a.split_k, a.workspace, a.workspace_bytes = S, ws, ws_bytes
    return a


def test_workspace_contents_do_not_matter_and_hold_the_partials():
    lib = _hip.load()
    fa, fb = "mxfp4_e2m1", "mxfp8_e5m2"
    for M, N, K, S, off in CASES[:5]:
        g = torch.Generator().manual_seed(M + N + K)
        dev = on_device(random_operand(g, M, K, fa) + random_operand(g, N, K, fb), off)
        bias = torch.randn(N, generator=g).to(DEV)
        n, ranges = slicing(K, S)
        want = split(dev, fa, fb, bias, torch.float32, S, n)
        ps = partials(dev, fa, fb, ranges)
        ws = torch.full((n * M * N * 4,), 0xFF, dtype=torch.uint8, device=DEV)            # every float a NaN
        ys = []
        for _ in range(2):
            y = torch.empty(M, N, device=DEV)
            a = _descriptor(fa, fb, [t.data_ptr() for t in dev], bias.data_ptr(), y, torch.float32, M, N, K, S, ws.data_ptr(), ws.numel())
            assert lib.qs_mx_matmul_splitk_v(ctypes.byref(a)) == 0
            ys.append(y)
        torch.cuda.synchronize()
        assert G.same(ys[0], want) and G.same(ys[1], want) and not ys[0].isnan().any()
        # every partial the reduction read was written by the first launch: the planes ARE the unsplit products of the slices
        planes = ws.view(torch.float32).view(n, M, N)
        assert all(torch.equal(planes[s].view(torch.int32), ps[s].view(torch.int32)) for s in range(n)), (M, N, K, S)


@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_margins_survive(fa, fb, out_dtype):
    """the five operands, y and the workspace carved out of pattern-filled allocations (tests/test_mx_gemm_canary_gpu.py): margins
    intact, inputs unchanged, nothing written past S' M N 4 bytes of the workspace, the body equal to the CPU reference"""
    lib = _hip.load()
    osz = torch.empty(0, dtype=out_dtype).element_size()
    for M, N, K, S, off in CASES[1:5] + CASES[6:]:
        g = torch.Generator().manual_seed(M * 1000 + N + K)
        ra, rb = G.scale_windows(K, fa, fb)
        G.assert_exact_class(K, fa, fb, ra, rb)
        ops = G.exact_operand(g, M, K, fa, ra) + G.exact_operand(g, N, K, fb, rb)
        bias = torch.randint(-16, 16, (N,), generator=g).float()
        guarded = []
        for t in ops:
            raw, body = _guarded(t.numel(), off)
            body.copy_(t.reshape(-1).to(DEV))
            guarded.append((raw, body, t.numel(), off))
        braw, bbody = _guarded(N * 4)
        bbody.copy_(bias.view(torch.uint8).to(DEV))
        yoff = osz if off else 0
        yraw, ybody = _guarded(M * N * osz, yoff)
        n = slicing(K, S)[0]
        wraw, wbody = _guarded(n * M * N * 4)
        assert wbody.data_ptr() % 16 == 0
        a = _descriptor(fa, fb, [b.data_ptr() for _, b, _, _ in guarded], bbody.data_ptr(), ybody, out_dtype, M, N, K, S, wbody.data_ptr(),
                        wbody.numel())
        what = (fa, fb, out_dtype, M, N, K, S, off)
        assert lib.qs_mx_matmul_splitk_route(ctypes.byref(a)) == (PLAIN if K % 16 or off else VEC), what
        assert lib.qs_mx_matmul_splitk_v(ctypes.byref(a)) == 0, what
        torch.cuda.synchronize()
        assert _intact(yraw, M * N * osz, yoff), ("y", what)
        assert _intact(wraw, n * M * N * 4), ("workspace", what)
        for name, (raw, body, nb, o), t in zip(("a_codes", "a_scales", "b_codes", "b_scales"), guarded, ops):
            assert _intact(raw, nb, o) and torch.equal(body.cpu(), t.reshape(-1)), (name, what)
        assert _intact(braw, N * 4) and torch.equal(bbody.cpu().view(torch.float32), bias), ("bias", what)
        want = G.reference(*ops[:2], fa, *ops[2:], fb, bias, out_dtype)[0]
        assert G.same(ybody.clone().view(out_dtype).view(M, N), want), what


def test_ff_scale_byte_in_the_second_slice():
    fa, fb = "mxfp8_e4m3", "mxfp6_e2m3"
    M, N, K, S = 130, 67, 1000, 3
    g = torch.Generator().manual_seed(3)
    ops = random_operand(g, M, K, fa) + random_operand(g, N, K, fb)
    n, ranges = slicing(K, S)
    clean = split(on_device(ops, 0), fa, fb, None, torch.float32, S, n)
    row, block = 77, 15
    assert ranges[1][0] <= 32 * block < ranges[1][1]
    ops[1][row, block] = 0xFF
    y = split(on_device(ops, 0), fa, fb, None, torch.float32, S, n)
    assert bool(y[row].isnan().all()) and not clean.isnan().any()
    keep = torch.arange(M, device=DEV) != row
    assert torch.equal(y[keep].view(torch.int32), clean[keep].view(torch.int32))


FX, FW, FG = "mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2"


def _step(x, w, b, dy, **kw):
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = mx_linear(xd, wd, bd, FX, FW, FG, **kw)
    y.backward(dy.to(DEV))
    return y.detach(), xd.grad, wd.grad, _hip.mx_gemm_last_split        # (the weight gradient is the backward's last product)


def _train_case(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    return (torch.randn(M, K, generator=g) * 2, torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g),
            torch.randn(M, N, generator=g) / N)


def test_training_with_a_split_weight_gradient():
    M, N, K = 640, 70, 90
    x, w, b, dy = _train_case(M, N, K)
    y1, dx1, dw1, s1 = _step(x, w, b, dy, wgrad_split_k=1)
    y3, dx3, dw3, s3 = _step(x, w, b, dy, wgrad_split_k=3)
    assert (s1, s3) == (1, 3) and torch.equal(y1, y3) and torch.equal(dx1, dx3)
    _, _, g_col, g_cs = mx_quantize_2way(dy.to(DEV), None, FG)
    _, _, x_col, x_cs = mx_quantize_2way(x.to(DEV), None, FX)
    assert torch.equal(dw3, mx_matmul(g_col, g_cs, FG, x_col, x_cs, FX, None, torch.float32, split_k=3))
    # the project's bound for a float32 output at contraction length L >= 512 (tests/test_mx_train_gpu.py): 2 L 2^-23 S + ulp
    _, y64, S = G.reference(g_col.cpu(), g_cs.cpu(), FG, x_col.cpu(), x_cs.cpu(), FX)
    ok, ratio = G.within(dw3, y64, 2 * M * 2.0 ** -23 * S + G.ulp(y64, torch.float32))
    print("dW, split 3, largest |err| / bound", ratio)
    assert ok, ratio


def test_training_default_splits_a_long_weight_gradient():
    M, N, K = 4096, 128, 128
    x, w, b, dy = _train_case(M, N, K)
    want = _hip.mx_split_plan(N, K, M, 0)[0]
    assert want > 1
    _, _, dw, s = _step(x, w, b, dy)
    assert s == want
    _, _, g_col, g_cs = mx_quantize_2way(dy.to(DEV), None, FG)
    _, _, x_col, x_cs = mx_quantize_2way(x.to(DEV), None, FX)
    assert torch.equal(dw, mx_matmul(g_col, g_cs, FG, x_col, x_cs, FX, None, torch.float32, split_k=want))
    assert torch.equal(dw, mx_matmul(g_col, g_cs, FG, x_col, x_cs, FX, None, torch.float32, split_k="auto"))


def test_graph_capture_replays_bit_for_bit():
    """both launches go to the capturing stream, one after the other (a linear graph: nothing forks), and the workspace comes from the
    graph's pool"""
    fa, fb = "mxfp8_e4m3", "mxfp4_e2m1"
    M, N, K = 128, 128, 256
    g = torch.Generator().manual_seed(11)
    sets = [on_device(random_operand(g, M, K, fa) + random_operand(g, N, K, fb), 0) for _ in range(3)]
    step = lambda ops: mx_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, None, torch.bfloat16, split_k=2)
    eager = [step(ops).clone() for ops in sets]
    static = tuple(t.clone() for t in sets[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = step(static)
    assert _hip.mx_gemm_last_split == 2
    for ops, want in list(zip(sets, eager))[1:]:
        for dst, src in zip(static, ops):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_y, want)
