"""Matrix products on MX codes on the GPU: the block-scaled MFMA kernel (qs_mx_matmul_v) against the float64 CPU reference of
tests/mx_gemm_ref.py -- bit for bit on the exact class (inputs for which every partial sum in any order is exact in float32), within
a derived bound on quantizer-produced inputs -- with the route of every launch asserted.

The general-class bound, per output element: exact products, every addition / alignment keeping at least 24 significant bits:
|y32 - y64| <= 2 K 2^-23 S + ulp_ydt(y64) (+ 2^-23 |bias|), S = sum_k |a_k b_k| in float64.  The general-class test holds the
kernel to ``mx_gemm_ref.model_bound`` as well, the bound that follows the instruction's measured accumulation and is valid at every K
(tests/test_mx_short_k_gpu.py applies it where this one is not)."""
import pytest
import torch
import torch.nn as nn

import mx_gemm_ref as G
import qsparse_amd as qs
from qsparse_amd import _hip
from qsparse_amd.mx_gemm import MXLinear, mx_matmul
from qsparse_amd.quantize import MXQuantizer, quantize_with_mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
VEC, PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN
# M, N from {1, 15, 16, 17, 127, 128, 129, 300}, K from the ragged list; between them every value of both
SHAPES = [(1, 300, 128), (15, 17, 129), (16, 128, 1000), (127, 129, 33), (300, 1, 31), (129, 16, 127), (128, 127, 32), (17, 15, 1),
          (300, 300, 256)]


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def exact_case(g, M, N, K, fa, fb):
    ra, rb = G.scale_windows(K, fa, fb)
    G.assert_exact_class(K, fa, fb, ra, rb)                 # K R_a R_b 2^(r_a + r_b) <= 2^24, before the kernel runs
    return G.exact_operand(g, M, K, fa, ra) + G.exact_operand(g, N, K, fb, rb)


def offset_by_one(t):
    """the same values on the device at a base one element past a 16-byte boundary (a slice of a larger allocation)"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() and view.is_contiguous()
    return view


def run(ops, fa, fb, route, bias=None, dt=torch.float32):
    ac, asc, bc, bsc = ops
    y = mx_matmul(ac, asc, fa, bc, bsc, fb, bias, dt)
    assert _hip.mx_gemm_last_route == route, (_hip.mx_gemm_last_route, route)
    return y


def check_exact(ops_cpu, fa, fb, route, bias=None, dt=torch.float32, ops_dev=None, what=""):
    want, _, _ = G.reference(*ops_cpu[:2], fa, *ops_cpu[2:], fb, bias, dt)
    dev = ops_dev or tuple(t.to(DEV) for t in ops_cpu)
    y = run(dev, fa, fb, route, None if bias is None else bias.to(DEV), dt)
    assert y.is_cuda and y.dtype == dt and G.same(y, want), (fa, fb, what)
    return y


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_exact_class_bit_for_bit(fa, fb):
    g = torch.Generator().manual_seed(100 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    for i, (M, N, K) in enumerate(SHAPES):
        ops = exact_case(g, M, N, K, fa, fb)
        route = VEC if K % 16 == 0 else PLAIN
        bias = torch.randint(-64, 64, (N,), generator=g).float() if i % 2 else None
        check_exact(ops, fa, fb, route, bias, what=(M, N, K))
        if i % 3 == 0:
            for dt in (torch.bfloat16, torch.float16):
                check_exact(ops, fa, fb, route, bias, dt, what=(M, N, K, dt))
    # base pointers one element past a 16-byte boundary: the byte-load kernel, also where K % 16 == 0
    ops = exact_case(g, 129, 130, 256, fa, fb)
    check_exact(ops, fa, fb, PLAIN, ops_dev=tuple(offset_by_one(t) for t in ops), what="offset bases")
    bias = torch.randint(-64, 64, (130,), generator=g).float()
    want = G.reference(*ops[:2], fa, *ops[2:], fb, bias)[0]
    y = mx_matmul(*(t.to(DEV) for t in ops[:2]), fa, *(t.to(DEV) for t in ops[2:]), fb, offset_by_one(bias))      # (float32: 4 bytes past)
    assert _hip.mx_gemm_last_route == VEC and G.same(y, want)


@pytest.mark.parametrize("fa,fb,K", [("mxfp4_e2m1", "mxfp4_e2m1", 4096), ("mxfp6_e2m3", "mxfp6_e2m3", 1024), ("mxfp8_e4m3", "mxfp8_e4m3", 8192),
                                     ("mxfp8_e4m3", "mxfp4_e2m1", 4096), ("mxfp6_e3m2", "mxfp8_e5m2", 4096)])
def test_exact_class_long_k(fa, fb, K):
    g = torch.Generator().manual_seed(K)
    ops = exact_case(g, 260, 200, K, fa, fb)
    check_exact(ops, fa, fb, VEC, what=K)


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_identity_against_an_asymmetric_matrix(fa, fb):
    """A = identity (code of 1.0 on the diagonal, scale 2^0): y must be B^T -- a transposed write of C cannot pass"""
    g = torch.Generator().manual_seed(3)
    K = 160
    one = int((G.table(fa)[: 1 << G.WIDTH[fa]] == 1.0).nonzero()[0])
    ac = torch.zeros(K, K, dtype=torch.uint8)
    ac[torch.arange(K), torch.arange(K)] = one
    asc = torch.full((K, 5), 127, dtype=torch.uint8)
    bc, bsc = G.exact_operand(g, 200, K, fb, 3)
    y = check_exact((ac, asc, bc, bsc), fa, fb, VEC)
    vb = G.values(bc, bsc, fb)
    assert torch.equal(y.cpu().double(), vb.t()) and not torch.equal(vb[:K, :K], vb[:K, :K].t())


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_ff_scale_bytes_give_nan_in_their_rows_and_columns_only(fa, fb):
    g = torch.Generator().manual_seed(9)
    for M, N, K, route in ((140, 150, 256, VEC), (33, 70, 100, PLAIN)):
        base = exact_case(g, M, N, K, fa, fb)
        for in_a, in_b in ((True, False), (False, True), (True, True)):
            ac, asc, bc, bsc = (t.clone() for t in base)
            nan = torch.zeros(M, N, dtype=torch.bool)
            if in_a:
                asc[5, 0], asc[M - 1, asc.shape[1] - 1] = 255, 255
                ac[5, :32] = 0                                              # (as the quantizer writes such a block)
                nan[5, :], nan[M - 1, :] = True, True
            if in_b:
                bsc[0, 1], bsc[N - 2, 0] = 255, 255
                bc[0, 32:64] = 0
                nan[:, 0], nan[:, N - 2] = True, True
            y = check_exact((ac, asc, bc, bsc), fa, fb, route, what=("0xFF", in_a, in_b))
            assert torch.equal(y.isnan().cpu(), nan)


def test_non_default_stream():
    g = torch.Generator().manual_seed(5)
    fa, fb = "mxfp8_e4m3", "mxfp4_e2m1"
    ops = exact_case(g, 200, 136, 512, fa, fb)
    dev = tuple(t.to(DEV) for t in ops)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = run(dev, fa, fb, VEC)
    s.synchronize()
    assert G.same(y, G.reference(*ops[:2], fa, *ops[2:], fb)[0])


def quantized_case(g, M, N, K, fa, fb):
    """codes and scales as the GPU quantizer writes them, from randn activations and randn / sqrt(K) weights"""
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    _, ac, asc = quantize_with_mx(x.to(DEV), fa, -1, return_codes=True)
    _, bc, bsc = quantize_with_mx(w.to(DEV), fb, -1, return_codes=True)
    return ac, asc, bc, bsc


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_general_class_within_the_derived_bound(fa, fb):
    g = torch.Generator().manual_seed(40 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    shapes = [(130, 140, 768, VEC), (70, 65, 1000, PLAIN)] + ([(96, 80, 8192, VEC)] if fa == fb or "mxfp8_e4m3" in (fa, fb) else [])
    for M, N, K, route in shapes:
        dev = quantized_case(g, M, N, K, fa, fb)
        cpu = tuple(t.cpu() for t in dev)
        bias = torch.randn(N, generator=g)
        inside = None
        for dt, b in ((torch.float32, None), (torch.bfloat16, bias), (torch.float32, bias), (torch.float16, None)):
            _, y64, S = G.reference(*cpu[:2], fa, *cpu[2:], fb, b, dt)
            y = run(dev, fa, fb, route, None if b is None else b.to(DEV), dt)
            bound = 2 * K * 2.0 ** -23 * S + G.ulp(y64, dt) + (0 if b is None else 2.0 ** -23 * b.abs().double())
            ok, ratio = G.within(y, y64, bound)
            print(fa, fb, (M, N, K), dt, "largest |err| / bound", ratio)
            assert ok, ((M, N, K), dt, ratio)
            if M * N * K <= 1.5 * 10 ** 7:                    # the products are materialised in float64, once per shape: (130, 140, 768)
                # on the VEC route is 112 MB, (70, 65, 1000) on the PLAIN one 36 MB; the K = 8192 shape (63 M products) stays with
                # the bound above alone
                inside = G.inside_groups(*cpu[:2], fa, *cpu[2:], fb) if inside is None else inside
                ok, ratio = G.within(y, y64, G.model_bound(*cpu[:2], fa, *cpu[2:], fb, y64, S, b, dt, inside=inside))
                print(fa, fb, (M, N, K), dt, "largest |err| / model bound", ratio)
                assert ok, ("model bound", (M, N, K), dt, ratio)


@pytest.mark.parametrize("fa,fb", [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp6_e2m3"), ("mxfp8_e5m2", "mxfp4_e2m1")])
def test_cpu_path_equals_gpu_path_on_the_exact_class(fa, fb):
    g = torch.Generator().manual_seed(77)
    for M, N, K in ((130, 129, 256), (40, 50, 100)):
        ops = exact_case(g, M, N, K, fa, fb)
        bias = torch.randint(-8, 8, (N,), generator=g).float()
        for dt in (torch.float32, torch.bfloat16):
            cpu = mx_matmul(*ops[:2], fa, *ops[2:], fb, bias, dt)
            gpu = mx_matmul(*(t.to(DEV) for t in ops[:2]), fa, *(t.to(DEV) for t in ops[2:]), fb, bias.to(DEV), dt)
            assert torch.equal(cpu, gpu.cpu())
    with pytest.raises(ValueError, match="is on"):
        mx_matmul(ops[0].to(DEV), ops[1].to(DEV), fa, ops[2], ops[3], fb)


@pytest.mark.parametrize("wfmt,afmt", [("mxfp4_e2m1", "mxfp8_e4m3"), ("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4_e2m1")])
def test_mxlinear_on_the_gpu_against_the_cpu(wfmt, afmt):
    torch.manual_seed(2)
    K, N = 200, 96
    layer = qs.quantize(nn.Linear(K, N), bits=G.WIDTH[wfmt], timeout=1, callback=MXQuantizer(wfmt, block_dim=1)).train()
    layer(torch.randn(3, K)), layer(torch.randn(3, K))
    cpu = MXLinear.from_quantized(layer.eval(), afmt)
    gpu = MXLinear.from_quantized(layer, afmt).to(DEV)
    assert gpu.weight_codes.is_cuda and torch.equal(gpu.weight_codes.cpu(), cpu.weight_codes)
    x = torch.randn(4, 37, K) * 2
    yc, yg = cpu(x), gpu(x.to(DEV))
    assert _hip.mx_gemm_last_route == PLAIN and yg.shape == (4, 37, N) and not yg.requires_grad          # K = 200: K % 16 != 0
    _, ac, asc = quantize_with_mx(x, afmt, -1, return_codes=True)
    _, y64, S = G.reference(ac.reshape(-1, K), asc.reshape(-1, asc.shape[-1]), afmt, cpu.weight_codes, cpu.weight_scales, wfmt, cpu.bias)
    bound = 2 * K * 2.0 ** -23 * S + G.ulp(y64, torch.float32) + 2.0 ** -23 * cpu.bias.abs().double()
    assert G.within(yg.reshape(-1, N), y64, bound)[0] and G.within(yc.reshape(-1, N), y64, bound)[0]
    from_gpu_layer = MXLinear.from_quantized(layer.to(DEV), afmt)                                        # built on the device
    assert torch.equal(from_gpu_layer.weight_codes.cpu(), cpu.weight_codes) and torch.equal(from_gpu_layer(x.to(DEV)), yg)
    with pytest.raises(RuntimeError, match="requires grad"):
        gpu(x.to(DEV).requires_grad_(True))


def test_graph_capture_of_quantize_then_matmul_replays_bit_for_bit():
    g = torch.Generator().manual_seed(11)
    fa, fb = "mxfp8_e4m3", "mxfp4_e2m1"
    M, N, K = 256, 384, 768
    _, bc, bsc = quantize_with_mx((torch.randn(N, K, generator=g) / K ** 0.5).to(DEV), fb, -1, return_codes=True)
    bias = torch.randn(N, generator=g).to(DEV)
    xs = [torch.randn(M, K, generator=g).bfloat16().to(DEV) for _ in range(3)]

    def step(x):
        _, ac, asc = quantize_with_mx(x, fa, -1, return_codes=True)
        return mx_matmul(ac, asc, fa, bc, bsc, fb, bias, torch.bfloat16)

    eager = [step(x).clone() for x in xs]
    static_x = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = step(static_x)
    for x, want in zip(xs, eager):
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_y, want)
