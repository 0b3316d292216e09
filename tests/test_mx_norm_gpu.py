"""``mx_norm.py`` on the GPU: qs_mx_norm_quant_v against the CPU path bit for bit (codes, scales, col pair, rstd, mean), its routes,
special values, two-way consistency, the layers and the training step (the checks of ``test_mx_norm.py`` on the device) and graph
capture.  The reference is the definition restated in ``mx_norm_ref.py`` and the quantizers the package had before."""
import copy

import pytest
import torch
import torch.nn as nn

import mx_norm_ref as NR
import qsparse_amd as qs
import test_mx_norm as T
from qsparse_amd import MXTrainNormLinear, _hip, mx_norm_quantize, mx_quantize_2way
from mx_norm_ref import DTS, EPS, FMTS, NORMS, WB, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_NORM_ROUTE_VEC, _hip.MX_NORM_ROUTE_PLAIN
ROWS, COLS = T.ROWS + (128, 257), T.COLS + (64, 4104)
NAMES = ("codes", "scales", "col_codes", "col_scales", "rstd", "mean")


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def dev(t):
    return None if t is None else t.to(DEV)


def agree(got, want, what):
    for name, a, r in zip(NAMES, got, want):
        assert (a is None) == (r is None), (name,) + what
        assert a is None or same(a.cpu(), r), (name,) + what


# ---- test 3: GPU against CPU, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_gpu_equals_cpu(norm, dtype):
    """every R x C x (weight, bias), the formats walking as in the CPU test; the route is VEC exactly where C % 32 == 0 (torch's
    allocations are 16-byte aligned)"""
    i = 0
    for R in ROWS:
        for C in COLS:
            for has_w, has_b in WB:
                x, w, b = NR.inputs(1000 * R + C, R, C, dtype, has_w, has_b)
                fmt, col_fmt = FMTS[i % 5], FMTS[(i + 2) % 5]
                i += 1
                want = mx_norm_quantize(x, w, b, norm=norm, eps=EPS, fmt=fmt, col_fmt=col_fmt, return_stats=True)
                got = mx_norm_quantize(dev(x), dev(w), dev(b), norm=norm, eps=EPS, fmt=fmt, col_fmt=col_fmt, return_stats=True)
                assert _hip.mx_norm_last_route == (VEC if C % 32 == 0 else PLAIN), (R, C)
                agree(got, want, (R, C, has_w, has_b, fmt, col_fmt))


@pytest.mark.parametrize("dtype", DTS, ids=str)
def test_offset_by_one_element_takes_the_plain_route(dtype):
    for norm in NORMS:
        for R, C in ((129, 96), (33, 1024), (128, 64)):
            x, w, b = NR.inputs(R + C, R, C, dtype)
            buf = torch.zeros(R * C + 1, dtype=dtype, device=DEV)
            buf[1:] = dev(x).reshape(-1)
            xo = buf[1:].view(R, C)
            wbuf = torch.zeros(C + 1, device=DEV)
            wbuf[1:] = dev(w)
            args = dict(norm=norm, eps=EPS, fmt="mxfp8_e4m3", col_fmt="mxfp6_e3m2", return_stats=True)
            want = mx_norm_quantize(dev(x), dev(w), dev(b), **args)
            assert _hip.mx_norm_last_route == VEC
            got = mx_norm_quantize(xo, dev(w), dev(b), **args)
            assert _hip.mx_norm_last_route == PLAIN
            agree(got, [t if t is None else t.cpu() for t in want], (norm, R, C, "x"))
            got = mx_norm_quantize(dev(x), wbuf[1:], dev(b), **args)
            assert _hip.mx_norm_last_route == PLAIN
            agree(got, [t if t is None else t.cpu() for t in want], (norm, R, C, "weight"))


def _special(dtype, R=70, C=96):
    x, w, b = NR.inputs(17, R, C, dtype)
    x[5, 40] = float("nan")
    x[37, 70] = float("inf")
    x[10] = 0
    x[11] = 0
    return x, w, b


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("dtype", DTS, ids=str)
def test_special_values(dtype, norm):
    """a NaN row and an Inf row are 0xFF in every block they touch and nowhere else: all three row blocks of their own row; in the col
    pair the one block of 32 rows that holds them, for every column.  All-zero rows give y = b"""
    x, w, b = _special(dtype)
    for fmt in FMTS:
        for bias in (b, None):
            want = mx_norm_quantize(x, w, bias, norm=norm, eps=EPS, fmt=fmt, col_fmt=fmt, return_stats=True)
            got = mx_norm_quantize(dev(x), dev(w), dev(bias), norm=norm, eps=EPS, fmt=fmt, col_fmt=fmt, return_stats=True)
            agree(got, want, (fmt, bias is None))
            codes, scales, cc, cs, rstd, _ = [t if t is None else t.cpu() for t in got]
            bad = torch.zeros(70, dtype=torch.bool)
            bad[5] = bad[37] = True
            assert bool((scales[bad] == 255).all()) and bool((scales[~bad] != 255).all())
            assert bool((codes[bad] == 0).all()) and bool(rstd[bad].isnan().all()) and bool(rstd[~bad].isfinite().all())
            assert bool((cs[:, :2] == 255).all()) and bool((cs[:, 2] != 255).all())           # rows 0-31, 32-63 | 64-69
            assert bool((cc[:, :64] == 0).all())
            if bias is None:
                assert bool((codes[10] == 0).all()) and bool((scales[10] == 0).all())
            else:
                rc, rs, _, _ = NR.ref_quant(b[None, :].clone(), fmt)
                assert torch.equal(codes[10:11], rc) and torch.equal(scales[10:11], rs) and torch.equal(codes[11], codes[10])


@pytest.mark.parametrize("norm", NORMS)
def test_f16_row_of_65504_and_subnormal_blocks(norm):
    R, C = 40, 128
    x, w, b = NR.inputs(23, R, C, torch.float16)
    x[3] = 65504.0
    x[4, ::2] = 65504.0
    x[4, 1::2] = -65504.0
    w[32:64] = 2.0 ** -131                      # y of the second block is a float32 subnormal in every row
    w[64:96] *= 2.0 ** -126                     # and the third straddles the smallest normal
    y = NR.ref_y(x, w, None, norm)[0]
    tiny = y[:, 32:64].abs().amax(-1)
    assert bool((tiny[4] > 0) & (tiny < 2.0 ** -126).all())
    for fmt in FMTS:
        want = mx_norm_quantize(x, w, None, norm=norm, eps=EPS, fmt=fmt, col_fmt=fmt, return_stats=True)
        got = mx_norm_quantize(dev(x), dev(w), None, norm=norm, eps=EPS, fmt=fmt, col_fmt=fmt, return_stats=True)
        agree(got, want, (fmt,))
        assert bool((got[1].cpu()[:, 1] == 0).all())                                         # the clamp at 2^-127


# ---- test 4: two-way consistency on the GPU ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
def test_two_way_consistency(norm):
    for R, C, dtype in ((257, 96, torch.bfloat16), (128, 1000, torch.float32), (33, 4104, torch.float16), (144, 64, torch.float32)):
        x, w, b = NR.inputs(R * C, R, C, dtype)
        y = NR.ref_y(x, w, b, norm)[0]
        for fmt, col_fmt in (("mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp4_e2m1", "mxfp6_e2m3")):
            two = mx_norm_quantize(dev(x), dev(w), dev(b), norm=norm, eps=EPS, fmt=fmt, col_fmt=col_fmt)
            one = mx_norm_quantize(dev(x), dev(w), dev(b), norm=norm, eps=EPS, fmt=fmt)
            _, _, cc, cs = mx_quantize_2way(dev(y), None, col_fmt)
            assert same(two[2], cc) and same(two[3], cs) and same(two[0], one[0]) and same(two[1], one[1])


# ---- tests 5 and 6 on the device ---------------------------------------------------------------------------------------------------
def test_inference_layers_gpu():
    T.check_inference_layers(DEV)
    with pytest.raises(ValueError, match="x is on cuda:0 but weight on cpu"):
        mx_norm_quantize(torch.randn(4, 32, device=DEV), torch.ones(32))


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape,N", [((2, 33, 96), 64), ((129, 128), 32)])
def test_norm_linear_gpu(shape, N, norm):
    T.check_norm_linear(DEV, shape, N, norm)


def test_norm_linear_gpu_equals_cpu_forward():
    """the forward product reads the same codes on both devices"""
    x, nw, nb, W, b, _ = T._train_case("cpu", (129, 128), 32, "layer", 9)
    args = dict(norm="layer", eps=EPS, fmt="mxfp8_e4m3", col_fmt="mxfp8_e4m3", return_stats=True)
    agree(mx_norm_quantize(dev(x), dev(nw), dev(nb), **args), mx_norm_quantize(x, nw, nb, **args), ("train",))


def test_unasked_gradients_gpu(monkeypatch):
    T.check_unasked_gradients(DEV, monkeypatch)


def test_layer_gpu():
    T.check_layer(DEV)


# ---- test 7: graph capture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
def test_captured_step_replays_bit_for_bit(norm):
    """forward and backward of one MXTrainNormLinear under torch.cuda.graph (a single layer: no parallel branches), replayed on new
    inputs"""
    g = torch.Generator().manual_seed(12)
    M, K, N = 64, 128, 64
    xs = [torch.randn(M, K, generator=g).to(DEV) for _ in range(3)]
    dys = [torch.randn(M, N, generator=g).to(DEV) for _ in range(3)]
    torch.manual_seed(0)
    fnorm = (nn.RMSNorm(K, eps=1e-5) if norm == "rms" else nn.LayerNorm(K)).to(DEV)
    init = MXTrainNormLinear.from_float(fnorm, nn.Linear(K, N).to(DEV))

    def step(layer, x, dy):
        for p in layer.parameters():
            p.grad = None
        xg = x.detach().requires_grad_(True)
        y = layer(xg)
        y.backward(dy)
        return (y.detach(), xg.grad) + tuple(p.grad for p in layer.parameters())

    eager = copy.deepcopy(init)
    want = [tuple(t.clone() for t in step(eager, x, dy)) for x, dy in zip(xs, dys)]

    layer = copy.deepcopy(init)
    static_x, static_dy = xs[0].clone(), dys[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(layer, static_x, static_dy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step(layer, static_x, static_dy)
    for x, dy, ref in zip(xs, dys, want):
        static_x.copy_(x)
        static_dy.copy_(dy)
        graph.replay()
        torch.cuda.synchronize()
        assert len(static_out) == len(ref) and all(same(a, r) for a, r in zip(static_out, ref))
