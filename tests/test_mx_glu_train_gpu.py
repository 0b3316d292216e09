"""Training through the gated MX products on the GPU: qs_mx_glu_bwd_quant2_v, qs_mx_glu_matmul_pre_v, qs_mx_grouped_glu_matmul_pre_v,
``mx_glu_linear``, ``mx_grouped_glu_linear`` and ``MXTrainGatedMoEFeedForward``.

The reference is never the code under test: it is a composition of calls the package had before, on the same device.  For the
backward quantizer that is ``dv32``, built by ELEMENTARY torch ops with one rounding each (no ``addcmul``, no fused
``silu_backward``: ATen contracts there) in the order of include/qsparse_hip.h, followed by ``mx_quantize_2way``.  Every assertion is
equality bit for bit."""
import pytest
import torch
import torch.nn.functional as F

import mx_guard as GD
import qsparse_amd as qs
from qsparse_amd import (MXTrainGatedMoEFeedForward, MXTrainGLULinear, MXTrainGroupedGLULinear, _hip, mx_glu_backward_quantize,
                         mx_glu_deinterleave, mx_glu_interleave, mx_glu_linear, mx_glu_matmul, mx_grouped_glu_linear,
                         mx_grouped_glu_matmul, mx_grouped_matmul, mx_grouped_weight_grad, mx_matmul, mx_quantize_2way, quantize_with_mx)
from qsparse_amd._mx_common import _act
from qsparse_amd.mx_batched_train import mx_quantize_2way_batched
from qsparse_amd.mx_grouped_train import _group_membership

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMTS = _hip.MX_FORMATS
ACTS = ("silu", "gelu", "relu")
DTS = (torch.float32, torch.bfloat16, torch.float16)
VEC, PLAIN = _hip.MX_Q2_ROUTE_TILE_VEC, _hip.MX_Q2_ROUTE_TILE_PLAIN
# (T, H): two row tiles with a ragged last one, three column tiles, the PLAIN col route; VEC with a short last col block of 16; one
# row; exactly one tile
SHAPES = [(130, 96), (144, 96), (1, 32), (128, 32)]
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def same(a, b):
    """bit for bit, a NaN equal to a NaN"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    return bool(((a.view(INT[a.dtype]) == b.view(INT[b.dtype])) | (a.isnan() & b.isnan())).all())


def dv_ref(dh, v, act):
    """dv32 [T, 2 H] by elementary torch ops on the device, one rounding each, in the header's order"""
    g, u = mx_glu_deinterleave(v.to(torch.float32), dim=-1)
    d = dh.to(torch.float32)
    if act == "silu":
        s = torch.sigmoid(g)
        t = 1.0 - s
        t = g * t
        t = 1.0 + t
        da, a = s * t, F.silu(g)
    elif act == "gelu":
        da, a = torch.ops.aten.gelu_backward(torch.ones_like(g), g), F.gelu(g)
    else:
        da, a = torch.where(g > 0, torch.ones_like(g), torch.where(g != g, g, torch.zeros_like(g))), _act(g, "relu")
    dg = d * u
    dg = dg * da
    return mx_glu_interleave(dg, d * a, dim=-1).contiguous()


def inputs(seed, T, H, ddt=torch.float32, vdt=torch.float32):
    g = torch.Generator().manual_seed(seed)
    dh = (torch.randn(T, H, generator=g) * torch.logspace(-3, 1, H)).to(ddt)
    v = (torch.randn(T, 2 * H, generator=g) * 3).to(vdt)
    return dh.to(DEV), v.to(DEV)


def check_quant(dh, v, act, row_fmt, col_fmt, route=None, **sr):
    got = mx_glu_backward_quantize(dh, v, act=act, row_fmt=row_fmt, col_fmt=col_fmt, **sr)
    if route is not None:
        assert _hip.mx_glu_bwd_last_route == route
    want = mx_quantize_2way(dv_ref(dh, v, act), row_fmt, col_fmt, *(sr[k] for k in ("rounding", "seed", "step") if k in sr))
    for name, a, b in zip(("row_codes", "row_scales", "col_codes", "col_scales"), got, want):
        assert (a is None and b is None) or torch.equal(a, b), (name, act, row_fmt, col_fmt, tuple(dh.shape), dh.dtype, v.dtype, sr)
    return got


# ---- 1. the backward quantizer, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H", SHAPES)
@pytest.mark.parametrize("act", ACTS)
def test_bwd_quant_every_act_and_shape(T, H, act):
    dh, v = inputs(100 + T + H, T, H)
    got = check_quant(dh, v, act, "mxfp8_e5m2", "mxfp8_e4m3", VEC if T % 16 == 0 else PLAIN)
    assert got[0].shape == (T, 2 * H) and got[1].shape == (T, 2 * H // 32)
    assert got[2].shape == (2 * H, T) and got[3].shape == (2 * H, (T + 31) // 32)
    assert all(t.dtype == torch.uint8 for t in got)


@pytest.mark.parametrize("ddt", DTS)
@pytest.mark.parametrize("vdt", DTS)
def test_bwd_quant_input_dtypes(ddt, vdt):
    for (T, H), route in (((144, 96), VEC), ((130, 96), PLAIN)):
        dh, v = inputs(7 + T, T, H, ddt, vdt)
        for act in ACTS:
            check_quant(dh, v, act, "mxfp8_e5m2", "mxfp6_e2m3", route)


@pytest.mark.parametrize("fmt", FMTS)
def test_bwd_quant_every_format_on_each_side_and_skipped_pairs(fmt):
    dh, v = inputs(31, 144, 96, torch.bfloat16, torch.float32)
    for other in FMTS:
        check_quant(dh, v, "silu", fmt, other, VEC)
    for T, H in ((144, 96), (130, 96)):
        dh, v = inputs(32, T, H)
        got = check_quant(dh, v, "gelu", fmt, None, VEC)          # (no col pair: T % 16 does not matter)
        assert got[2] is None and got[3] is None
        got = check_quant(dh, v, "gelu", None, fmt, VEC if T % 16 == 0 else PLAIN)
        assert got[0] is None and got[1] is None


def test_bwd_quant_unaligned_bases_take_plain():
    T, H = 144, 96
    dh, v = inputs(33, T, H, torch.bfloat16, torch.bfloat16)
    raw = torch.empty(T * H + 1, dtype=torch.bfloat16, device=DEV)
    dh1 = raw[1:].view(T, H)
    dh1.copy_(dh)
    check_quant(dh1, v, "silu", "mxfp8_e5m2", "mxfp8_e5m2", PLAIN)
    raw = torch.empty(T * 2 * H + 1, dtype=torch.bfloat16, device=DEV)
    v1 = raw[1:].view(T, 2 * H)
    v1.copy_(v)
    check_quant(dh, v1, "silu", "mxfp8_e5m2", "mxfp8_e5m2", PLAIN)


@pytest.mark.parametrize("T,H", [(144, 96), (130, 96)])
def test_bwd_quant_stochastic(T, H):
    dh, v = inputs(41, T, H, torch.bfloat16, torch.float32)
    outs = []
    for s in (0, 5):
        step = torch.tensor([s], dtype=torch.int64, device=DEV)
        for fmt in ("mxfp8_e5m2", "mxfp4_e2m1"):
            outs.append(check_quant(dh, v, "silu", fmt, fmt, VEC if T % 16 == 0 else PLAIN, rounding="stochastic", seed=1234, step=step))
    assert not torch.equal(outs[1][0], outs[3][0]) and not torch.equal(outs[1][2], outs[3][2])      # another step: other words
    check_quant(dh, v, "gelu", "mxfp6_e3m2", None, rounding="stochastic", seed=9, step=None)


@pytest.mark.parametrize("act", ACTS)
def test_bwd_quant_hand_built_values(act):
    """g in +-0, +-1, +-20, +-90 (expf saturates either way), u = 0, NaN and Inf in dh, g and u"""
    T, H = 16, 32
    gs = torch.tensor([0.0, -0.0, 1.0, -1.0, 20.0, -20.0, 90.0, -90.0, 0.5, -3.0, 8.0, -8.0, 1e-30, -1e-30, 104.0, -104.0])
    g = gs.repeat(2).unsqueeze(0).repeat(T, 1)
    u = torch.linspace(-2, 2, H).unsqueeze(0).repeat(T, 1)
    d = torch.ones(T, H) * torch.tensor([1.0, -0.5]).repeat(T // 2).unsqueeze(1)
    u[1, :] = 0.0
    u[2, 3], u[3, 4], u[4, 5] = float("nan"), float("inf"), float("-inf")
    g[5, 6], g[6, 7], g[7, 8] = float("nan"), float("inf"), float("-inf")
    d[8, 9], d[9, 10], d[10, 11] = float("nan"), float("inf"), float("-inf")
    d[11, :] = 0.0
    v = mx_glu_interleave(g, u, dim=-1).to(DEV)
    for fmt in ("mxfp8_e5m2", "mxfp8_e4m3"):
        check_quant(d.to(DEV), v, act, fmt, fmt, VEC)
    # and the values themselves, not only through the quantizer's NaN / Inf block rule: the finite rows alone
    keep = torch.tensor([0, 1, 11, 12, 13, 14, 15, 0, 1, 11, 12, 13, 14, 15, 0, 1])
    check_quant(d[keep].to(DEV), v[keep.to(DEV)], act, "mxfp8_e5m2", "mxfp8_e5m2", VEC)


# ---- 2. poisoned outputs and guard bytes ------------------------------------------------------------------------------------------
# (130, 96) and (1, 32) take PLAIN; (144, 96) the VEC stores: 4 bytes of row codes, 16 of col codes with a short last block of 16
@pytest.mark.parametrize("T,H", [(130, 96), (1, 32), (144, 96)])
def test_bwd_quant_writes_its_outputs_and_nothing_else(T, H):
    dh, v = inputs(51, T, H, torch.bfloat16, torch.float32)
    nb = (T + 31) // 32
    sizes = (T * 2 * H, T * 2 * H // 32, 2 * H * T, 2 * H * nb)
    shapes = ((T, 2 * H), (T, 2 * H // 32), (2 * H, T), (2 * H, nb))
    want = mx_quantize_2way(dv_ref(dh, v, "silu"), "mxfp8_e5m2", "mxfp8_e5m2")
    for offset in (0, 1, 16):
        carved = [GD.guarded(n, offset) for n in sizes]
        out = tuple(body.view(shape) for (_, body), shape in zip(carved, shapes))
        _hip.mx_glu_bwd_quant2(dh, v, "silu", "mxfp8_e5m2", "mxfp8_e5m2", out=out)
        # (offset 0 and 16 keep col_codes 16-byte aligned: VEC where T % 16 == 0; offset 1 is PLAIN with byte stores)
        assert _hip.mx_glu_bwd_last_route == (VEC if T % 16 == 0 and offset != 1 else PLAIN)
        for (raw, body), n, w in zip(carved, sizes, want):
            assert GD.intact(raw, n, offset)
            assert torch.equal(body.view(w.shape), w)          # every byte written: the poison 0xA5 survives nowhere by accident
    # a skipped pair leaves its (ignored) buffers alone
    carved = [GD.guarded(n) for n in sizes]
    out = tuple(body.view(shape) for (_, body), shape in zip(carved, shapes))
    _hip.mx_glu_bwd_quant2(dh, v, "silu", "mxfp8_e5m2", None, out=out)
    assert _hip.mx_glu_bwd_last_route == VEC                    # (no col pair: T % 16 does not matter)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    assert GD.intact(carved[0][0], sizes[0]) and GD.intact(carved[1][0], sizes[1])
    assert bool((carved[2][0] == GD.PATTERN).all()) and bool((carved[3][0] == GD.PATTERN).all())


# ---- 3. the forward with preact_dtype ---------------------------------------------------------------------------------------------
def codes_of(x, fmt):
    return tuple(quantize_with_mx(x, fmt, -1, return_codes=True)[1:])


def product_case(seed, T, H, K, fa, fb, E=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, K, generator=g) * 2
    lead = () if E is None else (E,)
    wg, wu = torch.randn(lead + (H, K), generator=g) / K ** 0.5, torch.randn(lead + (H, K), generator=g) / K ** 0.5
    bias = mx_glu_interleave(torch.randn(lead + (H,), generator=g), torch.randn(lead + (H,), generator=g), dim=-1)
    return codes_of(x.to(DEV), fa) + codes_of(mx_glu_interleave(wg, wu).to(DEV), fb) + (bias.to(DEV),)


PRE_PAIRS = [("mxfp8_e4m3", "mxfp4_e2m1"), ("mxfp6_e2m3", "mxfp6_e3m2")]


@pytest.mark.parametrize("fa,fb", PRE_PAIRS)
@pytest.mark.parametrize("K", [160, 72])
def test_dense_forward_keeps_preactivations(fa, fb, K):
    for T, H in SHAPES:
        ops = product_case(60 + T + K, T, H, K, fa, fb)
        for bias in (ops[4], None):
            args = (ops[0], ops[1], fa, ops[2], ops[3], fb, bias)
            for vdt in DTS:
                out, v = mx_glu_matmul(*args, act="silu", preact_dtype=vdt)
                assert same(out, mx_glu_matmul(*args, act="silu")) and same(v, mx_matmul(*args, vdt))
            out, v = mx_glu_matmul(*args, torch.bfloat16, act="gelu", preact_dtype=torch.float32)
            assert same(out, mx_glu_matmul(*args, torch.bfloat16, act="gelu")) and same(v, mx_matmul(*args))
            (c, s), v = mx_glu_matmul(*args, act="relu", out_fmt="mxfp8_e4m3", preact_dtype=torch.bfloat16)
            want = mx_glu_matmul(*args, act="relu", out_fmt="mxfp8_e4m3")
            assert torch.equal(c, want[0]) and torch.equal(s, want[1]) and same(v, mx_matmul(*args, torch.bfloat16))


@pytest.mark.parametrize("fa,fb", PRE_PAIRS)
@pytest.mark.parametrize("K", [160, 72])
def test_grouped_forward_keeps_preactivations(fa, fb, K):
    T, H, E = 130, 96, 4
    ops = product_case(70 + K, T, H, K, fa, fb, E)
    # an empty group and a tail; a non-monotone entry (clamped to its predecessor)
    for ends in ([40, 40, 100, 120], [64, 20, 100, 130]):
        offs = torch.tensor(ends, dtype=torch.int32, device=DEV)
        for bias in (ops[4], None):
            args = (ops[0], ops[1], fa, ops[2], ops[3], fb, offs, bias)
            for vdt in DTS:
                out, v = mx_grouped_glu_matmul(*args, act="silu", preact_dtype=vdt)
                assert same(out, mx_grouped_glu_matmul(*args, act="silu")) and same(v, mx_grouped_matmul(*args, vdt))
            (c, s), v = mx_grouped_glu_matmul(*args, act="gelu", out_fmt="mxfp8_e4m3", preact_dtype=torch.float32)
            want = mx_grouped_glu_matmul(*args, act="gelu", out_fmt="mxfp8_e4m3")
            assert torch.equal(c, want[0]) and torch.equal(s, want[1]) and same(v, mx_grouped_matmul(*args))


def test_forward_preactivations_poisoned_and_guarded():
    T, H, K = 130, 96, 72
    fa, fb = PRE_PAIRS[0]
    ops = product_case(80, T, H, K, fa, fb)
    args = (ops[0], ops[1], fa, ops[2], ops[3], fb, ops[4])
    want_v, want_y = mx_matmul(*args, torch.bfloat16), mx_glu_matmul(*args, act="silu")
    for offset in (0, 2):
        raw_v, body_v = GD.guarded(T * 2 * H * 2, offset)
        raw_y, body_y = GD.guarded(T * H * 4, 2 * offset)
        _hip.mx_glu_matmul(*args, "silu", torch.float32, None, out=body_y.view(torch.float32), preact_dtype=torch.bfloat16,
                           v_out=body_v.view(torch.bfloat16))
        assert GD.intact(raw_v, T * 2 * H * 2, offset) and GD.intact(raw_y, T * H * 4, 2 * offset)
        assert same(body_v.view(torch.bfloat16).view(T, 2 * H), want_v) and same(body_y.view(torch.float32).view(T, H), want_y)


# ---- 4. the functions -------------------------------------------------------------------------------------------------------------
def _leaf(t):
    return t.to(DEV).requires_grad_(True)


@pytest.fixture
def quant_calls(monkeypatch):
    """the (row_fmt, col_fmt) of every launch of the backward quantizer, in order"""
    calls, real = [], _hip.mx_glu_bwd_quant2

    def spy(dh, v, act, row_fmt, col_fmt, *args, **kw):
        calls.append((row_fmt, col_fmt))
        return real(dh, v, act, row_fmt, col_fmt, *args, **kw)

    monkeypatch.setattr(_hip, "mx_glu_bwd_quant2", spy)
    return calls


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("K", [160, 72])
def test_mx_glu_linear_against_the_written_out_composition(act, K, quant_calls):
    T, H = 130, 96
    g = torch.Generator().manual_seed(90 + K)
    fx, fw, fg = "mxfp8_e4m3", "mxfp6_e3m2", "mxfp8_e5m2"
    layer = MXTrainGLULinear.from_float(torch.randn(H, K, generator=g) / K ** 0.5, torch.randn(H, K, generator=g) / K ** 0.5,
                                        torch.randn(H, generator=g), torch.randn(H, generator=g), act=act, x_fmt=fx, w_fmt=fw,
                                        grad_fmt=fg).to(DEV)
    x, dh = _leaf(torch.randn(T, K, generator=g)), torch.randn(T, H, generator=g).to(DEV)
    h = layer(x)
    assert same(h.detach(), layer.to_inference()(x.detach()))
    h.backward(dh)
    # the composition, from public calls
    w, b = layer.weight.detach(), layer.bias.detach()
    x_row, x_rs, x_col, x_cs = mx_quantize_2way(x.detach(), fx, fx)
    w_row, w_rs, w_col, w_cs = mx_quantize_2way(w, fw, fw)
    v = mx_matmul(x_row, x_rs, fx, w_row, w_rs, fw, b)
    dv = dv_ref(dh, v, act)
    g_row, g_rs, g_col, g_cs = mx_quantize_2way(dv, fg, fg)
    assert same(x.grad, mx_matmul(g_row, g_rs, fg, w_col, w_cs, fw))
    assert same(layer.weight.grad, mx_matmul(g_col, g_cs, fg, x_col, x_cs, fx, split_k="auto"))      # (mx_linear's split rule)
    assert same(layer.bias.grad, dv.sum(0, dtype=torch.float32))
    assert quant_calls == [(fg, fg)]
    # need_dx / need_dw skip their pairs -- the quantizer is launched without them, nothing is saved for them -- and the gradients
    # asked for are unchanged
    x2 = x.detach().clone()
    layer.weight.grad = None
    h2 = layer(x2)
    assert h2.grad_fn.saved_tensors[3] is None and h2.grad_fn.saved_tensors[1] is not None        # (v, x_col, x_cs, w_col, w_cs)
    h2.backward(dh)
    assert quant_calls[1:] == [(None, fg)]
    assert same(layer.weight.grad, mx_matmul(g_col, g_cs, fg, x_col, x_cs, fx, split_k="auto"))
    x3 = _leaf(x.detach().cpu())
    y = mx_glu_linear(x3, w, None, act=act, x_fmt=fx, w_fmt=fw, grad_fmt=fg)
    assert y.grad_fn.saved_tensors[1] is None and y.grad_fn.saved_tensors[3] is not None
    y.backward(dh)
    assert quant_calls[2:] == [(fg, None)]
    v0 = mx_matmul(x_row, x_rs, fx, w_row, w_rs, fw, None)
    g_row0, g_rs0, _, _ = mx_quantize_2way(dv_ref(dh, v0, act), fg, None)
    assert same(x3.grad, mx_matmul(g_row0, g_rs0, fg, w_col, w_cs, fw))


@pytest.mark.parametrize("grouped", [False, True])
def test_stochastic_rounding_repeats_and_moves_on(grouped):
    T, H, K, E = 144, 96, 160, 4
    g = torch.Generator().manual_seed(95)
    lead = (E,) if grouped else ()
    w = _leaf(torch.randn(*lead, 2 * H, K, generator=g) / K ** 0.5)
    x, dh = torch.randn(T, K, generator=g).to(DEV), torch.randn(T, H, generator=g).to(DEV)
    offs = torch.tensor([40, 40, 100, 130], dtype=torch.int32, device=DEV)

    def run(step):
        xl = x.clone().requires_grad_(True)
        w.grad = None
        kw = dict(grad_fmt="mxfp4_e2m1", grad_rounding="stochastic", seed=77, step=step)
        (mx_grouped_glu_linear(xl, w, offs, None, **kw) if grouped else mx_glu_linear(xl, w, None, **kw)).backward(dh)
        return xl.grad, w.grad

    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    a = run(step)
    assert int(step) == 1
    b = run(torch.zeros(1, dtype=torch.int64, device=DEV))
    c = run(step)
    assert int(step) == 2
    assert same(a[0], b[0]) and same(a[1], b[1])
    assert not same(a[0], c[0]) and not same(a[1], c[1])
    if grouped:         # the composition at step 0, written out: the words are those of mx_quantize_2way on dv
        fx = fw = "mxfp8_e4m3"
        x_row, x_rs, x_col, x_cs = mx_quantize_2way(x, fx, fx)
        w_row, w_rs, w_col, w_cs = mx_quantize_2way_batched(w.detach(), fw, fw)
        dv = dv_ref(dh, mx_grouped_matmul(x_row, x_rs, fx, w_row, w_rs, fw, offs, None), "silu")
        g_row, g_rs, g_col, g_cs = mx_quantize_2way(dv, "mxfp4_e2m1", "mxfp4_e2m1", "stochastic", 77,
                                                    torch.zeros(1, dtype=torch.int64, device=DEV))
        assert same(a[0], mx_grouped_matmul(g_row, g_rs, "mxfp4_e2m1", w_col, w_cs, fw, offs))
        assert same(a[1], mx_grouped_weight_grad(g_col, g_cs, "mxfp4_e2m1", x_col, x_cs, fx, offs))


@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_mx_grouped_glu_linear_against_the_written_out_composition(act, quant_calls):
    T, H, K, E = 130, 96, 72, 4
    g = torch.Generator().manual_seed(97)
    fx, fw, fg = "mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2"
    layer = MXTrainGroupedGLULinear.from_float(torch.randn(E, H, K, generator=g) / K ** 0.5, torch.randn(E, H, K, generator=g) / K ** 0.5,
                                               torch.randn(E, H, generator=g), torch.randn(E, H, generator=g), act=act, x_fmt=fx, w_fmt=fw,
                                               grad_fmt=fg).to(DEV)
    offs = torch.tensor([40, 40, 100, 120], dtype=torch.int32, device=DEV)
    x, dh = _leaf(torch.randn(T, K, generator=g)), torch.randn(T, H, generator=g).to(DEV)
    h = layer(x, offs)
    assert same(h.detach(), layer.to_inference()(x.detach(), offs))
    h.backward(dh)
    w, b = layer.weight.detach(), layer.bias.detach()
    x_row, x_rs, x_col, x_cs = mx_quantize_2way(x.detach(), fx, fx)
    w_row, w_rs, w_col, w_cs = mx_quantize_2way_batched(w, fw, fw)
    v = mx_grouped_matmul(x_row, x_rs, fx, w_row, w_rs, fw, offs, b)
    dv = dv_ref(dh, v, act)
    g_row, g_rs, g_col, g_cs = mx_quantize_2way(dv, fg, fg)
    assert same(x.grad, mx_grouped_matmul(g_row, g_rs, fg, w_col, w_cs, fw, offs))
    assert same(layer.weight.grad, mx_grouped_weight_grad(g_col, g_cs, fg, x_col, x_cs, fx, offs))
    assert same(layer.bias.grad, _group_membership(offs, T) @ dv)
    assert quant_calls == [(fg, fg)]
    # need_dw alone, need_dx alone: the other pair is neither saved nor quantized
    layer.weight.grad = None
    h2 = layer(x.detach(), offs)
    assert h2.grad_fn.saved_tensors[3] is None and h2.grad_fn.saved_tensors[1] is not None        # (v, x_col, x_cs, w_col, w_cs, offs)
    h2.backward(dh)
    assert quant_calls[1:] == [(None, fg)]
    assert same(layer.weight.grad, mx_grouped_weight_grad(g_col, g_cs, fg, x_col, x_cs, fx, offs))
    x2 = _leaf(x.detach().cpu())
    y = mx_grouped_glu_linear(x2, w, offs, b, act=act, x_fmt=fx, w_fmt=fw, grad_fmt=fg)
    assert y.grad_fn.saved_tensors[1] is None and y.grad_fn.saved_tensors[3] is not None
    y.backward(dh)
    assert quant_calls[2:] == [(fg, None)]
    assert same(x2.grad, x.grad)


# ---- 5. the mixture-of-experts block ----------------------------------------------------------------------------------------------
def _moe(seed=5, T=96, D=64, H=64, E=4, k=2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    moe = MXTrainGatedMoEFeedForward.from_float(r(E, D), r(E, H, D) / D ** 0.5, None, r(E, H, D) / D ** 0.5, None, r(E, D, H) / H ** 0.5,
                                                r(E, D), k).to(DEV)
    return moe, r(T, D).to(DEV), r(T, D).to(DEV), r(T, D).to(DEV)


def test_gated_moe_forward_equals_inference_and_gradients_repeat():
    moe, x, dy, _ = _moe()
    with torch.no_grad():
        assert same(moe(x), moe.to_inference()(x))
    grads = []
    for _ in range(2):
        moe.zero_grad(set_to_none=True)
        xl = x.clone().requires_grad_(True)
        moe(xl).backward(dy)
        grads.append([xl.grad] + [p.grad.clone() for p in moe.parameters()])
    assert all(same(a, b) for a, b in zip(*grads))
    assert all(bool(g.isfinite().all()) and bool((g != 0).any()) for g in grads[0])


def test_gated_moe_captured_step_replays_with_other_tokens():
    moe, x0, dy, x1 = _moe(6)
    params = list(moe.parameters())

    def step(x):
        y = moe(x)
        return (y,) + torch.autograd.grad(y, [x] + params, dy)

    want = [t.detach().clone() for t in step(x1.clone().requires_grad_(True))]
    static_x = x0.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up outside the capture
        step(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step(static_x)
    with torch.no_grad():
        static_x.copy_(x1)                  # other token contents: another routing, other offs
    graph.replay()
    torch.cuda.synchronize()
    assert all(same(a.detach(), b) for a, b in zip(got, want))
    with torch.no_grad():
        assert not same(moe(x0), want[0])
