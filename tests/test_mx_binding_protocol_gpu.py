"""The protocol every MX binding of ``qsparse_amd/_hip.py`` keeps around its ``qs_mx_*_v`` entry point, binding by binding: the event
log's key ``f"{label}[{route}]"`` and its algorithmic bytes, the empty problem (documented empty outputs, nothing logged, the
``*_last_route`` global ``None``), and the global after a call the entry point refuses on the host.

The shapes are the smallest at which a swapped or forgotten field still shows: one tile, one K step, every extent distinct.  The bytes
of an entry are summed here from the tensors the test passed and the tensors the binding returned; the workspace of a split product
counts twice (written, then read).

The refused call is an ``out`` that shares bytes with an input.  Six entry points check that on the host and return ``QS_ERR_ARG``
before anything is enqueued: the four codes-out products and the two gated ones.  The other five bindings with an ``out=`` (``mx_bmm``,
``mx_grouped_matmul``, ``mx_grouped_wgrad``, ``mx_glu_bwd_quant2``, ``mx_quant2_batched``) have entry points without an overlap check:
an aliasing ``out`` would be launched there, a kernel racing with itself, so they have no refused case here.  Nothing in this file
provokes a device fault."""
import pytest
import torch

from qsparse_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, N, K = 48, 32, 64                                # dense: one tile, one K step
H = 32                                              # gated: b_codes has 2 H rows
G = 2                                               # batched
T, E, OFFS = 40, 3, [16, 16, 33]                    # grouped: an empty group, a tail that reaches nothing
CB, CH, CW, CC, COUT, KH, KW = 1, 5, 6, 32, 16, 3, 2
OH, OW = CH - KH + 1, CW - KW + 1                   # stride 1, no padding: 3 x 5
R, C = 40, 64                                       # the two-way quantizers
FA, FB, FO = "mxfp8_e4m3", "mxfp6_e2m3", "mxfp4_e2m1"
ONE = (1, 1)


def kb(n):
    return (n + _hip.MX_BLOCK - 1) // _hip.MX_BLOCK


def codes(*shape):
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV)


def scales(*shape):
    return torch.randint(120, 135, shape, dtype=torch.uint8, device=DEV)


def pair(*shape):
    """codes of `shape` and their scale bytes, blocks along the last axis"""
    return codes(*shape), scales(*shape[:-1], kb(shape[-1]))


def f32(*shape):
    return torch.randn(shape, device=DEV)


def offs():
    return torch.tensor(OFFS, dtype=torch.int32, device=DEV)


def flat(res):
    """the tensors of a binding's return value, in order, a None kept"""
    if isinstance(res, (tuple, list)):
        return [t for r in res for t in flat(r)]
    return [res]


def nbytes(tensors):
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


class Case:
    """one binding: `make(empty)` -> (call, the data tensors it passes, the shapes of what it returns, extra bytes of the log entry)"""

    def __init__(self, label, glob, make, alias=None, split=None):
        self.label, self.glob, self.make, self.alias, self.split = label, glob, make, alias, split


def _matmul(empty, k=K, split_k=1):
    m = 0 if empty else M
    (a, a_s), (b, b_s), bias = pair(m, k), pair(N, k), f32(N)
    extra = 0 if split_k == 1 else 2 * _hip.mx_split_plan(m, N, k, split_k)[1] if m else 0
    return (lambda: _hip.mx_matmul(a, a_s, FA, b, b_s, FB, bias, torch.bfloat16, split_k=split_k)), [a, a_s, b, b_s, bias], [(m, N)], extra


def _matmul_q(empty, out=None):
    m = 0 if empty else M
    (a, a_s), (b, b_s), bias = pair(m, K), pair(N, K), f32(N)
    if out == "alias":
        out = (a.view(-1)[:m * N], scales(m, kb(N)))
    return (lambda: _hip.mx_matmul_q(a, a_s, FA, b, b_s, FB, bias, FO, "relu", out)), [a, a_s, b, b_s, bias], [(m, N), (m, kb(N))], 0


def _bmm(empty):
    g = 0 if empty else G
    (a, a_s), (b, b_s) = pair(g, M, K), pair(g, N, K)
    return (lambda: _hip.mx_bmm(a, a_s, FA, b, b_s, FB, None, torch.float16)), [a, a_s, b, b_s], [(g, M, N)], 0


def _bmm_q(empty, out=None):
    g = 0 if empty else G
    (a, a_s), (b, b_s), bias = pair(g, M, K), pair(g, N, K), f32(g, N)
    if out == "alias":
        out = (a.view(-1)[:g * M * N], scales(g, M, kb(N)))
    return (lambda: _hip.mx_bmm_q(a, a_s, FA, b, b_s, FB, bias, FO, None, out)), [a, a_s, b, b_s, bias], [(g, M, N), (g, M, kb(N))], 0


def _grouped(empty):
    t = 0 if empty else T
    (a, a_s), (b, b_s), bias, o = pair(t, K), pair(E, N, K), f32(E, N), offs()
    return (lambda: _hip.mx_grouped_matmul(a, a_s, FA, b, b_s, FB, o, bias, torch.bfloat16)), [a, a_s, b, b_s, bias], [(t, N)], 0


def _grouped_q(empty, out=None):
    t = 0 if empty else T
    (a, a_s), (b, b_s), bias, o = pair(t, K), pair(E, N, K), f32(N), offs()
    if out == "alias":
        out = (a.view(-1)[:t * N], scales(t, kb(N)))
    return ((lambda: _hip.mx_grouped_matmul_q(a, a_s, FA, b, b_s, FB, o, bias, FO, "relu", out)), [a, a_s, b, b_s, bias],
            [(t, N), (t, kb(N))], 0)


def _glu_options(kind, rows):
    """keywords and result shapes of the three forms of a gated product: float y, codes, float y with the pre-activations kept"""
    if kind == "codes":
        return dict(out_fmt=FO), [(rows, H), (rows, H // 32)]
    if kind == "pre":
        return dict(out_dtype=torch.bfloat16, preact_dtype=torch.float16), [(rows, H), (rows, 2 * H)]
    return dict(out_dtype=torch.float32), [(rows, H)]


def _glu(kind):
    def make(empty, out=None):
        m = 0 if empty else M
        kw, shapes = _glu_options(kind, m)
        (b, b_s), bias = pair(2 * H, K), f32(2 * H)
        if out == "alias":         # a float32 y [M, H] over the bytes a_codes [M, K] starts in
            buf = codes(m * H * 4)
            a, a_s, out = buf[:m * K].view(m, K), scales(m, kb(K)), buf.view(torch.float32)
        else:
            a, a_s = pair(m, K)
        return (lambda: _hip.mx_glu_matmul(a, a_s, FA, b, b_s, FB, bias, "silu", out=out, **kw)), [a, a_s, b, b_s, bias], shapes, 0
    return make


def _grouped_glu(kind):
    def make(empty, out=None):
        t = 0 if empty else T
        kw, shapes = _glu_options(kind, t)
        (a, a_s), (b, b_s), bias, o = pair(t, K), pair(E, 2 * H, K), f32(E, 2 * H), offs()
        if out == "alias":
            out = (a.view(-1)[:t * H], scales(t, H // 32))
        return ((lambda: _hip.mx_grouped_glu_matmul(a, a_s, FA, b, b_s, FB, o, bias, "gelu", out=out, **kw)), [a, a_s, b, b_s, bias],
                shapes, 0)
    return make


def _glu_bwd(empty):
    t = 0 if empty else R
    dh, v = f32(t, H).bfloat16(), f32(t, 2 * H)
    return ((lambda: _hip.mx_glu_bwd_quant2(dh, v, "silu", FA, FB)), [dh, v],
            [(t, 2 * H), (t, kb(2 * H)), (2 * H, t), (2 * H, kb(t))], 0)


def _grouped_wgrad(empty):
    n = 0 if empty else N
    (gt, gt_s), (xt, xt_s), o = pair(n, T), pair(K, T), offs()
    return (lambda: _hip.mx_grouped_wgrad(gt, gt_s, FA, xt, xt_s, FB, o, torch.bfloat16)), [gt, gt_s, xt, xt_s], [(E, n, K)], 0


def _conv_operands(b):
    return pair(b, CH, CW, CC), pair(COUT, KH, KW, CC), f32(COUT)


def _conv(empty):
    b = 0 if empty else CB
    (x, x_s), (w, w_s), bias = _conv_operands(b)
    return ((lambda: _hip.mx_conv2d(x, x_s, FA, w, w_s, FB, bias, ONE, (0, 0), ONE, torch.bfloat16)), [x, x_s, w, w_s, bias],
            [(b, OH, OW, COUT)], 0)


def _conv_q(empty, out=None):
    b = 0 if empty else CB
    (x, x_s), (w, w_s), bias = _conv_operands(b)
    if out == "alias":
        out = (x.view(-1)[:b * OH * OW * COUT], scales(b, OH, OW, kb(COUT)))
    return ((lambda: _hip.mx_conv2d_q(x, x_s, FA, w, w_s, FB, bias, ONE, (0, 0), ONE, FO, "relu", out)), [x, x_s, w, w_s, bias],
            [(b, OH, OW, COUT), (b, OH, OW, kb(COUT))], 0)


def _conv_transpose(empty):
    b = 0 if empty else CB
    (x, x_s), (w, w_s), bias = _conv_operands(b)
    size = (CH - 1 + KH, (CW - 1) * 2 + KW)         # stride (1, 2): 7 x 12
    return ((lambda: _hip.mx_conv_transpose2d(x, x_s, FA, w, w_s, FB, bias, (1, 2), (0, 0), (0, 0), ONE, torch.float16)),
            [x, x_s, w, w_s, bias], [(b,) + size + (COUT,)], 0)


def _conv_wgrad(empty):
    cout = 0 if empty else COUT
    (dyt, dyt_s), (xt, xt_s) = pair(OH, OW, cout, CB), pair(CH, CW, CC, CB)
    extra = 2 * _hip.mx_conv_wgrad_plan(cout, KH * KW * CC, OH * OW * _hip.MX_BLOCK, 0)[1] if cout else 0
    return ((lambda: _hip.mx_conv2d_wgrad(dyt, dyt_s, FA, xt, xt_s, FB, (KH, KW), ONE, (0, 0), ONE, torch.float32)),
            [dyt, dyt_s, xt, xt_s], [(cout, KH, KW, CC)], extra)


def _quant2(col_fmt):
    def make(empty):
        r = 0 if empty else R
        x = f32(r, C)
        col = [(C, r), (C, kb(r))] if col_fmt is not None else [None, None]
        return (lambda: _hip.mx_quant2(x, FA, col_fmt)), [x], [(r, C), (r, kb(C))] + col, 0
    return make


def _quant2_batched(empty):
    g = 0 if empty else G
    x = f32(g, R, C).half()
    return ((lambda: _hip.mx_quant2_batched(x, 1, g, R, C, (0, R * C, C), FA, FB)), [x],
            [(g, R, C), (g, R, kb(C)), (g, C, R), (g, C, kb(R))], 0)


def _quant_fwd(empty):
    r = 0 if empty else R
    x = f32(r, C)
    return (lambda: _hip.mx_quant_fwd(x, FA, -1, want_codes=True)), [x], [(r, C), (r, C), (r, kb(C))], 0


CASES = {
    "mx_matmul": Case("mx_matmul", "mx_gemm_last_route", _matmul, split=("mx_gemm_last_split", 1)),
    "mx_matmul_splitk": Case("mx_matmul_splitk", "mx_gemm_last_route", lambda empty: _matmul(empty, 4 * 128, 2),
                             split=("mx_gemm_last_split", 2)),
    "mx_matmul_q": Case("mx_matmul_q", "mx_gemm_q_last_route", _matmul_q, alias=True),
    "mx_bmm": Case("mx_bmm", "mx_bmm_last_route", _bmm),
    "mx_bmm_q": Case("mx_bmm_q", "mx_bmm_q_last_route", _bmm_q, alias=True),
    "mx_grouped_matmul": Case("mx_grouped_matmul", "mx_grouped_last_route", _grouped),
    "mx_grouped_matmul_q": Case("mx_grouped_matmul_q", "mx_grouped_q_last_route", _grouped_q, alias=True),
    "mx_glu_matmul": Case("mx_glu_matmul", "mx_glu_last_route", _glu("float"), alias=True),
    "mx_glu_matmul_codes": Case("mx_glu_matmul", "mx_glu_last_route", _glu("codes")),
    "mx_glu_matmul_pre": Case("mx_glu_matmul_pre", "mx_glu_last_route", _glu("pre")),
    "mx_grouped_glu_matmul": Case("mx_grouped_glu_matmul", "mx_grouped_glu_last_route", _grouped_glu("float")),
    "mx_grouped_glu_matmul_codes": Case("mx_grouped_glu_matmul", "mx_grouped_glu_last_route", _grouped_glu("codes"), alias=True),
    "mx_grouped_glu_matmul_pre": Case("mx_grouped_glu_matmul_pre", "mx_grouped_glu_last_route", _grouped_glu("pre")),
    "mx_glu_bwd_quant2": Case("mx_glu_bwd_quant2", "mx_glu_bwd_last_route", _glu_bwd),
    "mx_grouped_wgrad": Case("mx_grouped_wgrad", "mx_grouped_wgrad_last_route", _grouped_wgrad),
    "mx_conv2d": Case("mx_conv2d", "mx_conv_last_route", _conv),
    "mx_conv2d_q": Case("mx_conv2d_q", "mx_conv_q_last_route", _conv_q, alias=True),
    "mx_conv_transpose2d": Case("mx_conv_transpose2d", "mx_conv_transpose_last_route", _conv_transpose),
    "mx_conv2d_wgrad": Case("mx_conv2d_wgrad", "mx_conv_wgrad_last_route", _conv_wgrad, split=("mx_conv_wgrad_last_split", 1)),
    "mx_quant2": Case("mx_quant2", "mx_quant2_last_route", _quant2(FB)),
    "mx_quant2_row_only": Case("mx_quant2", "mx_quant2_last_route", _quant2(None)),
    "mx_quant2_batched": Case("mx_quant2_batched", "mx_quant2_batched_last_route", _quant2_batched),
    "mx_quant_fwd": Case("mx_quant_fwd", "mx_last_route", _quant_fwd),
}


@pytest.fixture(autouse=True)
def _seeded():
    torch.manual_seed(0)
    yield
    _hip.take_event_pairs()        # (a failed case leaves no log running)


def check_shapes(res, shapes):
    got = flat(res)
    assert len(got) == len(shapes)
    for t, shape in zip(got, shapes):
        assert (t is None) == (shape is None)
        assert t is None or tuple(t.shape) == tuple(shape), (tuple(t.shape), shape)


@pytest.mark.parametrize("name", list(CASES))
def test_event_log(name):
    """(a) one entry, keyed by the label and the route the global reports, with the bytes of the operands passed and returned"""
    case = CASES[name]
    call, inputs, shapes, extra = case.make(False)
    setattr(_hip, case.glob, "stale")
    _hip.start_event_log()
    res = call()
    log = _hip.stop_event_log(with_bytes=True)
    route = getattr(_hip, case.glob)
    assert isinstance(route, int) and route > 0
    check_shapes(res, shapes)
    assert list(log) == [f"{case.label}[{route}]"]
    (_, logged), = log[f"{case.label}[{route}]"]
    print(name, "logged bytes", logged, "expected", nbytes(inputs) + nbytes(flat(res)) + extra)
    assert logged == nbytes(inputs) + nbytes(flat(res)) + extra
    if case.split is not None:
        assert getattr(_hip, case.split[0]) == case.split[1]
        assert (extra > 0) == (case.split[1] > 1)


@pytest.mark.parametrize("name", list(CASES))
def test_empty_problem(name):
    """(b) the documented empty outputs, no log entry, the route global None (the split one 1)"""
    case = CASES[name]
    call, _, shapes, _ = case.make(True)
    setattr(_hip, case.glob, "stale")
    if case.split is not None:
        setattr(_hip, case.split[0], 7)
    _hip.start_event_log()
    res = call()
    log = _hip.stop_event_log(with_bytes=True)
    check_shapes(res, shapes)
    assert any(0 in s for s in shapes if s is not None)
    assert log == {}
    assert getattr(_hip, case.glob) is None
    if case.split is not None:
        assert getattr(_hip, case.split[0]) == 1


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.alias])
def test_refused_call(name):
    """(c) an `out` that shares bytes with an input: QS_ERR_ARG from the host checks, nothing launched, the global None -- and set
    again by the next call that succeeds"""
    case = CASES[name]
    good = case.make(False)[0]
    good()
    assert getattr(_hip, case.glob) is not None
    bad = case.make(False, "alias")[0]
    with pytest.raises(_hip.QsparseHipError, match=r"_v: .*\(status -\d+\)"):
        bad()
    assert getattr(_hip, case.glob) is None
    good()
    assert isinstance(getattr(_hip, case.glob), int) and getattr(_hip, case.glob) > 0
