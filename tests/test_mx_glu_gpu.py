"""The gated (SwiGLU / GeGLU / ReGLU) products on MX codes on the GPU (qs_mx_glu_matmul_v, qs_mx_grouped_glu_matmul_v).

The reference is never the code under test.  It is this composition of calls the package had before, on the same device:
``mx_matmul(..., out_dtype=float32)`` on the interleaved weight (``mx_grouped_matmul`` for the grouped product),
``mx_glu_deinterleave(v, dim=-1)``, ``F.silu(g)`` / ``F.gelu(g)`` / the package's ReLU, ``* u``, then one rounding or
``quantize_with_mx(z, f, -1, return_codes=True)``.  Every assertion is equality bit for bit (``same``: a NaN equals a NaN, whose
payload no definition fixes); it rests on ATen's GPU ``silu`` / ``gelu`` evaluating the header's expressions with the same device
``expf`` / ``erff``.  Across devices equality is asserted for ``act="relu"`` alone, on operands whose products are exact."""
import pytest
import torch
import torch.nn.functional as F

import mx_gemm_ref as G
import qsparse_amd as qs
from qsparse_amd import (MXActivation, MXGatedMoEFeedForward, MXGLULinear, _hip, mx_glu_deinterleave, mx_glu_interleave, mx_glu_matmul,
                         mx_grouped_glu_matmul, mx_grouped_matmul, mx_matmul, quantize_with_mx)
from qsparse_amd._mx_common import _act
from qsparse_amd.mx_grouped import _offs_int32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMTS = G.FMTS
PAIRS = [(a, b) for a in FMTS for b in FMTS]
ACTS = ("silu", "gelu", "relu")
VEC, PLAIN = _hip.MX_GEMM_ROUTE_VEC, _hip.MX_GEMM_ROUTE_PLAIN
# (M, H, K): two row tiles with a ragged last one, a second column tile that is half empty (N = 192), two K steps with a short last
# one on the VEC route; the PLAIN route; one row; one output block
DENSE = [(130, 96, 160), (130, 96, 72), (1, 96, 160), (130, 32, 160)]
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
    both_nan = a.isnan() & b.isnan()
    return bool(((a.view(INT[a.dtype]) == b.view(INT[b.dtype])) | both_nan).all())


def codes_of(x, fmt):
    return tuple(quantize_with_mx(x, fmt, -1, return_codes=True)[1:])


def act_ref(g, act):
    return F.silu(g) if act == "silu" else F.gelu(g) if act == "gelu" else _act(g, "relu")


def epilogue_ref(v, act, out_dtype=torch.float32, out_fmt=None):
    """the reference's steps 2 - 4 on the float32 product v [rows, 2 H]"""
    g, u = mx_glu_deinterleave(v, dim=-1)
    z = act_ref(g, act) * u
    return z.to(out_dtype) if out_fmt is None else codes_of(z, out_fmt)


def check(got, want, what):
    if isinstance(want, tuple):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what
    else:
        assert same(got, want), what


def dense_case(seed, M, H, K, fa, fb):
    """(a_codes, a_scales, b_codes, b_scales, bias) on the device: gate values of a few units either side of 0, where silu and gelu bend"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 2
    wg, wu = torch.randn(H, K, generator=g) / K ** 0.5, torch.randn(H, K, generator=g) / K ** 0.5
    bias = mx_glu_interleave(torch.randn(H, generator=g), torch.randn(H, generator=g))
    return codes_of(x.to(DEV), fa) + codes_of(mx_glu_interleave(wg, wu).to(DEV), fb) + (bias.to(DEV),)


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_every_operand_pair_and_output_format(fa, fb):
    M, H, K = DENSE[0]
    ops = dense_case(900 + FMTS.index(fa) * 5 + FMTS.index(fb), M, H, K, fa, fb)
    v = mx_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, ops[4])
    check(mx_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, ops[4], act="silu"), epilogue_ref(v, "silu"), (fa, fb, "float32"))
    assert _hip.mx_glu_last_route == VEC
    for f in FMTS:
        got = mx_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, ops[4], act="silu", out_fmt=f)
        assert got[0].shape == (M, H) and got[1].shape == (M, H // 32) and got[0].dtype == got[1].dtype == torch.uint8
        check(got, epilogue_ref(v, "silu", out_fmt=f), (fa, fb, f))


@pytest.mark.parametrize("M,H,K", DENSE)
def test_every_act_and_output_at_every_shape(M, H, K):
    fa, fb = "mxfp8_e4m3", "mxfp6_e3m2"
    ops = dense_case(950 + M + H + K, M, H, K, fa, fb)
    for bias in (ops[4], None):
        v = mx_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, bias)
        for act in ACTS:
            for dt in (torch.float32, torch.bfloat16, torch.float16):
                y = mx_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, bias, dt, act=act)
                assert _hip.mx_glu_last_route == (VEC if K % 16 == 0 else PLAIN)
                assert y.shape == (M, H) and y.dtype == dt
                check(y, epilogue_ref(v, act, dt), (M, H, K, act, dt, bias is not None))
            check(mx_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, bias, act=act, out_fmt="mxfp8_e4m3"),
                  epilogue_ref(v, act, out_fmt="mxfp8_e4m3"), (M, H, K, act, "codes", bias is not None))


def offset_by_one(t):
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 1
    return view


def test_routes_are_those_of_the_ungated_codes_out_product():
    fa, fb = "mxfp8_e4m3", "mxfp4_e2m1"
    for (M, H, K), shift, route in ((DENSE[0], False, VEC), (DENSE[1], False, PLAIN), (DENSE[0], True, PLAIN)):
        ops = dense_case(7, M, H, K, fa, fb)
        if shift:
            ops = (offset_by_one(ops[0]),) + ops[1:]
        mx_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, ops[4], out_fmt="mxfp8_e4m3", act="relu")
        got = mx_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, ops[4], act="relu", out_fmt="mxfp8_e4m3")
        assert _hip.mx_glu_last_route == _hip.mx_gemm_q_last_route == route
        check(got, epilogue_ref(mx_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, ops[4]), "relu", out_fmt="mxfp8_e4m3"), (K, shift))
    empty = mx_glu_matmul(ops[0][:0], ops[1][:0], fa, ops[2], ops[3], fb, ops[4])
    assert empty.shape == (0, 96) and _hip.mx_glu_last_route is None


def test_relu_equals_the_cpu_path_on_exact_operands():
    """no transcendental: the CPU path (float64 products, rounded once) and the kernel agree where the products are exact"""
    fa, fb, (M, H, K) = "mxfp8_e4m3", "mxfp6_e2m3", DENSE[0]
    g = torch.Generator().manual_seed(11)
    ra, rb = G.scale_windows(K, fa, fb)
    G.assert_exact_class(K, fa, fb, ra, rb)
    a, b = G.exact_operand(g, M, K, fa, ra, 124), G.exact_operand(g, 2 * H, K, fb, rb, 130)
    bias = torch.randint(-64, 64, (2 * H,), generator=g).float()
    for out_fmt in (None, "mxfp8_e5m2"):
        cpu = mx_glu_matmul(a[0], a[1], fa, b[0], b[1], fb, bias, act="relu", out_fmt=out_fmt)
        dev = mx_glu_matmul(a[0].to(DEV), a[1].to(DEV), fa, b[0].to(DEV), b[1].to(DEV), fb, bias.to(DEV), act="relu", out_fmt=out_fmt)
        check(tuple(t.cpu() for t in dev) if out_fmt else dev.cpu(), cpu, out_fmt)


# ---- special values, hand-built codes: K = 32 (one block), the product of row m and weight row n is a_val[m] * w_val[n] exactly --------
GATES = (0x00, 0x80, 0x38, 0xB8, 0x7E, 0xFE, 0x30, 0xBC)          # +0, -0, 1, -1, 448, -448, 0.5, -1.5
UPS = (0x38, 0xB8, 0x7E, 0x30)                                    # 1, -1, 448, 0.5
# what row m of A is: (code at k = 0, code at k = 1, scale byte).  One in E4M3 / E5M2 is 0x38 / 0x3C
ROWS = {"mxfp8_e4m3": [(0x38, 0, 127), (0x38, 0, 134), (0xB8, 0, 134), (0x38, 0, 107), (0x38, 0, 227), (0xB8, 0, 227), (0, 0, 127),
                       (0x38, 0, 0xFF), (0x38, 0x7F, 127), (0x38, 0xFF, 127)],       # ... a zero row, a 0xFF scale, the E4M3 NaN codes
        "mxfp8_e5m2": [(0x3C, 0, 127), (0x3C, 0, 134), (0xBC, 0, 134), (0x3C, 0, 107), (0x3C, 0, 227), (0xBC, 0, 227), (0, 0, 127),
                       (0x3C, 0, 0xFF), (0x3C, 0x7C, 127), (0x3C, 0xFC, 127)]}       # ... an E5M2 +Inf code, a -Inf code
ZERO_ROW, FF_ROW, BAD_ROWS = 6, 7, (7, 8, 9)


def special_case(fa):
    H = 32
    a_codes = torch.zeros(len(ROWS[fa]), 32, dtype=torch.uint8)
    a_scales = torch.zeros(len(ROWS[fa]), 1, dtype=torch.uint8)
    for m, (c0, c1, s) in enumerate(ROWS[fa]):
        a_codes[m, 0], a_codes[m, 1], a_scales[m, 0] = c0, c1, s
    wg, wu = torch.zeros(H, 32, dtype=torch.uint8), torch.zeros(H, 32, dtype=torch.uint8)
    for t in range(H):
        wg[t, 0], wu[t, 0] = GATES[t % 8], UPS[(t // 8) % 4]
        wg[t, 1] = wu[t, 1] = 0x38          # (meets the NaN / Inf code of A at k = 1: times 0 it would be NaN either way)
    b_codes = mx_glu_interleave(wg, wu)
    return a_codes.to(DEV), a_scales.to(DEV), b_codes.to(DEV), torch.full((2 * H, 1), 127, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("fa", sorted(ROWS))
@pytest.mark.parametrize("act", ACTS)
def test_special_values(fa, act):
    """gates of +-0, +-1, +-448 under scales 2^0, 2^7 (silu(-57344) is -0), 2^-20 and 2^100 (a product beyond float32: Inf), a zero
    row, a 0xFF scale byte and NaN / Inf codes in A"""
    fb = "mxfp8_e4m3"
    ops = special_case(fa)
    v = mx_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb)
    assert v[ZERO_ROW].eq(0).all() and not v[list(BAD_ROWS)].isfinite().any() and v[:ZERO_ROW].isfinite().all()
    want = epilogue_ref(v, act)
    y = mx_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, act=act)
    check(y, want, (fa, act))
    if act != "relu":
        assert torch.signbit(want[want == 0]).any(), "the case holds a -0 result"
    for f in FMTS:
        codes, scales = mx_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, act=act, out_fmt=f)
        check((codes, scales), epilogue_ref(v, act, out_fmt=f), (fa, act, f))
        assert not codes[ZERO_ROW].any() and scales[ZERO_ROW].item() == 0, "an all-zero block: byte 0"
        for m in BAD_ROWS:
            assert not codes[m].any() and scales[m].item() == 0xFF, "a NaN block: byte 0xFF, codes 0"
        assert scales[4].item() == 0xFF, "a block that holds Inf (448 2^100 times 448 2^100): byte 0xFF"


# ---- the grouped product -----------------------------------------------------------------------------------------------------------
T, E, GH, GK = 200, 4, 96, 160
I32MIN, I32MAX = -2 ** 31, 2 ** 31 - 1
# offs and its dtype.  The first: an empty group, a group of one row, a boundary inside a tile, 11 tail rows; then the hostile ones of
# tests/test_mx_grouped_gpu.py at T = 200
OFFS = [([0, 1, 130, 189], torch.int32), ([200, 200, 200, 200], torch.int32), ([-7, 100, 99, 1000], torch.int32),
        ([I32MAX] * 4, torch.int32), ([I32MIN, 0, I32MIN, 150], torch.int32), ([2 ** 31, 0, 0, 0], torch.int64),
        ([100, 2 ** 32 + 5, 150, 2 ** 40], torch.int64), ([-2 ** 31 - 1, 50, -2 ** 63, 2 ** 63 - 1], torch.int64)]


def clamped(row, rows):
    out, c = [], 0
    for v in row:
        c = min(max(v, c), rows)
        out.append(c)
    return out


@pytest.fixture(scope="module")
def grouped_case():
    fa, fb = "mxfp8_e4m3", "mxfp4_e2m1"
    g = torch.Generator().manual_seed(77)
    x = torch.randn(T, GK, generator=g) * 2
    scale = torch.pow(2.0, torch.arange(E).float()).view(-1, 1, 1) / GK ** 0.5          # every expert its own scale
    wg, wu = torch.randn(E, GH, GK, generator=g) * scale, torch.randn(E, GH, GK, generator=g) * scale
    ops = codes_of(x.to(DEV), fa) + codes_of(mx_glu_interleave(wg, wu).to(DEV), fb)
    bias2 = mx_glu_interleave(torch.randn(E, GH, generator=g), torch.randn(E, GH, generator=g), dim=-1).to(DEV)
    return fa, fb, ops, (None, bias2[0].contiguous(), bias2)


def grouped_ref(ops, fa, fb, hand, bias, act, out_dtype=torch.float32, out_fmt=None):
    return epilogue_ref(mx_grouped_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, hand, bias), act, out_dtype, out_fmt)


@pytest.mark.parametrize("row,dtype", OFFS, ids=[str(i) for i in range(len(OFFS))])
def test_grouped_product_for_any_offs(grouped_case, row, dtype):
    fa, fb, ops, biases = grouped_case
    ends = clamped(row, T)
    offs, hand = torch.tensor(row, dtype=dtype, device=DEV), torch.tensor(ends, dtype=torch.int32, device=DEV)
    for j, act in enumerate(ACTS):
        bias = biases[(j + sum(ends)) % 3]
        y = mx_grouped_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, offs, bias, act=act)
        assert _hip.mx_grouped_glu_last_route == VEC and y.shape == (T, GH)
        check(y, grouped_ref(ops, fa, fb, hand, bias, act), (row, act, "float32"))
        assert y[ends[-1]:].eq(0).all() and not torch.signbit(y[ends[-1]:]).any(), "tail rows: +0"
        for e, (lo, hi) in enumerate(zip([0] + ends, ends)):          # a group is the dense gated product with its weight
            if hi > lo:
                be = None if bias is None else bias if bias.dim() == 1 else bias[e]
                assert same(y[lo:hi], mx_glu_matmul(ops[0][lo:hi], ops[1][lo:hi], fa, ops[2][e], ops[3][e], fb, be, act=act)), (row, e)
        codes, scales = mx_grouped_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, offs, bias, act=act, out_fmt="mxfp6_e2m3")
        check((codes, scales), grouped_ref(ops, fa, fb, hand, bias, act, out_fmt="mxfp6_e2m3"), (row, act, "codes"))
        assert not codes[ends[-1]:].any() and not scales[ends[-1]:].any(), "tail rows: code 0, byte 0"
    y16 = mx_grouped_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, offs, biases[2], torch.bfloat16, act="silu")
    check(y16, grouped_ref(ops, fa, fb, hand, biases[2], "silu", torch.bfloat16), (row, "bfloat16"))


def test_a_nan_row_stays_in_its_group(grouped_case):
    fa, fb, ops, biases = grouped_case
    offs = torch.tensor([50, 100, 150, 200], dtype=torch.int32, device=DEV)
    clean = mx_grouped_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, offs, biases[2], act="silu")
    assert clean.isfinite().all()
    a_scales = ops[1].clone()
    a_scales[60:70] = 0xFF          # ten rows of group 1
    got = mx_grouped_glu_matmul(ops[0], a_scales, fa, ops[2], ops[3], fb, offs, biases[2], act="silu")
    assert got[60:70].isnan().all()
    keep = torch.ones(T, dtype=torch.bool, device=DEV)
    keep[60:70] = False
    assert same(got[keep], clean[keep])
    codes, scales = mx_grouped_glu_matmul(ops[0], a_scales, fa, ops[2], ops[3], fb, offs, biases[2], act="silu", out_fmt="mxfp8_e4m3")
    assert scales[60:70].eq(0xFF).all() and not codes[60:70].any() and not scales[keep].eq(0xFF).any()


# ---- nothing else is written -----------------------------------------------------------------------------------------------------------
POISON, MARGIN = 0xA5, 256


def carve(nbytes):
    """a body of `nbytes` inside a poisoned allocation with a margin either side: (whole, body)"""
    whole = torch.full((nbytes + 2 * MARGIN,), POISON, dtype=torch.uint8, device=DEV)
    return whole, whole[MARGIN:MARGIN + nbytes]


def margins_intact(whole, nbytes):
    return bool(whole[:MARGIN].eq(POISON).all()) and bool(whole[MARGIN + nbytes:].eq(POISON).all())


@pytest.mark.parametrize("grouped", (False, True))
def test_nothing_outside_the_outputs_is_written(grouped_case, grouped):
    fa, fb, ops, biases = grouped_case
    rows, H = T, GH
    hand = [0, 1, 130, 189]
    offs = _offs_int32(torch.tensor(hand, device=DEV), T)
    if grouped:
        call = lambda **kw: _hip.mx_grouped_glu_matmul(ops[0], ops[1], fa, ops[2], ops[3], fb, offs, biases[2], "gelu", **kw)
        ref = lambda **kw: grouped_ref(ops, fa, fb, offs, biases[2], "gelu", **kw)
    else:
        call = lambda **kw: _hip.mx_glu_matmul(ops[0], ops[1], fa, ops[2][1], ops[3][1], fb, biases[1], "gelu", **kw)
        ref = lambda **kw: epilogue_ref(mx_matmul(ops[0], ops[1], fa, ops[2][1], ops[3][1], fb, biases[1]), "gelu", **kw)
    for dt in (torch.float32, torch.float16):
        n = rows * H * torch.empty(0, dtype=dt).element_size()
        whole, body = carve(n)
        y = call(out_dtype=dt, out=body.view(dt))
        check(y, ref(out_dtype=dt), ("poisoned float", grouped, dt))
        assert margins_intact(whole, n), ("float margins", grouped, dt)
        if grouped:
            assert y[hand[-1]:].eq(0).all() and not torch.signbit(y[hand[-1]:]).any()
    wc, bc = carve(rows * H)
    ws, bs = carve(rows * (H // 32))
    codes, scales = call(out_fmt="mxfp4_e2m1", out=(bc.view(rows, H), bs.view(rows, H // 32)))
    check((codes, scales), ref(out_fmt="mxfp4_e2m1"), ("poisoned codes", grouped))
    assert margins_intact(wc, rows * H) and margins_intact(ws, rows * (H // 32)), ("codes margins", grouped)
    if grouped:
        assert not codes[hand[-1]:].any() and not scales[hand[-1]:].any()
    # the rows past M of a padded allocation: the product of the first 130 rows into buffers of 200
    if not grouped:
        wc, bc = carve(rows * H)
        ws, bs = carve(rows * (H // 32))
        M = 130
        _hip.mx_glu_matmul(ops[0][:M], ops[1][:M], fa, ops[2][1], ops[3][1], fb, biases[1], "gelu", out_fmt="mxfp4_e2m1",
                           out=(bc[:M * H].view(M, H), bs[:M * (H // 32)].view(M, H // 32)))
        assert bc[M * H:].eq(POISON).all() and bs[M * (H // 32):].eq(POISON).all()
        assert torch.equal(bc[:M * H].view(M, H), codes[:M]) and torch.equal(bs[:M * (H // 32)].view(M, -1), scales[:M])


# ---- layers ------------------------------------------------------------------------------------------------------------------------
def test_layer_chain_hands_codes_on():
    g = torch.Generator().manual_seed(5)
    H, K = 64, 96
    lin = MXGLULinear.from_float(torch.randn(H, K, generator=g) / K ** 0.5, torch.randn(H, K, generator=g) / K ** 0.5,
                                 torch.randn(H, generator=g), torch.randn(H, generator=g), out_fmt="mxfp8_e4m3").to(DEV)
    x = (torch.randn(33, K, generator=g) * 2).to(DEV)
    out = lin(x)
    assert isinstance(out, MXActivation) and out.fmt == "mxfp8_e4m3"
    xc = codes_of(x, "mxfp8_e4m3")
    want = epilogue_ref(mx_matmul(xc[0], xc[1], "mxfp8_e4m3", lin.weight_codes, lin.weight_scales, "mxfp8_e4m3", lin.bias), "silu",
                        out_fmt="mxfp8_e4m3")
    check((out.codes, out.scales), want, "MXGLULinear")


def test_gated_moe_block_captures_and_replays():
    g = torch.Generator().manual_seed(6)
    Tk, D, H, experts = 64, 64, 64, 4
    rnd = lambda *s: torch.randn(*s, generator=g)
    moe = MXGatedMoEFeedForward.from_float(rnd(experts, D), rnd(experts, H, D) / 8, rnd(experts, H), rnd(experts, H, D) / 8, rnd(experts, H),
                                           rnd(experts, D, H) / 8, rnd(experts, D), 2, act="silu").to(DEV)
    xs = [rnd(Tk, D).to(DEV) for _ in range(2)]
    eager = [moe(x).clone() for x in xs]
    assert not same(eager[0], eager[1])
    # eager equals the written-out composition with the reference epilogue in place of the gated product
    x = xs[0]
    top, ids = torch.topk(x @ moe.router.t(), 2, -1)
    order = torch.argsort(ids.reshape(-1), stable=True)
    offs = (ids.reshape(-1).unsqueeze(1) == torch.arange(experts, device=DEV)).sum(0).cumsum(0).to(torch.int32)
    rows = codes_of(x[torch.div(order, 2, rounding_mode="floor")], "mxfp8_e4m3")
    hidden = grouped_ref(rows + (moe.up.weight_codes, moe.up.weight_scales), "mxfp8_e4m3", "mxfp8_e4m3", offs, moe.up.bias, "silu",
                         out_fmt="mxfp8_e4m3")
    y = moe.down(MXActivation(*hidden, "mxfp8_e4m3"), offs)[torch.argsort(order)].reshape(-1, 2, D)
    assert same(eager[0], (y * torch.softmax(top, -1).unsqueeze(-1)).sum(1))
    # one stream, no parallel branches
    static_x = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        moe(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = moe(static_x)
    for x, want in zip(reversed(xs), reversed(eager)):
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert same(static_y, want)
