"""Out-of-bounds and missed-store check for the grouped MX products, in the manner of tests/test_mx_bmm_canary_gpu.py: ``y``,
``out_codes`` and ``out_scales`` are carved out of larger allocations that hold a byte pattern (tests/mx_guard.py) in the margins AND
in the body.  After the launch not a byte outside the body may have changed, and the body equals ``mx_matmul`` group by group and
+0 (code 0, scale byte 0) in the tail: a tile that no work-group stored still holds the pattern, which a fresh ``torch.empty`` --
often the block a correct call has just freed -- would not show.  Groups that are empty, of one row, one under, at and one over the
128-row tile and over two tiles, N % 4 != 0 and N % 32 != 0: single-element stores and a short last scale block next to every group
boundary, where a row bound that is off by one writes into the next group.  ``tail``: the body ends at the allocation's last byte,
with the margin in front only.  The TIGHT cases leave 1 row modulo 128 in every group and in the tail, so the real number of M-tiles
equals the grid's bound ``floor((T + 127 (E + 1)) / 128)``: a bound that is one too small drops the last tile."""
import pytest
import torch

import mx_gemm_ref as G
from mx_guard import PAD, PATTERN, guarded, intact
from qsparse_amd import _hip, mx_matmul, quantize_with_mx
from test_mx_grouped import TIGHT, ends_of, m_tiles, mt_max

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES, TAIL = (0, 1, 127, 0, 0, 129, 128, 257, 0), 5
SHAPES = [(33, 100), (131, 64), (67, 100)]                    # N, K
ROUTE = {100: _hip.MX_GEMM_ROUTE_PLAIN, 64: _hip.MX_GEMM_ROUTE_VEC}
# sizes, tail: every range 1 modulo 128; the same without a tail; no group at all, the tail over two tiles
TIGHT_CASES = [TIGHT, (TIGHT[0], 0), ((), 129)]


def carve(nbytes, tail):
    """(raw, body, check): `body` of nbytes inside a pattern-filled allocation -- margins on both sides, or (tail) in front only"""
    if not tail:
        raw, body = guarded(nbytes)
        return raw, body, lambda: intact(raw, nbytes)
    raw = torch.full((PAD + nbytes,), PATTERN, dtype=torch.uint8, device=DEV)
    return raw, raw[PAD:], lambda: bool((raw[:PAD] == PATTERN).all())


def operands(g, sizes, tail, N, K, fa, fb):
    """(the six operand arguments, offs int32, bias [E, N], ends): every expert's weight under its own power of two"""
    E, T = len(sizes), sum(sizes) + tail
    x = torch.randn(T, K, generator=g) * 2
    w = torch.randn(E, N, K, generator=g) / K ** 0.5 * torch.pow(2.0, torch.arange(E) % 5.0).view(-1, 1, 1)
    ends = ends_of(sizes).tolist() if E else []
    ops = (tuple(quantize_with_mx(x.to(DEV), fa, -1, return_codes=True)[1:]) + (fa,) +
           ((tuple(quantize_with_mx(w.to(DEV), fb, -1, return_codes=True)[1:])) if E else
            (torch.zeros(0, N, K, dtype=torch.uint8, device=DEV), torch.zeros(0, N, -(-K // 32), dtype=torch.uint8, device=DEV))) + (fb,))
    return ops, torch.tensor(ends, dtype=torch.int32, device=DEV), torch.randn(E, N, generator=g).to(DEV), ends


def expected(ops, ends, bias, dt=torch.float32, **kw):
    """mx_matmul group by group over zeros: [T, N] in `dt`, or with out_fmt (codes [T, N], scales [T, ceil(N / 32)])"""
    ac, asc, fa, bc, bsc, fb = ops
    T, N = ac.shape[0], bc.shape[1]
    q = kw.get("out_fmt") is not None
    want = (torch.zeros(T, N, dtype=torch.uint8, device=DEV), torch.zeros(T, -(-N // 32), dtype=torch.uint8, device=DEV)) if q else \
        (torch.zeros(T, N, dtype=dt, device=DEV),)
    for e, (lo, hi) in enumerate(zip([0] + ends, ends)):
        if hi > lo:
            got = mx_matmul(ac[lo:hi], asc[lo:hi], fa, bc[e], bsc[e], fb, bias[e], dt, **kw)
            for full, piece in zip(want, got if q else (got,)):
                full[lo:hi] = piece
    return want if q else want[0]


def check_y(g, sizes, tail_rows, N, K, fa, fb, dt, tail):
    ops, offs, bias, ends = operands(g, sizes, tail_rows, N, K, fa, fb)
    T = sum(sizes) + tail_rows
    what = (sizes, tail_rows, N, K, fa, fb, dt, tail)
    raw, body, ok = carve(T * N * torch.empty(0, dtype=dt).element_size(), tail)
    y = _hip.mx_grouped_matmul(*ops, offs, bias, dt, out=body.view(dt))
    torch.cuda.synchronize()
    assert y.data_ptr() == body.data_ptr() and y.shape == (T, N) and _hip.mx_grouped_last_route == ROUTE[K], what
    assert ok(), ("y margins", what)
    assert G.same(y, expected(ops, ends, bias, dt)), what                    # (the tail: +0; an unwritten tile: the pattern)


def check_codes(g, sizes, tail_rows, N, K, fa, fb, out_fmt, act, tail):
    ops, offs, bias, ends = operands(g, sizes, tail_rows, N, K, fa, fb)
    T, nb = sum(sizes) + tail_rows, -(-N // 32)
    what = (sizes, tail_rows, N, K, out_fmt, act, tail)
    craw, cbody, cok = carve(T * N, tail)
    sraw, sbody, sok = carve(T * nb, tail)
    codes, scales = _hip.mx_grouped_matmul_q(*ops, offs, bias, out_fmt, act, out=(cbody, sbody))
    torch.cuda.synchronize()
    assert codes.data_ptr() == cbody.data_ptr() and scales.data_ptr() == sbody.data_ptr() and _hip.mx_grouped_q_last_route == ROUTE[K], what
    assert cok(), ("out_codes margins", what)
    assert sok(), ("out_scales margins", what)
    want = expected(ops, ends, bias, out_fmt=out_fmt, act=act)
    assert torch.equal(cbody.view(T, N), want[0]) and torch.equal(sbody.view(T, nb), want[1]), what


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("fa,fb", [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4_e2m1")])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_y_margins_survive_and_every_row_is_stored(fa, fb, dt, tail):
    for N, K in SHAPES:
        assert N % 4 and N % 32
        check_y(torch.Generator().manual_seed(N + K), SIZES, TAIL, N, K, fa, fb, dt, tail)


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("act", [None, "relu"])
def test_codes_and_scales_margins_survive_and_every_row_is_stored(act, tail):
    for N, K in SHAPES:
        check_codes(torch.Generator().manual_seed(N + K + 1), SIZES, TAIL, N, K, "mxfp8_e4m3", "mxfp6_e2m3", "mxfp4_e2m1", act, tail)


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("sizes,tail_rows", TIGHT_CASES)
def test_the_last_tile_of_a_tight_grid_is_stored(sizes, tail_rows, tail):
    T, N = sum(sizes) + tail_rows, 129
    assert m_tiles(ends_of(sizes).tolist() if sizes else [], T) == mt_max(T, len(sizes))        # tight: the bound has no spare tile
    for K in (64, 100):
        g = torch.Generator().manual_seed(T + K)
        for dt in (torch.float32, torch.bfloat16):
            check_y(g, sizes, tail_rows, N, K, "mxfp8_e4m3", "mxfp4_e2m1", dt, tail)
        check_codes(g, sizes, tail_rows, N, K, "mxfp8_e4m3", "mxfp4_e2m1", "mxfp8_e4m3", "relu", tail)
