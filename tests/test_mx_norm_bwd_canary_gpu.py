"""Out-of-bounds check for the MX norm backward, in the manner of tests/test_mx_quant2_canary_gpu.py, through the C ABI: every pointer
of a qs_mx_norm_bwd_v call -- dxhat, x, weight, rstd, mean, dx, dweight, dbias and the workspace -- is a body inside its own
pattern-filled allocation.  After the launch every margin must be intact, every input byte-identical, every output asked for equal to
the CPU path of ``mx_norm_backward`` bit for bit (tests/test_mx_norm_bwd.py pins that to the definition) and every output not asked
for still hold the pattern.  Output allocations are filled with 0xA5, the margins of the inputs with 0xFF, a NaN in all three dtypes.

The workspace is a body of EXACTLY the bytes qs_mx_norm_bwd_plan tells (restated here from the header's formula), so a store or a
load behind c1, c2 or the partials [ceil(R / 128), C] lands in a margin; every case runs twice, on a workspace that holds 0xA5 and on
one that holds 0xFF (NaN), so a part that is read before it is written, or a stale part that the fold takes in, changes the result.
The bases are where the header allows them weakest; the shapes are the smallest at which a mechanism changes: the 128 x 64 tile, ragged
last tiles in both directions, the statistics pass of 512, and more than 128 row tiles in the fold on the VEC route."""
import ctypes

import pytest
import torch

import mx_norm_bwd_ref as BR
from mx_guard import guarded, intact
from mx_norm_ref import DTS, NORMS, same
from qsparse_amd import _hip, mx_norm_backward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_NORM_BWD_ROUTE_VEC, _hip.MX_NORM_BWD_ROUTE_PLAIN
OUT, NAN = 0xA5, 0xFF       # the fill of an output's allocation; of an input's margins
ERR_ALIGN, ERR_WORKSPACE = -3, -4
SHAPES = ((1, 1), (16, 32), (128, 64), (129, 96), (130, 100), (257, 64), (5, 520), (67, 1056), (16400, 32))
RAGGED = ((129, 96), (130, 100))        # a VEC and a PLAIN shape, both with a one- or two-row last tile and a half-filled column tile
NAMES = ("dx", "dweight", "dbias")
ALL = (True, True, True)
SUBSETS = [tuple(bool(bits & (1 << i)) for i in range(3)) for bits in range(1, 8)]


def _plan(R, C, layer, need_dx, need_cols):
    """the header's formula: up16(4 R), twice in layer mode, with dx; plus 2 up16(4 ceil(R / 128) C) with dweight or dbias"""
    def up16(n):
        return (n + 15) // 16 * 16
    return (up16(4 * R) * (2 if layer else 1) if need_dx else 0) + (2 * up16(4 * -(-R // 128) * C) if need_cols else 0)


_refs = {}


def _reference(R, C, dtype, norm, has_w, gdtype):
    """a case of mx_norm_bwd_ref (statistics from the CPU forward) and the CPU path's three results, computed once per key"""
    key = (R, C, dtype, norm, has_w, gdtype)
    if key not in _refs:
        dxhat, x, rstd, mean, w = case = BR.case(*key)
        res = mx_norm_backward(dxhat, x, rstd, mean, w, norm=norm)
        assert all(bool(t.isfinite().all()) for t in res + (rstd,)), key     # the reference alone is finite
        _refs[key] = (case, dict(zip(NAMES, res)))
    return _refs[key]


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


class _Operand:
    """`nbytes` at pad + `offset` bytes of its own allocation filled with `pattern`; `data` (an input) is copied into the body"""

    def __init__(self, nbytes, offset, pattern, data=None):
        self.nbytes, self.offset, self.pattern = nbytes, offset, pattern
        self.raw, self.body = guarded(nbytes, offset, pattern=pattern)
        self.data = None if data is None else _bytes(data)
        if data is not None:
            self.body.copy_(self.data.to(DEV))
        self.ptr = self.body.data_ptr()

    def margins(self, nbytes=None):
        return intact(self.raw, self.nbytes if nbytes is None else nbytes, self.offset, pattern=self.pattern)

    def holds(self, t):
        return torch.equal(self.body.cpu(), _bytes(t))

    def untouched(self):
        return bool((self.body == self.pattern).all())


def _run(lib, norm, dtype, gdtype, R, C, has_w, needs=ALL, offs={}, fill=OUT, ws_off=0, ws_short=0, refused=0):
    """one guarded call with every check of this file; `offs` in elements, `ws_off` in bytes, `fill` what the workspace holds on entry,
    `ws_short` the bytes workspace_bytes says less than the plan, `refused` the QS_ERR_* expected.  Returns (operands, route)"""
    (dxhat, x, rstd, mean, w), ref = _reference(R, C, dtype, norm, has_w, gdtype)
    what = (norm, dtype, gdtype, R, C, has_w, needs, offs, hex(fill), ws_off, ws_short)
    layer = norm == "layer"
    if not layer:
        mean = torch.full((R,), -1, dtype=torch.int32).view(torch.float32)      # 0xFF bytes, a NaN: mean is ignored in rms mode
    ins = {n: _Operand(t.numel() * t.element_size(), offs.get(n, 0) * t.element_size(), NAN, t)
           for n, t in (("dxhat", dxhat), ("x", x), ("weight", w), ("rstd", rstd), ("mean", mean)) if t is not None}
    esz = x.element_size()
    sizes = dict(dx=R * C * esz, dweight=4 * C, dbias=4 * C)
    outs = {n: _Operand(sizes[n], offs.get(n, 0) * (esz if n == "dx" else 4), OUT) for n in NAMES}
    asked = [n for n, need in zip(NAMES, needs) if need]

    # the plan, restated; the workspace is exactly that long and its allocation holds `fill` throughout
    plan = _plan(R, C, layer, needs[0], needs[1] or needs[2])
    assert plan > 0 and _hip.mx_norm_bwd_plan(R, C, norm, needs[0], needs[1] or needs[2]) == plan, what
    ws = _Operand(plan, ws_off, fill)
    assert ws.ptr % 16 == ws_off % 16, what

    a = _hip.MxNormBwdArgs()
    a.struct_size = ctypes.sizeof(a)
    a.mode, a.xdt, a.gdt = _hip.MX_NORMS.index(norm), _hip._DT[dtype], _hip._DT[gdtype]
    for n, op in ins.items():
        setattr(a, n, op.ptr)
    for n in asked:
        setattr(a, n, outs[n].ptr)
    a.workspace, a.workspace_bytes = ws.ptr, plan - ws_short
    a.R, a.C = R, C
    a.stream = _hip._stream(ins["x"].body)

    # the documented rule, from the pointers actually passed (an absent weight or dx is a null pointer: aligned)
    p = {"dxhat": ins["dxhat"].ptr, "x": ins["x"].ptr, "weight": ins["weight"].ptr if has_w else 0, "dx": outs["dx"].ptr if needs[0] else 0}
    route = VEC if C % 32 == 0 and all(v % 16 == 0 for v in p.values()) else PLAIN
    if refused:
        assert lib.qs_mx_norm_bwd_route(ctypes.byref(a)) == refused and lib.qs_mx_norm_bwd_v(ctypes.byref(a)) == refused, what
    else:
        assert lib.qs_mx_norm_bwd_route(ctypes.byref(a)) == route, what
        assert lib.qs_mx_norm_bwd_v(ctypes.byref(a)) == 0, what
    torch.cuda.synchronize()

    for n, op in ins.items():
        assert op.margins() and torch.equal(op.body.cpu(), op.data), (n, what)
    assert ws.margins(), ("workspace", what)
    if refused:
        assert ws.untouched(), ("workspace", what)
    for n, op in outs.items():
        assert op.margins(), (n, what)
        if n in asked and not refused:
            assert op.holds(ref[n]), (n, what)
        else:
            assert op.untouched(), (n, what)
    return dict(outs, workspace=ws), route


def _both_fills(lib, *args, **kw):
    """the case on a workspace that holds 0xA5 and on one that holds NaN: nothing is read before it is written"""
    routes = {_run(lib, *args, fill=fill, **kw)[1] for fill in (OUT, NAN)}
    assert len(routes) == 1
    return routes.pop()


@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_every_shape_on_an_exact_workspace(norm, dtype):
    """all three outputs, with and without weight; VEC exactly where C % 32 == 0 -- at (16400, 32) with T = 129 row tiles, so the fold's
    strided accumulation over more than 128 partials runs on the VEC route"""
    lib = _hip.load()
    for R, C in SHAPES:
        for has_w in (True, False):
            assert _both_fills(lib, norm, dtype, torch.float32, R, C, has_w) == (VEC if C % 32 == 0 else PLAIN), (R, C)
    assert -(-SHAPES[-1][0] // 128) > 128 and SHAPES[-1][1] % 32 == 0


@pytest.mark.parametrize("gdtype", DTS, ids=str)
@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_every_pair_of_dtypes(norm, dtype, gdtype):
    """the nine (xdt, gdt) instantiations, gdt = float16 among them, on both routes"""
    lib = _hip.load()
    for (R, C), route in zip(RAGGED, (VEC, PLAIN)):
        assert _both_fills(lib, norm, dtype, gdtype, R, C, True) == route
        assert _both_fills(lib, norm, dtype, gdtype, R, C, False, offs={"dweight": 1, "dbias": 1, "rstd": 1, "mean": 1}) == route


@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_every_subset_of_the_outputs(norm, dtype):
    """each with the exact workspace of its own plan, also 16 bytes into its allocation; what is not asked for keeps the pattern"""
    lib = _hip.load()
    for (R, C), route in zip(RAGGED, (VEC, PLAIN)):
        for needs in SUBSETS:
            assert _both_fills(lib, norm, dtype, torch.float32, R, C, True, needs=needs) == route
            assert _both_fills(lib, norm, dtype, torch.float32, R, C, True, needs=needs, ws_off=16) == route


@pytest.mark.parametrize("norm", NORMS)
def test_a_short_or_misaligned_workspace_is_refused_and_nothing_written(norm):
    lib = _hip.load()
    for R, C in RAGGED:
        for needs in (ALL, (True, False, False), (False, False, True)):
            _run(lib, norm, torch.bfloat16, torch.float32, R, C, True, needs=needs, ws_short=1, refused=ERR_WORKSPACE)
            _run(lib, norm, torch.bfloat16, torch.float32, R, C, True, needs=needs, ws_off=8, refused=ERR_ALIGN)


@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_one_misaligned_operand_takes_the_plain_route(norm, dtype):
    """dx alone, dxhat alone, x alone, weight alone one element off: PLAIN, and the bytes of the aligned VEC run (both are the CPU's)"""
    lib = _hip.load()
    for R, C in ((129, 96), (257, 64)):
        for gdtype in (torch.float32, torch.float16):
            assert _both_fills(lib, norm, dtype, gdtype, R, C, True) == VEC
            for n in ("dx", "dxhat", "x", "weight"):
                assert _both_fills(lib, norm, dtype, gdtype, R, C, True, offs={n: 1}) == PLAIN, n


@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_column_sums_and_statistics_at_four_byte_alignment(norm, dtype):
    lib = _hip.load()
    for R, C in RAGGED + ((67, 1056), (257, 64)):
        assert _both_fills(lib, norm, dtype, torch.float32, R, C, True, offs={"dweight": 1, "dbias": 1, "rstd": 1, "mean": 1}) == \
            (VEC if C % 32 == 0 else PLAIN)


def test_the_guard_can_fail():
    """the same call judged with bodies one row shorter than the R the library was given: the last row's legitimate stores lie in what
    is then counted as margin (inside the allocations all the same), and `intact` must say so"""
    R, C = 129, 96
    ops, _ = _run(_hip.load(), "layer", torch.bfloat16, torch.float32, R, C, True)
    assert ops["dx"].margins() and not ops["dx"].margins((R - 1) * C * 2)
    assert ops["workspace"].margins() and not ops["workspace"].margins(_plan(R, C, True, True, True) - 16)


@pytest.mark.parametrize("norm", NORMS)
def test_float16_dxhat(norm):
    """the sibling of test_mx_norm_bwd_gpu.py's test_bfloat16_dxhat, through the public function"""
    for R, C, dtype in ((300, 520, torch.bfloat16), (129, 96, torch.float32)):
        case = BR.case(R, C, dtype, norm, True, torch.float16)
        assert case[0].dtype == torch.float16
        dxhat, x, rstd, mean, w = [t if t is None else t.to(DEV) for t in case]
        got = mx_norm_backward(dxhat, x, rstd, mean, w, norm=norm)
        assert all(same(a.cpu(), r) for a, r in zip(got, mx_norm_backward(*case, norm=norm)))
