"""Out-of-bounds check for the two calls that take the residual stream, in the manner of tests/test_mx_norm_canary_gpu.py and
tests/test_mx_norm_bwd_canary_gpu.py, through the C ABI: every pointer of a qs_mx_add_norm_quant_v call -- x, residual, weight, bias, h,
the four code / scale outputs, rstd, mean -- and of a qs_mx_norm_bwd_res_v call -- dxhat, x, dresidual, weight, rstd, mean, dx, dweight,
dbias and the workspace -- is a body inside its own pattern-filled allocation.  After the launch every margin must be intact, every input
byte-identical, every output asked for equal to the CPU path bit for bit (tests/test_mx_add_norm.py pins that to the composition and to
the definition) and every output not asked for still hold the pattern.  Output allocations are filled with 0xA5, the margins of the
inputs with 0xFF -- a NaN in all three dtypes, so an over-read that enters a sum shows as NaN statistics.

The bases are where the header allows them weakest on each route, and each of x, residual, h, dresidual alone off 16 bytes (PLAIN).  The
shapes are the smallest at which a mechanism changes: the 128 x 64 tile, the block of 32, the statistics pass of 512, ragged last tiles."""
import ctypes

import pytest
import torch

import mx_norm_bwd_ref as BR
import test_mx_add_norm as A
from mx_guard import guarded, intact
from mx_norm_ref import DTS, EPS, NORMS, WB
from qsparse_amd import _hip, mx_add_norm_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_NORM_ROUTE_VEC, _hip.MX_NORM_ROUTE_PLAIN
OUT, NAN = 0xA5, 0xFF       # the fill of an output's allocation; of an input's margins
FMT_PAIRS = [("mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp4_e2m1", "mxfp6_e2m3"), ("mxfp6_e3m2", "mxfp4_e2m1")]      # all five formats
SHAPES = ((1, 1), (1, 32), (16, 32), (128, 64), (129, 96), (130, 72), (33, 31), (5, 520), (144, 544))
# the weakest bases: the VEC route leaves the outputs' free (byte stores of codes and scales, rstd / mean at 4 bytes); PLAIN takes
# every tensor at its element's alignment, weight and bias at 4 bytes
WEAK_VEC = {"row_codes": 3, "col_codes": 1, "row_scales": 1, "col_scales": 1, "rstd": 1, "mean": 1}
WEAK_PLAIN = dict(WEAK_VEC, x=1, residual=1, h=1, weight=1, bias=1)


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


class _Operand:
    """`nbytes` at pad + `offset` bytes of its own allocation; an input (`data` given) has 0xFF margins, an output is 0xA5 throughout"""

    def __init__(self, nbytes, offset, data=None, pattern=None):
        self.nbytes, self.offset = nbytes, offset
        self.pattern = pattern if pattern is not None else (OUT if data is None else NAN)
        self.raw, self.body = guarded(nbytes, offset, pattern=self.pattern)
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


# ---- qs_mx_add_norm_quant_v ----------------------------------------------------------------------------------------------------------------
_refs = {}


def _reference(norm, xdt, rdt, row_fmt, col_fmt, R, C, wb):
    """the inputs of test_mx_add_norm.add_inputs and what the CPU path makes of them, computed once per key"""
    key = (norm, xdt, rdt, row_fmt, col_fmt, R, C, wb)
    if key not in _refs:
        x, res, w, b = A.add_inputs(1000 * R + C, R, C, xdt, rdt, *wb)
        h, rc, rs, cc, cs, rstd, mean = mx_add_norm_quantize(x, res, w, b, norm=norm, eps=EPS, fmt=row_fmt, col_fmt=col_fmt, return_stats=True)
        # the reference alone is finite and in range: no block is NaN by the inputs' own doing
        assert bool(h.isfinite().all()) and bool(rstd.isfinite().all()) and not bool((rs == 0xFF).any()) and not bool((cs == 0xFF).any()), key
        _refs[key] = ((x, res, w, b), dict(h=h, row_codes=rc, row_scales=rs, col_codes=cc, col_scales=cs, rstd=rstd, mean=mean))
    return _refs[key]


def _run_add(lib, norm, xdt, rdt, row_fmt, col_fmt, R, C, wb, col, offs):
    """one guarded call; `offs` in elements for x, residual, h, weight, bias, rstd and mean, in bytes for codes and scales.  Returns
    (operands, route)"""
    (x, res, w, b), ref = _reference(norm, xdt, rdt, row_fmt, col_fmt, R, C, wb)
    what = (norm, xdt, rdt, row_fmt, col_fmt, R, C, wb, col, offs)
    nbr, nbc = -(-R // 32), -(-C // 32)
    ins = {n: _Operand(t.numel() * t.element_size(), offs.get(n, 0) * t.element_size(), t)
           for n, t in (("x", x), ("residual", res), ("weight", w), ("bias", b)) if t is not None}
    rsz = res.element_size()
    sizes = dict(h=R * C * rsz, row_codes=R * C, row_scales=R * nbc, col_codes=C * R, col_scales=C * nbr, rstd=4 * R, mean=4 * R)
    unit = dict(h=rsz, rstd=4, mean=4)
    outs = {n: _Operand(sizes[n], offs.get(n, 0) * unit.get(n, 1)) for n in sizes}
    asked = ["h", "row_codes", "row_scales", "rstd"] + (["col_codes", "col_scales"] if col else []) + (["mean"] if norm == "layer" else [])

    a = _hip.MxAddNormQuantArgs()
    a.struct_size = ctypes.sizeof(a)
    a.mode = _hip.MX_NORMS.index(norm)
    a.row_format, a.col_format = _hip.MX_FORMATS.index(row_fmt), _hip.MX_FORMATS.index(col_fmt) if col else -1
    a.xdt, a.rdt, a.eps = _hip._DT[xdt], _hip._DT[rdt], EPS
    for n, op in list(ins.items()) + list(outs.items()):        # an output that is not asked for is passed all the same: it is ignored
        setattr(a, n, op.ptr)
    a.R, a.C = R, C
    a.stream = _hip._stream(ins["x"].body)

    # the documented rule, from the pointers actually passed (an absent weight or bias is a null pointer: aligned)
    p = {n: ins[n].ptr if n in ins else 0 for n in ("x", "residual", "weight", "bias")}
    p["h"] = outs["h"].ptr
    route = VEC if C % 32 == 0 and all(v % 16 == 0 for v in p.values()) else PLAIN
    assert lib.qs_mx_add_norm_quant_route(ctypes.byref(a)) == route, what
    assert lib.qs_mx_add_norm_quant_v(ctypes.byref(a)) == 0, what
    torch.cuda.synchronize()

    for n, op in ins.items():
        assert op.margins() and torch.equal(op.body.cpu(), op.data), (n, what)
    for n, op in outs.items():
        assert op.margins(), (n, what)
        if n in asked:
            assert op.holds(ref[n]), (n, what)
        else:
            assert op.untouched(), (n, what)
    return outs, route


@pytest.mark.parametrize("xdt,rdt", A.PAIRS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_add_norm_margins_survive_every_route(norm, xdt, rdt):
    lib = _hip.load()
    turn = NORMS.index(norm) + A.PAIRS.index((xdt, rdt))
    fmts = FMT_PAIRS[turn % 3]
    seen = set()
    for i, (R, C) in enumerate(SHAPES):
        wb = WB[(i + turn) % 4]
        vec = C % 32 == 0
        assert _run_add(lib, norm, xdt, rdt, *fmts, R, C, wb, True, {})[1] == (VEC if vec else PLAIN), (R, C)
        # the weakest bases of the shape's own route; without the col pair, whose outputs must keep the pattern
        assert _run_add(lib, norm, xdt, rdt, *fmts, R, C, wb, True, WEAK_VEC if vec else WEAK_PLAIN)[1] == (VEC if vec else PLAIN), (R, C)
        assert _run_add(lib, norm, xdt, rdt, *fmts, R, C, wb, False, WEAK_PLAIN)[1] == PLAIN, (R, C)
        seen.add(vec)
    for R, C in ((16, 32), (129, 96), (144, 544)):                 # VEC shapes: each tensor alone off 16 bytes
        for n in ("x", "residual", "h", "weight", "bias"):
            assert _run_add(lib, norm, xdt, rdt, *fmts, R, C, (True, True), True, {n: 1})[1] == PLAIN, (R, C, n)
    assert seen == {True, False}


def test_the_add_norm_guard_can_fail():
    """the same call judged with bodies one row shorter than the R the library was given: `intact` must say so"""
    R, C = 129, 96
    outs, _ = _run_add(_hip.load(), "layer", torch.float32, torch.bfloat16, *FMT_PAIRS[0], R, C, (True, True), True, {})
    for n, short in (("h", (R - 1) * C * 2), ("row_codes", (R - 1) * C), ("rstd", (R - 1) * 4)):
        assert outs[n].margins() and not outs[n].margins(short), n


# ---- qs_mx_norm_bwd_res_v --------------------------------------------------------------------------------------------------------------------
BVEC, BPLAIN = _hip.MX_NORM_BWD_ROUTE_VEC, _hip.MX_NORM_BWD_ROUTE_PLAIN
NAMES = ("dx", "dweight", "dbias")
SUBSETS = ((True, True, True), (True, False, False), (True, True, False), (True, False, True))
BWEAK_VEC = {"rstd": 1, "mean": 1, "dweight": 1, "dbias": 1}
BWEAK_PLAIN = dict(BWEAK_VEC, dxhat=1, x=1, dresidual=1, weight=1, dx=1)
_brefs = {}


def _plan(R, C, layer, need_cols):
    """the header's formula with dx asked for: up16(4 R), twice in layer mode, plus 2 up16(4 ceil(R / 128) C) with dweight or dbias"""
    def up16(n):
        return (n + 15) // 16 * 16
    return up16(4 * R) * (2 if layer else 1) + (2 * up16(4 * -(-R // 128) * C) if need_cols else 0)


def _breference(R, C, dtype, norm, has_w, gdtype):
    key = (R, C, dtype, norm, has_w, gdtype)
    if key not in _brefs:
        case, dres = BR.case(*key), A.dres_of(R, C, dtype)
        res = A.run_bwd("cpu", case, norm, dres)
        assert all(bool(t.isfinite().all()) for t in tuple(res) + (case[2],)), key      # the reference alone is finite
        _brefs[key] = (case, dres, dict(zip(NAMES, res)))
    return _brefs[key]


def _run_bwd(lib, norm, dtype, gdtype, R, C, has_w, needs, offs, fill=OUT):
    """one guarded call on a workspace of exactly the plan's bytes that holds `fill`; `offs` in elements.  Returns (operands, route)"""
    (dxhat, x, rstd, mean, w), dres, ref = _breference(R, C, dtype, norm, has_w, gdtype)
    what = (norm, dtype, gdtype, R, C, has_w, needs, offs, hex(fill))
    layer = norm == "layer"
    if not layer:
        mean = torch.full((R,), -1, dtype=torch.int32).view(torch.float32)      # 0xFF bytes, a NaN: mean is ignored in rms mode
    ins = {n: _Operand(t.numel() * t.element_size(), offs.get(n, 0) * t.element_size(), t)
           for n, t in (("dxhat", dxhat), ("x", x), ("dresidual", dres), ("weight", w), ("rstd", rstd), ("mean", mean)) if t is not None}
    esz = x.element_size()
    sizes = dict(dx=R * C * esz, dweight=4 * C, dbias=4 * C)
    outs = {n: _Operand(sizes[n], offs.get(n, 0) * (esz if n == "dx" else 4)) for n in NAMES}
    asked = [n for n, need in zip(NAMES, needs) if need]
    plan = _plan(R, C, layer, needs[1] or needs[2])
    assert _hip.mx_norm_bwd_plan(R, C, norm, True, needs[1] or needs[2]) == plan, what
    ws = _Operand(plan, 0, pattern=fill)

    a = _hip.MxNormBwdResArgs()
    a.struct_size = ctypes.sizeof(a)
    a.mode, a.xdt, a.gdt = _hip.MX_NORMS.index(norm), _hip._DT[dtype], _hip._DT[gdtype]
    for n, op in ins.items():
        setattr(a, n, op.ptr)
    for n in asked:
        setattr(a, n, outs[n].ptr)
    a.workspace, a.workspace_bytes = ws.ptr, plan
    a.R, a.C = R, C
    a.stream = _hip._stream(ins["x"].body)

    p = {"dxhat": ins["dxhat"].ptr, "x": ins["x"].ptr, "dresidual": ins["dresidual"].ptr, "weight": ins["weight"].ptr if has_w else 0,
         "dx": outs["dx"].ptr}
    route = BVEC if C % 32 == 0 and all(v % 16 == 0 for v in p.values()) else BPLAIN
    assert lib.qs_mx_norm_bwd_res_route(ctypes.byref(a)) == route, what
    assert lib.qs_mx_norm_bwd_res_v(ctypes.byref(a)) == 0, what
    torch.cuda.synchronize()

    for n, op in ins.items():
        assert op.margins() and torch.equal(op.body.cpu(), op.data), (n, what)
    assert ws.margins(), ("workspace", what)
    for n, op in outs.items():
        assert op.margins(), (n, what)
        if n in asked:
            assert op.holds(ref[n]), (n, what)
        else:
            assert op.untouched(), (n, what)
    return dict(outs, workspace=ws), route


@pytest.mark.parametrize("dtype", DTS, ids=str)
@pytest.mark.parametrize("norm", NORMS)
def test_backward_margins_survive_every_route(norm, dtype):
    """every shape with the subset of the outputs and dxhat's dtype rotating, on the weakest bases of its route and on a workspace
    that holds NaN; then each of x, dresidual, dxhat, dx alone off 16 bytes"""
    lib = _hip.load()
    turn = NORMS.index(norm) + DTS.index(dtype)
    for i, (R, C) in enumerate(SHAPES):
        vec = C % 32 == 0
        gdt, needs, has_w = DTS[(i + turn) % 3], SUBSETS[(i + turn) % 4], bool((i + turn) & 1)
        assert _run_bwd(lib, norm, dtype, gdt, R, C, has_w, SUBSETS[0], {})[1] == (BVEC if vec else BPLAIN), (R, C)
        assert _run_bwd(lib, norm, dtype, gdt, R, C, has_w, needs, BWEAK_VEC if vec else BWEAK_PLAIN, NAN)[1] == (BVEC if vec else BPLAIN)
        assert _run_bwd(lib, norm, dtype, gdt, R, C, has_w, needs, BWEAK_PLAIN)[1] == BPLAIN, (R, C)
    for R, C in ((16, 32), (129, 96), (144, 544)):
        for n in ("x", "dresidual", "dxhat", "dx"):
            assert _run_bwd(lib, norm, dtype, DTS[turn % 3], R, C, True, SUBSETS[0], {n: 1}, NAN)[1] == BPLAIN, (R, C, n)


def test_the_backward_guard_can_fail():
    R, C = 129, 96
    ops, _ = _run_bwd(_hip.load(), "layer", torch.bfloat16, torch.float32, R, C, True, SUBSETS[0], {})
    assert ops["dx"].margins() and not ops["dx"].margins((R - 1) * C * 2)
