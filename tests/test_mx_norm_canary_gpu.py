"""Out-of-bounds check for the MX normalising quantizer, in the manner of tests/test_mx_quant2_canary_gpu.py, through the C ABI: every
pointer of a qs_mx_norm_quant_v call -- x, weight, bias, the four code / scale outputs, rstd, mean -- is a body inside its own
pattern-filled allocation.  After the launch every margin must be intact, every input byte-identical, every output asked for equal to
the CPU path of ``mx_norm_quantize`` bit for bit (tests/test_mx_norm.py pins that to the definition) and every output not asked for
still hold the pattern.  Output allocations are filled with 0xA5, the margins of the inputs with 0xFF -- a NaN in all three dtypes, so
an over-read that enters a sum or a maximum shows as NaN statistics and 0xFF scale bytes.

The bases are where the header allows them weakest: row_codes off 4 bytes and col_codes off 16 on the VEC route (the byte-store arms
of its two phases), the scales at odd addresses, rstd and mean at 4 bytes, and each of x, weight, bias alone off 16 bytes (PLAIN).  The
shapes are the smallest at which a mechanism changes: the 128 x 64 tile, the block of 32, the statistics pass of 512, R % 16."""
import ctypes

import pytest
import torch

import mx_norm_ref as NR
from mx_guard import guarded, intact
from qsparse_amd import _hip, mx_norm_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_NORM_ROUTE_VEC, _hip.MX_NORM_ROUTE_PLAIN
OUT, NAN = 0xA5, 0xFF       # the fill of an output's allocation; of an input's margins
PAIRS = [("mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp4_e2m1", "mxfp6_e2m3"), ("mxfp6_e3m2", "mxfp4_e2m1")]      # all five formats
SHAPES = ((1, 1), (1, 32), (16, 32), (128, 64), (129, 96), (130, 72), (33, 31), (300, 1), (1, 300), (5, 520), (144, 544), (160, 96))
WEAKEST = {"row_codes": 3, "col_codes": 1, "row_scales": 1, "col_scales": 1, "rstd": 1, "mean": 1}


def _route(C):
    return VEC if C % 32 == 0 else PLAIN


def _cases():
    """(R, C, (weight, bias) present | None: rotated over the shapes, col pair asked for, {operand: offset of its base}, route) -- the
    offsets in elements for x, weight, bias, rstd and mean, in bytes for codes and scales"""
    out = [(R, C, None, True, {}, _route(C)) for R, C in SHAPES]
    out += [(R, C, None, True, {"row_codes": o}, VEC) for R, C in ((129, 96), (144, 544)) for o in (1, 2, 3)]
    out += [(R, C, None, True, {"col_codes": o}, VEC) for R, C in ((16, 32), (160, 96), (144, 544)) for o in (4, 1, 16)]
    out += [(R, C, None, True, {"row_scales": 1, "col_scales": 3, "rstd": 1, "mean": 1}, _route(C))
            for R, C in ((129, 96), (130, 72), (144, 544), (33, 31))]
    out += [(R, C, None, True, WEAKEST, _route(C)) for R, C in ((160, 96), (144, 544), (129, 65))]
    out += [(R, C, (True, True), True, {n: 1}, PLAIN) for R, C in ((129, 96), (160, 96)) for n in ("x", "weight", "bias")]
    out += [(R, C, None, False, offs, _route(C)) for R, C in ((1, 1), (129, 96), (130, 72), (160, 96)) for offs in ({}, WEAKEST)]
    return out


CASES = _cases()
_refs = {}


def _reference(norm, dtype, row_fmt, col_fmt, R, C, wb):
    """the inputs of mx_norm_ref.inputs and what the CPU path makes of them, computed once per key: (x, w, b), {output: tensor}"""
    key = (norm, dtype, row_fmt, col_fmt, R, C, wb)
    if key not in _refs:
        x, w, b = NR.inputs(1000 * R + C, R, C, dtype, *wb)
        rc, rs, cc, cs, rstd, mean = mx_norm_quantize(x, w, b, norm=norm, eps=NR.EPS, fmt=row_fmt, col_fmt=col_fmt, return_stats=True)
        # the reference alone is finite and in range: no block is NaN by the inputs' own doing
        assert bool(rstd.isfinite().all()) and not bool((rs == 0xFF).any()) and not bool((cs == 0xFF).any()), key
        _refs[key] = ((x, w, b), dict(row_codes=rc, row_scales=rs, col_codes=cc, col_scales=cs, rstd=rstd, mean=mean))
    return _refs[key]


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


class _Operand:
    """`nbytes` at pad + `offset` bytes of its own allocation; an input (`data` given) has 0xFF margins, an output is 0xA5 throughout"""

    def __init__(self, nbytes, offset, data=None):
        self.nbytes, self.offset, self.pattern = nbytes, offset, OUT if data is None else NAN
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


def _run(lib, norm, dtype, row_fmt, col_fmt, R, C, wb, col, offs, route):
    """one guarded call with every check of this file; returns (operands, the arms the pointers select)"""
    (x, w, b), ref = _reference(norm, dtype, row_fmt, col_fmt, R, C, wb)
    what = (norm, dtype, row_fmt, col_fmt, R, C, wb, col, offs)
    esz = x.element_size()
    nbr, nbc = -(-R // 32), -(-C // 32)
    ins = {n: _Operand(t.numel() * t.element_size(), offs.get(n, 0) * t.element_size(), t)
           for n, t in (("x", x), ("weight", w), ("bias", b)) if t is not None}
    sizes = dict(row_codes=R * C, row_scales=R * nbc, col_codes=C * R, col_scales=C * nbr, rstd=4 * R, mean=4 * R)
    outs = {n: _Operand(sizes[n], offs.get(n, 0) * (4 if n in ("rstd", "mean") else 1)) for n in sizes}
    asked = ["row_codes", "row_scales", "rstd"] + (["col_codes", "col_scales"] if col else []) + (["mean"] if norm == "layer" else [])

    a = _hip.MxNormQuantArgs()
    a.struct_size = ctypes.sizeof(a)
    a.mode = _hip.MX_NORMS.index(norm)
    a.row_format, a.col_format = _hip.MX_FORMATS.index(row_fmt), _hip.MX_FORMATS.index(col_fmt) if col else -1
    a.xdt, a.eps = _hip._DT[dtype], NR.EPS
    for n, op in list(ins.items()) + list(outs.items()):        # an output that is not asked for is passed all the same: it is ignored
        setattr(a, n, op.ptr)
    a.R, a.C = R, C
    a.stream = _hip._stream(ins["x"].body)

    # the documented rule, from the pointers actually passed (an absent weight or bias is a null pointer: aligned)
    p = {n: ins[n].ptr if n in ins else 0 for n in ("x", "weight", "bias")}
    assert all(p[n] % 16 == (offs.get(n, 0) * (esz if n == "x" else 4)) % 16 for n in p if n in ins), what
    want_route = VEC if C % 32 == 0 and all(v % 16 == 0 for v in p.values()) else PLAIN
    assert want_route == route, what
    arms = {"VEC" if route == VEC else "PLAIN"}
    if route == VEC:
        arms.add("VEC row_vec=%d" % (outs["row_codes"].ptr % 4 == 0))
        if col:
            arms.add("VEC col_vec=0 by R" if R % 16 else "VEC col_vec=%d by alignment" % (outs["col_codes"].ptr % 16 == 0))
    elif C % 32 == 0:
        arms.add("PLAIN by " + " ".join(n for n in p if p[n] % 16) + " alone")
    assert lib.qs_mx_norm_quant_route(ctypes.byref(a)) == want_route, what
    assert lib.qs_mx_norm_quant_v(ctypes.byref(a)) == 0, what
    torch.cuda.synchronize()

    for n, op in ins.items():
        assert op.margins() and torch.equal(op.body.cpu(), op.data), (n, what)
    for n, op in outs.items():
        assert op.margins(), (n, what)
        if n in asked:
            assert op.holds(ref[n]), (n, what)
        else:
            assert op.untouched(), (n, what)
    return outs, arms


@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
@pytest.mark.parametrize("dtype", NR.DTS, ids=str)
@pytest.mark.parametrize("norm", NR.NORMS)
def test_margins_survive_every_route(norm, dtype, row_fmt, col_fmt):
    lib = _hip.load()
    turn = NR.NORMS.index(norm) + NR.DTS.index(dtype) + PAIRS.index((row_fmt, col_fmt))
    seen, wbs = set(), set()
    for R, C, wb, col, offs, route in CASES:
        if wb is None:
            wb = NR.WB[((SHAPES.index((R, C)) if (R, C) in SHAPES else 0) + turn) % 4]
        wbs.add(wb)
        seen |= _run(lib, norm, dtype, row_fmt, col_fmt, R, C, wb, col, offs, route)[1]
    print(sorted(seen))
    assert wbs == set(NR.WB)
    assert seen >= {"VEC", "PLAIN", "VEC row_vec=1", "VEC row_vec=0", "VEC col_vec=1 by alignment", "VEC col_vec=0 by alignment",
                    "VEC col_vec=0 by R", "PLAIN by x alone", "PLAIN by weight alone", "PLAIN by bias alone"}


def test_the_guard_can_fail():
    """the same call judged with bodies one row shorter than the R the library was given: the last row's legitimate stores lie in what
    is then counted as margin (inside the allocations all the same), and `intact` must say so"""
    R, C = 129, 96
    outs, _ = _run(_hip.load(), "layer", torch.bfloat16, *PAIRS[0], R, C, (True, True), True, {}, VEC)
    nbc = -(-C // 32)
    for n, short in (("row_codes", (R - 1) * C), ("row_scales", (R - 1) * nbc), ("rstd", (R - 1) * 4), ("mean", (R - 1) * 4)):
        assert outs[n].margins() and not outs[n].margins(short), n
