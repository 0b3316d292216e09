"""Out-of-bounds check for the MX rotary kernels, in the manner of tests/test_mx_softmax_train_canary_gpu.py, through the C ABI: every
pointer of a qs_mx_rope_quant2_v and of a qs_mx_rope_v call -- x, cos, sin, the four code outputs, y -- is a body inside its own
pattern-filled allocation.  After the launches every margin must be intact, every input byte-identical and every output equal to the
CPU path bit for bit (tests/test_mx_rope.py pins that to the definition).  Output allocations are filled with 0xA5, the margins of the
inputs with 0xFF -- a NaN in all three dtypes and in the float32 tables, so an over-read of x, of a partner or of a table entry poisons
the pair computed from it and its blocks in both directions.

The bases are taken where the header allows them strongest (everything 16-byte aligned) and weakest: codes and scales at odd
addresses, x and y off one element, the tables off one float.  T = 33, d = 72 crosses the block along T and has a short third block
along d with h = 36 off the two-byte vector width; T = 129, d = 2 crosses the 128-row tile with rows of a single pair.  Neither can
take the quantizing kernel's VEC route (T % 16 != 0); T = 16, d = 64 with aligned bases is its VEC launch, the same shape with the
weakest bases the PLAIN one.  The expected route of every launch is computed from the header's conditions and asserted."""
import ctypes

import pytest
import torch

import mx_rope_ref as RR
from mx_guard import guarded, intact
from qsparse_amd import _hip, mx_rope, mx_rope_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_ROPE_ROUTE_VEC, _hip.MX_ROPE_ROUTE_PLAIN
OUT, NAN = 0xA5, 0xFF       # the fill of an output's allocation; of an input's margins
G = 3
SHAPES = ((33, 72), (129, 2), (16, 64))
WEAKEST = {"row_codes": 3, "row_scales": 1, "col_codes": 1, "col_scales": 1, "x": 1, "y": 1, "cos": 1, "sin": 1}
PAIRS = ("row_codes", "row_scales", "col_codes", "col_scales")
RF, CF = "mxfp8_e4m3", "mxfp6_e3m2"
_refs = {}


def _reference(dtype, shape, interleaved, inverse):
    key = (dtype, shape, interleaved, inverse)
    if key not in _refs:
        T, d = shape
        x = RR.inputs(100 * T + d, (G, T, d), dtype)
        cos, sin = RR.tables(T, d, T)
        kw = dict(interleaved=interleaved, inverse=inverse)
        _refs[key] = (x, cos, sin, mx_rope_quantize(x, cos, sin, row_fmt=RF, col_fmt=CF, **kw),
                      {od: mx_rope(x, cos, sin, out_dtype=od, **kw) for od in (dtype, torch.float32)})
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

    def margins(self):
        return intact(self.raw, self.nbytes, self.offset, pattern=self.pattern)


def _run(lib, dtype, shape, interleaved, inverse, offs):
    x, cos, sin, codes, dense = _reference(dtype, shape, interleaved, inverse)
    what = (dtype, shape, interleaved, inverse, sorted(offs))
    T, d = shape
    es = x.element_size()
    ins = {"x": _Operand(x.numel() * es, offs.get("x", 0) * es, x), "cos": _Operand(cos.numel() * 4, offs.get("cos", 0) * 4, cos),
           "sin": _Operand(sin.numel() * 4, offs.get("sin", 0) * 4, sin)}
    v = 4 if dtype == torch.float32 else 8
    vec_ok = not offs and d % v == 0 and (interleaved or (d // 2) % v == 0)       # (the header's conditions; the strides are T d and d)
    stream = _hip._stream(ins["x"].body)

    def common(a):
        a.struct_size = ctypes.sizeof(a)
        a.xdt, a.interleaved, a.inverse = _hip._DT[dtype], int(interleaved), int(inverse)
        a.x, a.cos, a.sin = ins["x"].ptr, ins["cos"].ptr, ins["sin"].ptr
        a.G0, a.G1, a.R, a.C = 1, G, T, d
        a.x_stride_g0, a.x_stride_g1, a.x_stride_r = 0, T * d, d
        a.stream = stream

    # ---- the quantizing call: all four outputs ----
    outs = {n: _Operand(codes[i].numel(), offs.get(n, 0)) for i, n in enumerate(PAIRS)}
    a = _hip.MxRopeQuant2Args()
    common(a)
    a.row_format, a.col_format = _hip.MX_FORMATS.index(RF), _hip.MX_FORMATS.index(CF)
    a.row_codes, a.row_scales, a.col_codes, a.col_scales = (outs[n].ptr for n in PAIRS)
    assert lib.qs_mx_rope_quant2_route(ctypes.byref(a)) == (VEC if vec_ok and T % 16 == 0 else PLAIN), what
    assert lib.qs_mx_rope_quant2_v(ctypes.byref(a)) == 0, what
    torch.cuda.synchronize()
    for n, ref in zip(PAIRS, codes):
        assert outs[n].margins(), (n, what)
        assert torch.equal(outs[n].body.cpu(), _bytes(ref)), (n, what)

    # ---- the dense call, to x's dtype and to float32 ----
    for od, ref in dense.items():
        y = _Operand(ref.numel() * ref.element_size(), offs.get("y", 0) * ref.element_size())
        b = _hip.MxRopeArgs()
        common(b)
        b.y, b.ydt = y.ptr, _hip._DT[od]
        assert lib.qs_mx_rope_route(ctypes.byref(b)) == (VEC if vec_ok else PLAIN), (od, what)
        assert lib.qs_mx_rope_v(ctypes.byref(b)) == 0, (od, what)
        torch.cuda.synchronize()
        assert y.margins(), (od, what)
        assert RR.same_bits(y.body.cpu().view(od).view(ref.shape), ref), (od, what)
    for n, op in ins.items():
        assert op.margins() and torch.equal(op.body.cpu(), op.data), (n, what)


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("dtype", RR.DTS, ids=str)
def test_margins_survive(dtype, interleaved):
    lib = _hip.load()
    for shape in SHAPES:
        for inverse in (False, True):
            for offs in ({}, WEAKEST):
                _run(lib, dtype, shape, interleaved, inverse, offs)
