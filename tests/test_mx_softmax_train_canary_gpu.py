"""Out-of-bounds check for the training side of the MX softmax quantizer, in the manner of tests/test_mx_softmax_canary_gpu.py, through
the C ABI: every pointer of a qs_mx_softmax_quant2_v and of a qs_mx_softmax_bwd_quant_v call -- s, dp, mask, both pairs, m, Z, D -- is a
body inside its own pattern-filled allocation.  After the launches every margin must be intact, every input byte-identical and every
output equal to the CPU path bit for bit (tests/test_mx_softmax_train.py pins that to the definition).  Output allocations are filled
with 0xA5, the margins of the inputs with 0xFF -- a NaN in all three dtypes, so an over-read that enters a maximum or a sum shows as a
NaN row.

The bases are where the header allows them weakest: codes and scales at odd addresses, s, dp and mask off one element, m, Z and D off
one float.  T = 33 crosses the block of 32 along T; S = 33 is a short second block, S = 197 the headline's odd row of four tiles."""
import ctypes

import pytest
import torch

import mx_softmax_ref as SR
from mx_guard import guarded, intact
from qsparse_amd import _hip, mx_softmax_backward_quantize, mx_softmax_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_SOFTMAX_ROUTE_VEC, _hip.MX_SOFTMAX_ROUTE_PLAIN
OUT, NAN = 0xA5, 0xFF       # the fill of an output's allocation; of an input's margins
SCALE = 0.37
SHAPES = ((2, 33, 33), (2, 33, 197))
MODES = ("none", "mask_ts", "mask_gts", "causal")
WEAKEST = {"row_codes": 3, "row_scales": 1, "col_codes": 1, "col_scales": 1, "s": 1, "dp": 1, "mask": 1, "m": 1, "Z": 1, "D": 1}
_refs = {}


def _reference(dtype, fmt, shape, mode, sr):
    key = (dtype, fmt, shape, mode, sr)
    if key not in _refs:
        G, T, S = shape
        s = SR.scores(1000 * S + T, shape, dtype)
        dp = torch.randn(shape, generator=torch.Generator().manual_seed(S)).to(dtype)
        mask = SR.float_mask(S + T, {"mask_ts": (T, S), "mask_gts": shape}[mode]) if mode.startswith("mask") else None
        fwd = mx_softmax_quantize(s, mask, scale=SCALE, is_causal=mode == "causal", fmt=fmt, col_fmt=fmt, return_stats=True)
        bwd = mx_softmax_backward_quantize(dp, s, fwd[4], fwd[5], mask, scale=SCALE, is_causal=mode == "causal", row_fmt=fmt, col_fmt=fmt,
                                           rounding="stochastic" if sr else "nearest", seed=17,
                                           step=torch.tensor([2], dtype=torch.int64) if sr else None)
        _refs[key] = ((s, dp, mask), fwd, bwd)
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


PAIRS = ("row_codes", "row_scales", "col_codes", "col_scales")


def _run(lib, dtype, fmt, shape, mode, offs, sr):
    (s, dp, mask), fwd, bwd = _reference(dtype, fmt, shape, mode, sr)
    what = (dtype, fmt, shape, mode, sorted(offs), sr)
    G, T, S = shape
    es = s.element_size()
    ins = {"s": _Operand(s.numel() * es, offs.get("s", 0) * es, s), "dp": _Operand(dp.numel() * es, offs.get("dp", 0) * es, dp)}
    if mask is not None:
        ins["mask"] = _Operand(mask.numel() * 4, offs.get("mask", 0) * 4, mask)
    mptr = ins["mask"].ptr if mask is not None else None

    # ---- the forward: both pairs, m and Z ----
    outs = {n: _Operand(fwd[i].numel(), offs.get(n, 0)) for i, n in enumerate(PAIRS)}
    outs.update({n: _Operand(G * T * 4, offs.get(n, 0) * 4) for n in ("m", "Z")})
    a = _hip.MxSoftmaxQuant2Args()
    a.struct_size = ctypes.sizeof(a)
    a.row_format = a.col_format = _hip.MX_FORMATS.index(fmt)
    a.sdt, a.causal, a.scale = _hip._DT[dtype], int(mode == "causal"), SCALE
    a.s, a.mask, a.mask_slices = ins["s"].ptr, mptr, G if mode == "mask_gts" else 1
    a.row_codes, a.row_scales, a.col_codes, a.col_scales = (outs[n].ptr for n in PAIRS)
    a.m, a.Z = outs["m"].ptr, outs["Z"].ptr
    a.G, a.T, a.S = shape
    a.stream = _hip._stream(ins["s"].body)
    assert lib.qs_mx_softmax_quant2_route(ctypes.byref(a)) == PLAIN, what       # (S % 32 != 0)
    assert lib.qs_mx_softmax_quant2_v(ctypes.byref(a)) == 0, what
    torch.cuda.synchronize()
    for n, ref in zip(PAIRS + ("m", "Z"), fwd):
        assert outs[n].margins(), (n, what)
        assert torch.equal(outs[n].body.cpu(), _bytes(ref)), (n, what)

    # ---- the backward: both pairs, D ----
    bouts = {n: _Operand(bwd[i].numel(), offs.get(n, 0)) for i, n in enumerate(PAIRS)}
    bouts["D"] = _Operand(G * T * 4, offs.get("D", 0) * 4)
    step = torch.tensor([2], dtype=torch.int64, device=DEV)
    b = _hip.MxSoftmaxBwdQuantArgs()
    b.struct_size = ctypes.sizeof(b)
    b.row_format = b.col_format = _hip.MX_FORMATS.index(fmt)
    b.sdt = b.ddt = _hip._DT[dtype]
    b.causal, b.scale, b.rounding = int(mode == "causal"), SCALE, int(sr)
    b.dp, b.s, b.mask, b.mask_slices = ins["dp"].ptr, ins["s"].ptr, mptr, G if mode == "mask_gts" else 1
    b.m, b.Z, b.D = outs["m"].ptr, outs["Z"].ptr, bouts["D"].ptr
    b.row_codes, b.row_scales, b.col_codes, b.col_scales = (bouts[n].ptr for n in PAIRS)
    b.G, b.T, b.S = shape
    b.stream = a.stream
    b.seed, b.step, b.index_base = 17, step.data_ptr() if sr else None, 0
    assert lib.qs_mx_softmax_bwd_quant_route(ctypes.byref(b)) == PLAIN, what
    assert lib.qs_mx_softmax_bwd_quant_v(ctypes.byref(b)) == 0, what
    torch.cuda.synchronize()
    for n, op in ins.items():
        assert op.margins() and torch.equal(op.body.cpu(), op.data), (n, what)
    for n in ("m", "Z"):                                          # read by the backward, not written
        assert outs[n].margins() and torch.equal(outs[n].body.cpu(), _bytes(fwd[4 if n == "m" else 5])), (n, what)
    assert bouts["D"].margins(), what
    for n, ref in zip(PAIRS, bwd):
        assert bouts[n].margins(), (n, what)
        assert torch.equal(bouts[n].body.cpu(), _bytes(ref)), (n, what)


@pytest.mark.parametrize("fmt,sr", (("mxfp8_e4m3", False), ("mxfp4_e2m1", True)))
@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
def test_margins_survive(dtype, fmt, sr):
    lib = _hip.load()
    for shape in SHAPES:
        for mode in MODES:
            for offs in ({}, WEAKEST):
                _run(lib, dtype, fmt, shape, mode, offs, sr)
