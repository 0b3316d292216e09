"""Out-of-bounds check for the MX softmax quantizer, in the manner of tests/test_mx_norm_canary_gpu.py, through the C ABI: every pointer
of a qs_mx_softmax_quant_v call -- s, mask, codes, scales -- is a body inside its own pattern-filled allocation.  After the launch every
margin must be intact, every input byte-identical and both outputs equal to the CPU path of ``mx_softmax_quantize`` bit for bit
(tests/test_mx_softmax.py pins that to the definition).  Output allocations are filled with 0xA5, the margins of the inputs with 0xFF --
a NaN in all three dtypes, so an over-read that enters a maximum or a sum shows as a NaN row: 0xFF scale bytes.

The bases are where the header allows them weakest: codes off 1, 2 and 3 bytes, scales at odd addresses, s and mask off one element.
The shapes are the smallest at which a mechanism changes: one element, the block of 32, a short last block, the pass of 512, a second
pass, the headline's odd row of 197; T crosses the four rows of a work-group."""
import ctypes

import pytest
import torch

import mx_softmax_ref as SR
from mx_guard import guarded, intact
from qsparse_amd import _hip, mx_softmax_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_SOFTMAX_ROUTE_VEC, _hip.MX_SOFTMAX_ROUTE_PLAIN
OUT, NAN = 0xA5, 0xFF       # the fill of an output's allocation; of an input's margins
SCALE = 0.37
SHAPES = ((1, 1, 1), (1, 1, 32), (2, 5, 33), (1, 4, 512), (1, 3, 520), (2, 9, 197))
MODES = ("none", "mask_ts", "mask_gts", "causal")
WEAKEST = {"codes": 3, "scales": 1, "s": 1, "mask": 1}
OFFSETS = ({}, {"codes": 1}, {"codes": 2}, {"codes": 3}, {"scales": 1}, {"s": 1}, {"mask": 1}, WEAKEST, {"codes": 8, "scales": 3})
_refs = {}


def _reference(dtype, fmt, shape, mode):
    """the inputs and what the CPU path makes of them, computed once per key: (s, mask | None), (codes, scales)"""
    key = (dtype, fmt, shape, mode)
    if key not in _refs:
        G, T, S = shape
        s = SR.scores(1000 * S + T, shape, dtype)
        mask = SR.float_mask(S + T, {"mask_ts": (T, S), "mask_gts": shape}[mode]) if mode.startswith("mask") else None
        codes, scales = mx_softmax_quantize(s, mask, scale=SCALE, is_causal=mode == "causal", fmt=fmt)
        assert not bool((scales == 0xFF).any()), key      # the reference alone is finite: no block is NaN by the inputs' own doing
        _refs[key] = ((s, mask), (codes, scales))
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


def _run(lib, dtype, fmt, shape, mode, offs):
    """one guarded call with every check of this file; returns (outputs, route)"""
    (s, mask), (codes, scales) = _reference(dtype, fmt, shape, mode)
    what = (dtype, fmt, shape, mode, offs)
    G, T, S = shape
    ins = {"s": _Operand(s.numel() * s.element_size(), offs.get("s", 0) * s.element_size(), s)}
    if mask is not None:
        ins["mask"] = _Operand(mask.numel() * 4, offs.get("mask", 0) * 4, mask)
    outs = {"codes": _Operand(codes.numel(), offs.get("codes", 0)), "scales": _Operand(scales.numel(), offs.get("scales", 0))}

    a = _hip.MxSoftmaxQuantArgs()
    a.struct_size = ctypes.sizeof(a)
    a.format, a.sdt, a.causal, a.scale = _hip.MX_FORMATS.index(fmt), _hip._DT[dtype], int(mode == "causal"), SCALE
    a.s, a.mask = ins["s"].ptr, ins["mask"].ptr if mask is not None else None
    a.mask_slices = G if mode == "mask_gts" else 1
    a.codes, a.scales = outs["codes"].ptr, outs["scales"].ptr
    a.G, a.T, a.S = shape
    a.stream = _hip._stream(ins["s"].body)

    # the documented rule, from the pointers actually passed (an absent mask is a null pointer: aligned)
    mptr = ins["mask"].ptr if mask is not None else 0
    want_route = VEC if S % 32 == 0 and ins["s"].ptr % 16 == 0 and mptr % 16 == 0 and outs["codes"].ptr % 8 == 0 else PLAIN
    assert lib.qs_mx_softmax_quant_route(ctypes.byref(a)) == want_route, what
    assert lib.qs_mx_softmax_quant_v(ctypes.byref(a)) == 0, what
    torch.cuda.synchronize()

    for n, op in ins.items():
        assert op.margins() and torch.equal(op.body.cpu(), op.data), (n, what)
    for n, ref in (("codes", codes), ("scales", scales)):
        assert outs[n].margins(), (n, what)
        assert torch.equal(outs[n].body.cpu(), _bytes(ref)), (n, what)
    return outs, want_route


@pytest.mark.parametrize("fmt", ("mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e3m2"))
@pytest.mark.parametrize("dtype", SR.DTS, ids=str)
def test_margins_survive_every_route(dtype, fmt):
    lib = _hip.load()
    seen = set()
    for shape in SHAPES:
        for mode in MODES:
            for offs in OFFSETS:
                if "mask" in offs and not mode.startswith("mask") and offs is not WEAKEST:
                    continue
                route = _run(lib, dtype, fmt, shape, mode, offs)[1]
                seen.add((route, shape[2] % 32 == 0, tuple(sorted(offs))))
    routes = {r for r, _, _ in seen}
    assert routes == {VEC, PLAIN}
    # an S that would take VEC goes PLAIN for each misaligned base alone; codes off 8 bytes stays VEC
    for n in ("codes", "s", "mask"):
        assert (PLAIN, True, (n,)) in seen, n
    assert (VEC, True, ("codes", "scales")) in seen and (VEC, True, ("scales",)) in seen


def test_the_guard_can_fail():
    """the same call judged with bodies one row shorter than the T the library was given: the last row's legitimate stores lie in what
    is then counted as margin (inside the allocations all the same), and `intact` must say so"""
    G, T, S = 2, 9, 197
    outs, _ = _run(_hip.load(), torch.bfloat16, "mxfp8_e4m3", (G, T, S), "mask_ts", {})
    nb = -(-S // 32)
    for n, short in (("codes", (G * T - 1) * S), ("scales", (G * T - 1) * nb)):
        assert outs[n].margins() and not outs[n].margins(short), n
