"""The plan-consistency guard of `site_plan_guard.py` itself (no GPU): the wrapped `_hip.site_fwd` / `site_stats` / `site_bwd` are handed
CPU tensors that disagree with a hand-built `SitePlanStruct` in one field each -- numel, dtype, layout, alignment, gate size, device, the
riders -- and must raise `AssertionError` naming that field before anything reaches the library (`_hip.load` is a recorder here); a
consistent call passes through unchanged."""
import ctypes

import pytest
import torch

import site_plan_guard
from qsparse_amd import _hip

_site_plan_guard = site_plan_guard.fixture()

N, C, H, W = 2, 8, 4, 4
NUMEL = N * C * H * W


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("qs_site_"):
            raise AttributeError(name)
        return lambda *a: (self.calls.append((name, a)), 0)[1]


@pytest.fixture
def rec(monkeypatch, plan_guard):
    r = Recorder()
    monkeypatch.setattr(_hip, "load", lambda: r)
    monkeypatch.setattr(_hip, "_stream", lambda t: None)
    return r


def plan(layout=0, xdt=torch.bfloat16, ydt=torch.float32, n=N, c=C, h=H, w=W):
    s = _hip.SitePlanStruct()
    s.N, s.C, s.H, s.W = n, c, h, w
    s.layout, s.xdt, s.ydt, s.bits = layout, _hip._DT[xdt], _hip._DT[ydt], 4
    return s, ctypes.byref(s)


def t(shape=(N, C, H, W), dtype=torch.bfloat16, cl=False):
    x = torch.zeros(shape, dtype=dtype)
    return x.contiguous(memory_format=torch.channels_last) if cl else x


def misaligned(shape=(N, C, H, W), dtype=torch.bfloat16):
    n = 1
    for s in shape:
        n *= s
    buf = torch.zeros(n + 16, dtype=dtype)
    off = 1 if buf.data_ptr() % 16 == 0 else 0
    x = buf[off:off + n].view(shape)
    assert x.data_ptr() % 16
    return x


def gate(nbytes=(NUMEL + 7) // 8):
    return torch.zeros(nbytes, dtype=torch.uint8)


def fwd(ref, **over):
    a = dict(x=t(), y=t(dtype=torch.float32), gate_bits=gate(), flags=_hip.SITE_LIVE, t_mag=1, k=3, t_q=2)
    a.update(over)
    return _hip.site_fwd(ref, a.pop("x"), a.pop("y"), a.pop("gate_bits"), a.pop("flags"), a.pop("t_mag"), a.pop("k"), a.pop("t_q"), **a)


def bwd(ref, **over):
    a = dict(g=t(dtype=torch.float32), gate_bits=gate(), gx=t(), flags=0, lo_mul=-8.0, hi_mul=7.0)
    a.update(over)
    return _hip.site_bwd(ref, a.pop("g"), a.pop("gate_bits"), a.pop("gx"), a.pop("flags"), a.pop("lo_mul"), a.pop("hi_mul"), **a)


FWD_CASES = [
    ("numel", dict(x=t((N, C, H, W + 1)))),
    ("numel", dict(y=t((N, C, H - 1, W), dtype=torch.float32))),
    ("dtype", dict(x=t(dtype=torch.float32))),
    ("dtype", dict(y=t(dtype=torch.bfloat16))),
    ("layout", dict(x=t(cl=True))),                                  # channels_last x, NCHW plan
    ("layout", dict(x=t((N, C, W, H)).transpose(2, 3))),             # same numel and shape, other strides
    ("layout", dict(x=t((N, C * H, W)))),                            # same numel, other shape
    ("alignment", dict(x=misaligned())),
    ("alignment", dict(y=misaligned(dtype=torch.float32))),
    ("gate.size", dict(gate_bits=gate((NUMEL + 7) // 8 - 1))),
    ("gate.dtype", dict(gate_bits=torch.zeros((NUMEL + 7) // 8, dtype=torch.int8))),
    ("image.numel", dict(image=t((N, C, H, W - 1)))),
    ("image.dtype", dict(image=t(dtype=torch.float32))),
    ("decimal.dtype", dict(decimal=torch.zeros(1, dtype=torch.float64))),
    ("gathered.size", dict(gathered=torch.zeros(2 * 2 * C - 1), world=2)),
    ("xback", dict(xback=torch.zeros(NUMEL, dtype=torch.bfloat16))),
]


@pytest.mark.parametrize("field,over", FWD_CASES, ids=[f"{f}-{i}" for i, (f, _) in enumerate(FWD_CASES)])
def test_forward_mismatch_raises_before_the_native_call(field, over, rec):
    _, ref = plan()
    with pytest.raises(AssertionError, match=field.replace(".", r"\.")):
        fwd(ref, **over)
    assert rec.calls == []


BWD_CASES = [
    ("gx.numel", dict(gx=t((N, C, H, 2 * W)))),
    ("gx.dtype", dict(gx=t(dtype=torch.float32))),
    ("g.dtype", dict(g=t(dtype=torch.float16))),
    ("g.layout", dict(g=t(dtype=torch.float32, cl=True))),
    ("g.alignment", dict(g=misaligned(dtype=torch.float32))),
    ("gate.size", dict(gate_bits=gate(3))),
    ("g2.dtype", dict(g2=t(dtype=torch.float32))),
    ("g3.numel", dict(g3=t((N, C, H, W + 2)))),
    ("gx_image.layout", dict(gx_image=t(cl=True))),
    ("act_x.dtype", dict(act_x=t(dtype=torch.float32))),
    ("act_x.numel", dict(act_x=t((N + 1, C, H, W)))),
]


@pytest.mark.parametrize("field,over", BWD_CASES, ids=[f"{f}-{i}" for i, (f, _) in enumerate(BWD_CASES)])
def test_backward_mismatch_raises_before_the_native_call(field, over, rec):
    _, ref = plan()
    with pytest.raises(AssertionError, match=field.replace(".", r"\.")):
        bwd(ref, **over)
    assert rec.calls == []


def test_other_layouts_and_stats(rec):
    # channels_last plan: an NCHW x is the wrong layout, a channels_last one passes
    _, ref = plan(layout=1)
    with pytest.raises(AssertionError, match="x.layout"):
        fwd(ref, y=t(dtype=torch.float32, cl=True))
    fwd(ref, x=t(cl=True), y=t(dtype=torch.float32, cl=True))
    # 2-d and token-major plans
    _, ref2 = plan(layout=2, n=16, c=8, h=1, w=1)
    fwd(ref2, x=t((16, 8)), y=t((16, 8), dtype=torch.float32), gate_bits=gate(16))
    with pytest.raises(AssertionError, match="x.layout"):
        fwd(ref2, x=t((8, 16)).t(), y=t((16, 8), dtype=torch.float32), gate_bits=gate(16))
    _, ref3 = plan(layout=3, n=2, c=8, h=5, w=1)
    fwd(ref3, x=t((2, 5, 8)), y=t((2, 5, 8), dtype=torch.float32), gate_bits=gate(10))
    with pytest.raises(AssertionError, match="x.layout"):
        fwd(ref3, x=t((2, 8, 5)), y=t((2, 8, 5), dtype=torch.float32), gate_bits=gate(10))
    assert [c[0] for c in rec.calls] == ["qs_site_fwd"] * 3
    # the statistics half: x and the record
    _, ref = plan()
    with pytest.raises(AssertionError, match="record.size"):
        _hip.site_stats(ref, t(), 0, torch.zeros(2 * C - 1))
    with pytest.raises(AssertionError, match="x.numel"):
        _hip.site_stats(ref, t((N, C, H, W + 1)), 0, torch.zeros(2 * C))
    _hip.site_stats(ref, t(), 0, torch.zeros(2 * C))
    assert [c[0] for c in rec.calls] == ["qs_site_fwd"] * 3 + ["qs_site_stats"]


def test_plan_device_is_the_one_it_was_built_for(rec):
    s, ref = plan()
    s._guard_device = torch.device("meta")       # (what `fused._site_plan` records under the guard)
    with pytest.raises(AssertionError, match="x.device"):
        fwd(ref)
    assert rec.calls == []


def test_consistent_calls_pass_through_unchanged(rec, plan_guard, monkeypatch):
    _, ref = plan()
    x, y, bits, img, dec = t(), t(dtype=torch.float32), gate(), t(), torch.zeros(1)
    fwd(ref, x=x, y=y, gate_bits=bits, image=img, decimal=dec, xback=True)
    g, gx, g2 = t(dtype=torch.float32), t(), t()
    bwd(ref, g=g, gate_bits=bits, gx=gx, g2=g2, decimal=dec)
    assert plan_guard.checked == {"site_fwd": 1, "site_stats": 0, "site_bwd": 1}
    guarded = list(rec.calls)
    # the same calls without the guard reach the library with the same arguments
    rec.calls.clear()
    for name in ("site_fwd", "site_bwd"):
        monkeypatch.setattr(_hip, name, getattr(_hip, name).__wrapped__)
    fwd(ref, x=x, y=y, gate_bits=bits, image=img, decimal=dec, xback=True)
    bwd(ref, g=g, gate_bits=bits, gx=gx, g2=g2, decimal=dec)
    assert [c[0] for c in guarded] == ["qs_site_fwd", "qs_site_bwd"] and guarded == rec.calls
