"""Plan-consistency guard for the composite site calls (`_hip.site_fwd` / `site_stats` / `site_bwd`).

Those entry points get no sizes from their caller: only pointers and a cached `qs_site_plan` (`_hip.SitePlanStruct`: N, C, H, W,
layout, dtype codes, state pointers) built once by `fused._site_plan` or `sparse._prune_plan`.  A tensor launched with a plan built for
another geometry makes the kernels read and write out of bounds, or process part of the tensor.  The guard wraps the three entry
points and, BEFORE the native call, checks every tensor operand against the plan:

  * x (and, in the backward, g / g2 / g3 / gx / act_x / gx_image): numel == N*C*H*W, the shape and dense strides the plan's layout
    names (0 NCHW-contiguous, 1 channels_last, 2 `(N, C)`, 3 token-major `(N, T=H, C)`; extents of 1 carry any stride), 16-byte
    aligned, on the plan's device; x, gx and act_x have dtype code `xdt`, y has `ydt`;
  * the gate bitmap holds at least ceil(numel / 8) bytes; the autocast image has x's geometry; `xback` aliases x;
  * the per-call scalars' buffers (decimal step, exchange record, gathered records) are float32 and large enough.

A mismatch raises `AssertionError` naming the field, so a stale plan fails a test in Python and never reaches the GPU.

A test module turns it on for every test with one line::

    _site_plan_guard = site_plan_guard.fixture()

(the fixture, `plan_guard`, is a `Guard`, whose `checked` counts the launches it let through)."""
import inspect

import pytest
import torch

from qsparse_amd import _hip, fused, sparse

_BY_CODE = {code: dt for dt, code in _hip._DT.items()}
_HALF = (torch.bfloat16, torch.float16)


def plan_struct(plan_ref) -> "_hip.SitePlanStruct":
    """the `SitePlanStruct` behind `ctypes.byref(struct)` (or the struct itself)"""
    c = getattr(plan_ref, "_obj", plan_ref)
    assert isinstance(c, _hip.SitePlanStruct), f"plan: {type(c).__name__} is not a SitePlanStruct"
    return c


def geometry(c):
    """(shape, dense strides) of a tensor of the plan's layout"""
    N, C, H, W = int(c.N), int(c.C), int(c.H), int(c.W)
    if c.layout == 0:
        return (N, C, H, W), (C * H * W, H * W, W, 1)
    if c.layout == 1:
        return (N, C, H, W), (H * W * C, 1, W * C, C)
    if c.layout == 2:
        return (N, C), (C, 1)
    if c.layout == 3:
        return (N, H, C), (H * C, C, 1)
    raise AssertionError(f"plan.layout: {c.layout} is not a qs_site_plan layout")


def _fail(what):
    raise AssertionError("site plan guard: " + what)


def check_like_plan(name, t, c, device, dtype=None, dtypes=None):
    """t is a dense tensor of the plan's geometry (and of `dtype`, or one of `dtypes`) on `device`"""
    if not isinstance(t, torch.Tensor):
        _fail(f"{name}: {type(t).__name__} is not a tensor")
    shape, strides = geometry(c)
    numel = c.N * c.C * c.H * c.W
    if t.numel() != numel:
        _fail(f"{name}.numel {t.numel()} != plan N*C*H*W = {numel} (plan {tuple(shape)})")
    if dtype is not None and t.dtype != dtype:
        _fail(f"{name}.dtype {t.dtype} != plan dtype {dtype}")
    if dtypes is not None and t.dtype not in dtypes:
        _fail(f"{name}.dtype {t.dtype} not in {dtypes}")
    if tuple(t.shape) != shape or any(s != d for s, d, n in zip(t.stride(), strides, shape) if n != 1):
        _fail(f"{name}.layout: shape {tuple(t.shape)} strides {t.stride()} are not the dense ones of plan.layout {c.layout} "
              f"(shape {shape} strides {strides})")
    if t.data_ptr() % 16:
        _fail(f"{name}.alignment: data_ptr % 16 == {t.data_ptr() % 16}")
    if t.device != device:
        _fail(f"{name}.device {t.device} != plan device {device}")


def check_buffer(name, t, device, dtype, min_bytes):
    if not isinstance(t, torch.Tensor):
        _fail(f"{name}: {type(t).__name__} is not a tensor")
    if t.dtype != dtype:
        _fail(f"{name}.dtype {t.dtype} != {dtype}")
    if not t.is_contiguous():
        _fail(f"{name}.layout: not contiguous")
    if t.numel() * t.element_size() < min_bytes:
        _fail(f"{name}.size: {t.numel() * t.element_size()} bytes < {min_bytes}")
    if t.device != device:
        _fail(f"{name}.device {t.device} != plan device {device}")


def _device(c, x):
    dev = getattr(c, "_guard_device", None)
    return dev if dev is not None else x.device


def _xdt(c):
    dt = _BY_CODE.get(int(c.xdt))
    if dt is None:
        _fail(f"plan.xdt: {c.xdt} is not a dtype code")
    return dt


def _gate(gate, c, device):
    if gate is not None:
        check_buffer("gate", gate, device, torch.uint8, (c.N * c.C * c.H * c.W + 7) // 8)


def check_fwd(plan_ref, x, y, gate_bits, flags, t_mag, k, t_q, image=None, gathered=None, world=1, xback=False, decimal=None):
    c = plan_struct(plan_ref)
    dev = _device(c, x)
    check_like_plan("x", x, c, dev, dtype=_xdt(c))
    ydt = _BY_CODE.get(int(c.ydt))
    if ydt is None:
        _fail(f"plan.ydt: {c.ydt} is not a dtype code")
    check_like_plan("y", y, c, dev, dtype=ydt)
    _gate(gate_bits, c, dev)
    if image is not None:
        check_like_plan("image", image, c, dev, dtypes=_HALF)
    if gathered is not None:
        check_buffer("gathered", gathered, dev, torch.float32, int(world) * 2 * c.C * 4)
    if isinstance(xback, torch.Tensor):
        if xback.data_ptr() != x.data_ptr():
            _fail("xback: does not alias x")
    elif xback not in (True, False):
        _fail(f"xback: {xback!r}")
    if decimal is not None:
        check_buffer("decimal", decimal, dev, torch.float32, 4)


def check_stats(plan_ref, x, flags, record):
    c = plan_struct(plan_ref)
    dev = _device(c, x)
    check_like_plan("x", x, c, dev, dtype=_xdt(c))
    check_buffer("record", record, dev, torch.float32, 2 * c.C * 4)


def check_bwd(plan_ref, g, gate_bits, gx, flags, lo_mul, hi_mul, g2=None, decimal=None, g3=None, gx_image=None, act_x=None):
    c = plan_struct(plan_ref)
    dev = _device(c, gx)
    xdt = _xdt(c)
    check_like_plan("gx", gx, c, dev, dtype=xdt)
    if g is not None:
        check_like_plan("g", g, c, dev, dtypes=(torch.float32, xdt))
    _gate(gate_bits, c, dev)
    for name, t in (("g2", g2), ("g3", g3), ("gx_image", gx_image)):
        if t is not None:
            check_like_plan(name, t, c, dev, dtypes=_HALF)
    if act_x is not None:
        check_like_plan("act_x", act_x, c, dev, dtype=xdt)
    if decimal is not None:
        check_buffer("decimal", decimal, dev, torch.float32, 4)


class Guard:
    """wraps the entry points of `_hip` (through `monkeypatch`) with the checks above"""

    def __init__(self, monkeypatch):
        self.checked = {"site_fwd": 0, "site_stats": 0, "site_bwd": 0}
        for name, check in (("site_fwd", check_fwd), ("site_stats", check_stats), ("site_bwd", check_bwd)):
            monkeypatch.setattr(_hip, name, self._wrap(name, getattr(_hip, name), check))
        # the plan's device: what the plan was built for (a hand-built struct has none: x's device then)
        monkeypatch.setattr(fused, "_site_plan", self._tag(fused._site_plan, "h"))
        monkeypatch.setattr(sparse, "_prune_plan", self._tag(sparse._prune_plan, "x"))

    def _wrap(self, name, real, check):
        sig = inspect.signature(real)

        def guarded(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            check(**b.arguments)
            self.checked[name] += 1
            return real(*a, **k)

        guarded.__wrapped__ = real
        return guarded

    @staticmethod
    def _tag(real, arg):
        sig = inspect.signature(getattr(real, "__wrapped__", real))

        def tagged(*a, **k):
            plan = real(*a, **k)
            if plan is not None:
                plan.c._guard_device = sig.bind(*a, **k).arguments[arg].device
            return plan

        tagged.__wrapped__ = real
        return tagged


def fixture():
    """an autouse fixture for the calling module: every test in it runs behind the guard"""

    @pytest.fixture(autouse=True, name="plan_guard")
    def plan_guard(monkeypatch):
        return Guard(monkeypatch)

    return plan_guard
