"""The steady-state fast path of the fused prune -> quantize pair (`fused._FastPair`): once the schedules have finished, a step only
compares a signature of everything the full path's decisions depend on, advances the counters and issues the same composite call.

A pair WITH the fast path and a twin WITHOUT it (arming disabled) run the same steps through a series of disturbances -- each of
which must send the next step through the full path: evaluation / training switches, another input shape or layout, a hook, an
option, a configuration attribute (`stop_mask_refresh`: the mask freezes), a counter written from outside, a parameter re-created
by `.to()` -- and agree bit for bit on outputs, gradients and every state tensor at every step (reference semantics:
sparse.py:215-273, quantize.py:473-518, which `tests/test_site_composite_gpu.py` pins for the full path against the oracle)."""
import pytest
import torch
import torch.nn as nn

import qsparse_amd as qs
import site_plan_guard
from golden_io import same
from qsparse_amd import fused
from qsparse_amd.fused import FusedPruneQuantize

pytestmark = pytest.mark.gpu
_site_plan_guard = site_plan_guard.fixture()      # every composite site launch is checked against its plan first
qs.set_qsparse_options(log_on_created=False, log_during_train=False)
DEV = "cuda"


def make(act, kind="scaler", **cbkw):
    p = qs.prune(sparsity=0.5, start=1, interval=1, repetition=2, dimensions={1},
                 callback=qs.MagnitudePruningCallback(**cbkw))
    q = qs.quantize(bits=4, timeout=2, channelwise=-1, callback=qs.ScalerQuantizer() if kind == "scaler" else qs.DecimalQuantizer())
    return FusedPruneQuantize(nn.Sequential(act, p), q).to(DEV).train()


def state(m):
    p, q = m[0][1], m[1]
    return [p.mask, getattr(p.callback, "magnitude", p.callback.t), q.weight, p._n_updates, q._n_updates, p.callback.t, p._cur_sparsity,
            torch.tensor(q.callback.t)]


def data(step, shape, dtype, channels_last):
    g = torch.Generator().manual_seed(500 + step)
    x = (torch.randn(shape, generator=g) * torch.linspace(0.3, 3, shape[1]).view(1, -1, 1, 1)).to(dtype)
    gr = torch.randn(shape, generator=g)
    if channels_last:
        x, gr = x.contiguous(memory_format=torch.channels_last), gr.contiguous(memory_format=torch.channels_last)
    return x.to(DEV), gr.to(DEV)


class Runs:
    """counts which route each forward of the pair took"""

    def __init__(self, monkeypatch):
        self.fast = self.full = 0
        real_try, real_full = fused._FastPair.try_run, fused.fused_prune_quantize

        def try_run(f, seq, x):
            out = real_try(f, seq, x)
            if out is not fused._MISS and type(out) is not fused._ActMiss:
                self.fast += 1
            return out

        def full(*a, **k):
            self.full += 1
            return real_full(*a, **k)

        monkeypatch.setattr(fused._FastPair, "try_run", try_run)
        monkeypatch.setattr(fused, "fused_prune_quantize", full)


@pytest.mark.parametrize("act,inplace", [("relu", False), ("relu", True), ("identity", False), ("relu6", False)])
@pytest.mark.parametrize("kind", ["scaler", "decimal"])
def test_fast_path_equals_the_full_path_through_disturbances(act, inplace, kind, monkeypatch):
    mk = {"relu": lambda: nn.ReLU(inplace=inplace), "identity": lambda: nn.Identity(), "relu6": lambda: nn.ReLU6()}[act]
    a, b = make(mk(), kind), make(mk(), kind)
    runs = Runs(monkeypatch)
    real_arm = fused._FastPair.arm
    monkeypatch.setattr(fused._FastPair, "arm", classmethod(lambda cls, seq, *r: None if seq is b else real_arm.__func__(cls, seq, *r)))
    shape, dtype, cl = (6, 16, 8, 8), torch.bfloat16, False
    log = []
    handle = None
    for step in range(40):
        # ---- disturbances, the same for both ----
        if step == 12:
            a.eval(), b.eval()
        if step == 13:
            a.train(), b.train()
        if step == 16:
            shape = (4, 16, 6, 10)
        if step == 19:
            cl = True
        if step == 22:
            qs.set_qsparse_options(relu_gate=False)
        if step == 24:
            qs.set_qsparse_options(relu_gate=True)
        if step == 26:
            handle = (a[0][1].register_forward_hook(lambda *_: None), b[0][1].register_forward_hook(lambda *_: None))
        if step == 28:
            handle[0].remove(), handle[1].remove()
        if step == 30:          # the mask freezes from here on (the steady state of the layerwise recipe)
            a[0][1].callback.stop_mask_refresh = b[0][1].callback.stop_mask_refresh = 5
        if step == 33:          # a counter written from outside (a checkpoint being loaded, say)
            with torch.no_grad():
                a[1]._n_updates.add_(3), b[1]._n_updates.add_(3)
        if step == 36:          # parameters re-created: the state tensors are other objects now
            a.to(torch.device(DEV)), b.to(torch.device(DEV))
            a[0][1].mask = nn.Parameter(a[0][1].mask.detach().clone(), requires_grad=False)
            b[0][1].mask = nn.Parameter(b[0][1].mask.detach().clone(), requires_grad=False)
        x, gr = data(step, shape, dtype, cl)
        outs = []
        before = (runs.fast, runs.full)
        for m in (a, b):
            xd = x.clone().requires_grad_(True)
            y = m(xd.clone() if inplace else xd)
            (gx,) = torch.autograd.grad(y, xd, gr.to(y.dtype))
            outs.append((y.detach(), gx))
        log.append((step, runs.fast - before[0], runs.full - before[1]))
        assert same(outs[0][0].cpu(), outs[1][0].cpu()) and same(outs[0][1].cpu(), outs[1][1].cpu()), ("output / gradient", step)
        for sa, sb in zip(state(a), state(b)):
            assert same(sa.detach().cpu(), sb.detach().cpu()), ("state", step)
    qs.set_qsparse_options(relu_gate=True)
    took = {s: (f, u) for s, f, u in log}
    # the pair with the fast path: full path while the schedules run and right after every disturbance, fast path in between
    for s in (8, 9, 10, 11, 15, 18, 21, 25, 29, 32, 35, 39):
        assert took[s][0] == 1, (s, log)
    for s in (0, 1, 2, 12, 13, 16, 19, 22, 24, 26, 27, 28, 30, 36):
        assert took[s][0] == 0, (s, log)
    assert took[33][0] == 1          # (a counter written from outside is simply re-read: the host mirror sees the version counter)


def test_fast_path_is_not_copied_and_survives_deepcopy_and_state_dict_round_trips(monkeypatch):
    import copy
    a = make(nn.ReLU())
    for step in range(8):
        x, gr = data(step, (6, 16, 8, 8), torch.float32, False)
        x.requires_grad_(True)
        torch.autograd.grad(a(x), x, gr)
    assert a.__dict__.get("_qs_fast") is not None
    b = copy.deepcopy(a)
    assert b.__dict__.get("_qs_fast") is None                      # raw pointers never travel
    sd = {k: v.clone() for k, v in a.state_dict().items()}
    for step in range(8, 14):
        x, gr = data(step, (6, 16, 8, 8), torch.float32, False)
        outs = []
        for m in (a, b):
            xd = x.clone().requires_grad_(True)
            y = m(xd)
            outs.append((y.detach().cpu(), torch.autograd.grad(y, xd, gr)[0].cpu()))
        assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1]), step
    a.load_state_dict(sd)                                          # in-place copies: the host mirrors see the version counters
    b.load_state_dict(sd)
    for step in range(14, 18):
        x, gr = data(step, (6, 16, 8, 8), torch.float32, False)
        outs = []
        for m in (a, b):
            xd = x.clone().requires_grad_(True)
            y = m(xd)
            outs.append((y.detach().cpu(), torch.autograd.grad(y, xd, gr)[0].cpu()))
        assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1]), step
        for sa, sb in zip(state(a), state(b)):
            assert same(sa.detach().cpu(), sb.detach().cpu()), step
