"""The steady-state fast path of the fused prune -> quantize pair behind an activation the kernels do not fold (`_FastPair` fold 3:
nn.GELU in either form, nn.SiLU, nn.Tanh, nn.RReLU in training, any module passed to `convert(..., activation_layers=[...])`).  The
site's plan is built for the activation's OUTPUT h, and an activation can change h while x stays the same; the fast path must then
miss -- before anything is launched or advanced -- and the full path continue with that h, without running the activation again.

Method of `test_fast_path_gpu.py`: a pair WITH the fast path and a twin WITHOUT it run the same seeded steps through the same
disturbances and agree bit for bit on outputs, input gradients and every state tensor, and the route of every step is asserted.  The
twin's h is copied to the CPU at every step and `oracle.PruneSim` / `oracle.QuantizeSim` replay it: y, mask, magnitude and scale
equal the oracle's (reference semantics: sparse.py:215-273, quantize.py:473-518).  Every composite launch runs behind the plan
guard (`site_plan_guard.py`): a stale plan fails in Python, never on the device.  The activation runs exactly once per forward on
every route (a random one -- nn.RReLU, dropout -- would otherwise draw twice and leave the reference's module-by-module semantics)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import qsparse_amd as qs
import site_plan_guard
from golden_io import same
from oracle import qs_oracle as O
from qsparse_amd import fused
from qsparse_amd.fused import FusedPruneQuantize, fuse_prune_quantize_pairs
from test_fast_path_gpu import Runs, state

pytestmark = pytest.mark.gpu
_site_plan_guard = site_plan_guard.fixture()      # every composite site launch is checked against its plan first
qs.set_qsparse_options(log_on_created=False, log_during_train=False)
DEV = "cuda"
START, INTERVAL, REPS, TIMEOUT = 1, 1, 2, 2


class Shaper(nn.Module):
    """a random activation (tanh, then dropout) whose attributes change its output h while x stays the same"""

    def __init__(self, cd, rd):
        super().__init__()
        self.cd, self.rd = cd, rd            # the channel dim, the dim `rep` repeats along
        self.rep, self.to_f32, self.flip_layout, self.misalign, self.extra_c = 1, False, False, False, 0

    def forward(self, x):
        h = F.dropout(torch.tanh(x), 0.2, training=True)
        if self.rep > 1:
            h = torch.cat([h] * self.rep, dim=self.rd)
        if self.extra_c:
            h = torch.cat([h, h.narrow(self.cd, 0, self.extra_c)], dim=self.cd)
        if self.to_f32:
            h = h.float()
        if self.flip_layout:
            h = h.contiguous() if not h.is_contiguous() else h.contiguous(memory_format=torch.channels_last)
        if self.misalign:                    # a copy one element into a larger buffer (2 bytes for bf16, 4 for float32)
            buf = torch.empty(h.numel() + 16, dtype=h.dtype, device=h.device)
            m = buf.as_strided(h.shape, h.stride(), 1)
            m.copy_(h)
            h = m
        return h


# x shape, dtype, channels_last, channel dim (the prune layer's `dimensions`), another x shape, oracle anchor
LAYOUTS = {
    "nchw-bf16": ((6, 16, 8, 8), torch.bfloat16, False, 1, (4, 16, 6, 10), True),
    "nchw-f32": ((6, 16, 8, 8), torch.float32, False, 1, (4, 16, 6, 10), True),
    "cl-bf16": ((6, 16, 8, 8), torch.bfloat16, True, 1, (4, 16, 6, 10), False),
    "2d-f32": ((32, 48), torch.float32, False, 1, (24, 48), True),
    "token-bf16": ((4, 10, 32), torch.bfloat16, False, 2, (3, 12, 32), True),
}
ACTS = {
    "gelu": lambda: nn.GELU(),
    "gelu-tanh": lambda: nn.GELU(approximate="tanh"),
    "silu": lambda: nn.SiLU(),
    "tanh": lambda: nn.Tanh(),
    "rrelu": lambda: nn.RReLU(0.1, 0.3),
}


def make(act, kind, cd):
    p = qs.prune(sparsity=0.5, start=START, interval=INTERVAL, repetition=REPS, dimensions={cd})
    q = qs.quantize(bits=4, timeout=TIMEOUT, channelwise=-1, callback=qs.ScalerQuantizer() if kind == "scaler" else qs.DecimalQuantizer())
    return FusedPruneQuantize(nn.Sequential(act, p), q).to(DEV).train()


def data(step, shape, dtype, channels_last, cd):
    g = torch.Generator().manual_seed(900 + step)
    scale = torch.linspace(0.3, 3, shape[cd]).view([-1 if i == cd else 1 for i in range(len(shape))])
    x = (torch.randn(shape, generator=g) * scale).to(dtype)
    gr = torch.randn(shape, generator=g)
    if channels_last:
        x, gr = x.contiguous(memory_format=torch.channels_last), gr.contiguous(memory_format=torch.channels_last)
    return x.to(DEV), gr.to(DEV)


def counted(*acts):
    """a function returning how often the activation modules ran (an instance `forward`: hooks would switch the fast path off)"""
    n = [0]

    def wrap(real):
        def forward(x):
            n[0] += 1
            return real(x)
        return forward

    for act in acts:
        act.forward = wrap(act.forward)
    return lambda: n[0]


class Twins:
    """the pair `a` (fast path) and its twin `b` (arming disabled); h of every full-path step of `b` is recorded"""

    def __init__(self, monkeypatch, mk, kind, cd):
        self.a, self.b = make(mk(), kind, cd), make(mk(), kind, cd)
        self.runs = Runs(monkeypatch)
        real_arm = fused._FastPair.arm
        b = self.b
        monkeypatch.setattr(fused._FastPair, "arm", classmethod(lambda cls, seq, *r: None if seq is b else real_arm.__func__(cls, seq, *r)))
        self.h = None
        real_full = fused.fused_prune_quantize

        def full(p, q, h, *r, **k):
            if p is b[0][1]:
                self.h = h.detach().cpu()
            return real_full(p, q, h, *r, **k)

        monkeypatch.setattr(fused, "fused_prune_quantize", full)

    def step(self, x, gr, seed, calls):
        """one step of both (the same RNG state for each): ((y, gx) or the exception) per model, routes of `a`"""
        outs = []
        before = (self.runs.fast, self.runs.full)
        self.h = None
        for m in (self.a, self.b):
            torch.manual_seed(seed)
            c0 = calls()
            xd = x.clone().requires_grad_(True)
            try:
                y = m(xd)
            except AssertionError:
                raise                    # (the plan guard)
            except Exception as e:       # (the module-by-module route's own error: both must raise it)
                outs.append((type(e), str(e)))
            else:
                if y.shape != gr.shape:  # (an activation that changed the shape)
                    gr = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed)).to(DEV)
                (gx,) = torch.autograd.grad(y, xd, gr.to(y.dtype))
                outs.append((y.detach().as_subclass(torch.Tensor).cpu(), gx.cpu()))
            assert calls() - c0 == 1, ("activation calls in one forward", calls() - c0)
        return outs, self.runs.fast - before[0]


def compare(twins, outs, tag):
    (ya, ga), (yb, gb) = outs
    if isinstance(ya, type):
        assert (ya, ga) == (yb, gb), ("the same error", tag, outs)
    else:
        assert same(ya, yb) and same(ga, gb), ("output / gradient", tag)
    for sa, sb in zip(state(twins.a), state(twins.b)):
        assert same(sa.detach().cpu(), sb.detach().cpu()), ("state", tag)


class Oracle:
    def __init__(self, kind, cd):
        self.psim = O.PruneSim(0.5, [cd], START, INTERVAL, REPS, False)
        self.qsim = O.QuantizeSim(kind, 4, -1, TIMEOUT)

    def step(self, h, training, y, m, tag):
        """replays the twin's h; y: the twin's output (or the error it raised), m: the twin"""
        if isinstance(y, type):
            with pytest.raises(Exception):
                self.qsim.step(self.psim.step(h, training), training)
        else:
            y_ref = self.qsim.step(self.psim.step(h, training).contiguous(), training)
            assert y.dtype == y_ref.dtype and same(y.contiguous(), y_ref.contiguous()), ("output vs oracle", tag)
        p, q = m[0][1], m[1]
        assert same(p.mask.detach().cpu(), self.psim.mask), ("mask vs oracle", tag)
        if self.psim.magnitude is not None:
            assert same(p.callback.magnitude.detach().cpu(), self.psim.magnitude), ("magnitude vs oracle", tag)
        assert same(q.weight.detach().cpu(), self.qsim.weight), ("scale vs oracle", tag)
        assert p._n_updates.item() == self.psim.n_updates and q._n_updates.item() == self.qsim.n_updates, ("counters vs oracle", tag)


@pytest.mark.parametrize("kind", ["scaler", "decimal"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("act", list(ACTS) + ["shaper"])
def test_fast_path_behind_an_unfolded_activation_equals_the_full_path(act, layout, kind, monkeypatch, plan_guard):
    shape, dtype, cl, cd, shape2, anchor = LAYOUTS[layout]
    four = len(shape) == 4
    rd = 3 if four else (1 if cd == 2 else 0)
    mk = (lambda: Shaper(cd, rd)) if act == "shaper" else ACTS[act]
    tw = Twins(monkeypatch, mk, kind, cd)
    acts = (tw.a[0][0], tw.b[0][0])
    calls = counted(*acts)
    oracle = Oracle(kind, cd) if anchor else None

    def shaper(**kw):
        for m in acts:
            for k, v in kw.items():
                setattr(m, k, v)

    # disturbances after the schedules have finished and the pair has armed (x's signature unchanged unless stated)
    plan = {6: "x shape", 8: "eval", 9: "train"}
    if act == "shaper":
        plan.update({11: "grow", 13: "shrink", 23: "misalign", 25: "aligned", 27: "extra C", 28: "C back"})
        if dtype == torch.bfloat16:
            plan.update({15: "to f32", 17: "dtype back"})
        if four:
            plan.update({19: "flip layout", 21: "layout back"})
    elif act.startswith("gelu"):
        plan.update({11: "flip approximate", 13: "approximate back"})
    full_at = {0, 1, 2} | set(plan) | ({24} if "misalign" in plan.values() else set())
    fast_at = {4, 5} | {s + 1 for s in plan if s + 1 not in full_at}
    xshape, training = shape, True
    log = {}
    for step in range(30):
        what = plan.get(step)
        if what == "x shape":
            xshape = shape2
        elif what == "eval":
            tw.a.eval(), tw.b.eval()
            training = False
        elif what == "train":
            tw.a.train(), tw.b.train()
            training = True
        elif what in ("grow", "shrink"):
            shaper(rep=2 if what == "grow" else 1)
        elif what in ("to f32", "dtype back"):
            shaper(to_f32=what == "to f32")
        elif what in ("flip layout", "layout back"):
            shaper(flip_layout=what == "flip layout")
        elif what in ("misalign", "aligned"):
            shaper(misalign=what == "misalign")
        elif what in ("extra C", "C back"):
            shaper(extra_c=2 if what == "extra C" else 0)
        elif what in ("flip approximate", "approximate back"):
            for m in acts:
                m.approximate = {"none": "tanh", "tanh": "none"}[m.approximate]
        x, gr = data(step, xshape, dtype, cl, cd)
        tag = (act, layout, kind, step, what)
        outs, fast = tw.step(x, gr, 4000 + step, calls)
        log[step] = fast
        compare(tw, outs, tag)
        if oracle is not None:
            assert tw.h is not None, tag
            oracle.step(tw.h, training, outs[1][0], tw.b, tag)
    for s in sorted(full_at):
        assert log[s] == 0, ("full path expected", s, plan.get(s), log)
    for s in sorted(fast_at):
        assert log[s] == 1, ("fast path expected", s, plan.get(s), log)
    assert plan_guard.checked["site_fwd"] >= 20, plan_guard.checked


def test_fast_path_under_autocast_follows_the_autocast_state(monkeypatch, plan_guard):
    """fp32 x under torch.autocast: the identity fold (the site writes the bf16 image) is chosen per autocast state"""
    tw = Twins(monkeypatch, ACTS["gelu"], "scaler", 1)
    calls = counted(tw.a[0][0], tw.b[0][0])
    log = {}
    for step in range(16):
        on = step not in (8, 9)
        x, gr = data(step, (6, 16, 8, 8), torch.float32, False, 1)
        with torch.autocast("cuda", torch.bfloat16, enabled=on):
            outs, log[step] = tw.step(x, gr, 5000 + step, calls)
        compare(tw, outs, ("autocast", step))
    assert [log[s] for s in (4, 5, 6, 7, 8, 9, 10, 11, 15)] == [1, 1, 1, 1, 0, 1, 0, 1, 1], log


# ------------------------------------------------------------------------------------------------------------------------------------
# one evaluation of the GELU per forward on every route, `act_rider` rejecting the h it computed included
# ------------------------------------------------------------------------------------------------------------------------------------
class GeluSpy:
    """counts torch.nn.functional.gelu (what nn.GELU.forward calls); `cl`: its output comes back channels_last, a layout unlike
    x's, which `act_rider` rejects"""

    def __init__(self, monkeypatch):
        self.calls, self.cl = 0, False
        self.real = real = F.gelu

        def gelu(x, approximate="none"):
            self.calls += 1
            h = real(x, approximate=approximate)
            return h.contiguous(memory_format=torch.channels_last) if (self.cl and h.dim() == 4) else h

        monkeypatch.setattr(F, "gelu", gelu)

    def once(self, m, x):
        c = self.calls
        y = m(x)
        assert self.calls - c == 1, ("GELU evaluations in one forward", self.calls - c)
        return y


def plain(act, q, p=None):
    """the module-by-module route (a plain `nn.Sequential`: the GELU is an autograd node of its own; no option is changed, which
    would send the pair under test through its full path)"""
    return (nn.Sequential(nn.Sequential(act, p), q) if p is not None else nn.Sequential(act, q)).to(DEV).train()


def _plain(m, x, gr):
    xd = x.clone().requires_grad_(True)
    y = m(xd)
    return y.detach().cpu(), torch.autograd.grad(y, xd, gr.to(y.dtype))[0].cpu()


@pytest.mark.parametrize("rejected", [False, True])
def test_gelu_runs_once_per_forward_on_every_route(rejected, monkeypatch, plan_guard):
    spy = GeluSpy(monkeypatch)
    spy.cl = rejected
    tw = Twins(monkeypatch, ACTS["gelu"], "scaler", 1)
    pq = make(nn.GELU(), "scaler", 1)
    ref = plain(pq[0][0], pq[1], pq[0][1])
    assert type(ref) is nn.Sequential and type(ref[0]) is nn.Sequential
    log = {}
    for step in range(14):
        if step in (9, 11):              # fast-path misses after the GELU ran (erf <-> tanh: another h signature)
            for m in (tw.a[0][0], tw.b[0][0], ref[0][0]):
                m.approximate = {"none": "tanh", "tanh": "none"}[m.approximate]
        x, gr = data(step, (6, 16, 8, 8), torch.bfloat16, False, 1)
        n = spy.calls
        outs, log[step] = tw.step(x, gr, 6000 + step, lambda: spy.calls)
        assert spy.calls - n == 2, ("GELU evaluations of the two forwards", step, spy.calls - n)
        compare(tw, outs, ("gelu once", rejected, step))
        y_ref, g_ref = _plain(ref, x, gr)
        assert same(outs[0][0], y_ref) and same(outs[0][1], g_ref), ("vs the module-by-module route", rejected, step)
    # (a rejected h enters the graph through `_ActGrad`: the same signature as the tanh form's autograd output -- no miss then)
    assert all(log[s] == 1 for s in (4, 5, 6, 7, 8, 10, 12, 13)) and log[9] == log[11] == int(rejected), log


def test_a_gelu_output_aten_lays_out_unlike_x_is_evaluated_once(monkeypatch):
    """a dense x whose extent-1 dim has an unusual stride (a permuted batch of one): ATen's GELU returns the contiguous layout,
    `act_rider` rejects it, and both sites -- the pair and the quantize-only site -- put that very h into the graph"""
    spy = GeluSpy(monkeypatch)
    pair, pq = make(nn.GELU(), "scaler", 1), make(nn.GELU(), "scaler", 1)
    pair_ref = plain(pq[0][0], pq[1], pq[0][1])
    aq = fuse_prune_quantize_pairs(nn.Sequential(nn.Sequential(nn.GELU(), qs.quantize(bits=4, timeout=1, channelwise=-1))))[0].to(DEV).train()
    aq_ref = plain(nn.GELU(), qs.quantize(bits=4, timeout=1, channelwise=-1))
    assert type(aq) is fused.FusedActQuantize and type(aq_ref) is nn.Sequential
    for step in range(6):
        g = torch.Generator().manual_seed(700 + step)
        x = (torch.randn(16, 8, 8, 1, generator=g) * 2).to(torch.bfloat16).to(DEV).permute(3, 0, 1, 2)
        gr = torch.randn(1, 16, 8, 8, generator=g).to(DEV)
        assert x.stride() == (1, 64, 8, 1) and spy.real(x).stride() != x.stride()     # (what `act_rider` rejects)
        for m, m_ref in ((pair, pair_ref), (aq, aq_ref)):
            xd = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
            assert xd.stride() == x.stride()
            y = spy.once(m, xd)
            (gx,) = torch.autograd.grad(y, xd, gr.to(y.dtype))
            y_ref, g_ref = _plain(m_ref, x, gr)
            assert same(y.detach().cpu(), y_ref) and same(gx.cpu(), g_ref), ("vs the module-by-module route", m is aq, step)
