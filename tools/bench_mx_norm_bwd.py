#!/usr/bin/env python
"""mx_norm_backward (qs_mx_norm_bwd_v) against what it replaces and against ATen, and the MXTrainNormLinear step with
norm_backward="fused" against "torch" and against norm module -> MXTrainLinear.

Kernel level, all three outputs, float32 dxhat: the torch chain of mx_norm.py (_norm_xhat + _norm_backward + the cast of dx) and ATen's
own norm backward (F.rms_norm / F.layer_norm under autograd, the forward outside the timed window; its incoming gradient has x's dtype,
so for a bfloat16 x it reads half the gradient bytes).  The fraction of 8 TB/s is for the algorithmic bytes: one read of dxhat and x,
one write of dx.
HIP events around `--iters` calls, the median of three such runs after a warm-up, the spread (max - min of the three) recorded; every
comparator in the same process.  Writes profiles/mx_norm_bwd.json.  The bar per comparison: faster than the comparator by more than
the comparator's own spread."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import qsparse_amd as qs  # noqa: E402
from qsparse_amd.mx_norm import _norm_backward, _norm_xhat  # noqa: E402

SHAPES = ((8192, 4096), (50432, 768))
STEPS = ((8192, 4096, 4096), (50432, 768, 3072))
PEAK = 8.0e12


def timed(fn, iters, warmup=5):
    """(median, spread) in microseconds per call over three runs of `iters` calls"""
    for _ in range(warmup):
        fn()
    runs = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        runs.append(a.elapsed_time(b) * 1e3 / iters)
    runs.sort()
    return runs[1], runs[2] - runs[0]


def versus(rec, name, fused_us, fn, iters):
    us, spread = timed(fn, iters)
    rec[f"{name}_us"], rec[f"{name}_spread_us"] = round(us, 2), round(spread, 2)
    rec[f"ratio_to_{name}"] = round(us / fused_us, 3)
    rec[f"beats_{name}"] = bool(us - fused_us > spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_norm_bwd.json"))
    args = ap.parse_args()
    dev = "cuda:0"
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    torch.manual_seed(0)
    kernels, steps = [], []
    for R, C in SHAPES:
        w, b = (torch.rand(C, device=dev) + 0.5), torch.randn(C, device=dev)
        dxhat = torch.randn(R, C, device=dev)
        for dtype in (torch.bfloat16, torch.float32):
            x = (torch.randn(R, C, device=dev) * 3 + 0.5).to(dtype)
            for norm in ("rms", "layer"):
                rstd, mean = qs.mx_norm_quantize(x, w, b if norm == "layer" else None, norm=norm, return_stats=True)[-2:]
                rec = dict(case=f"{norm} [{R}, {C}] x {str(dtype)[6:]}, dxhat float32")
                fu, fs = timed(lambda: qs.mx_norm_backward(dxhat, x, rstd, mean, w, norm=norm), args.iters)
                nbytes = dxhat.numel() * 4 + 2 * x.numel() * x.element_size()
                rec.update(fused_us=round(fu, 2), fused_spread_us=round(fs, 2), algorithmic_bytes=nbytes,
                           fraction_of_8TBps=round(nbytes / (fu * 1e-6) / PEAK, 3))

                def chain():
                    dx, dw, db = _norm_backward(dxhat, _norm_xhat(x, rstd, mean), rstd, w, norm)
                    return dx.to(dtype), dw, db

                versus(rec, "torch_chain", fu, chain, args.iters)
                xa = x.clone().requires_grad_(True)
                wa, ba = w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
                ga = dxhat.to(dtype)
                if norm == "rms":
                    ya, leaves = F.rms_norm(xa, (C,), wa, 1e-6), (xa, wa)
                else:
                    ya, leaves = F.layer_norm(xa, (C,), wa, ba, 1e-6), (xa, wa, ba)
                versus(rec, "aten", fu, lambda: torch.autograd.grad(ya, leaves, ga, retain_graph=True), args.iters)
                del ya, xa
                print(json.dumps(rec), flush=True)
                kernels.append(rec)
    del dxhat, x
    # the training step: forward + backward, bfloat16 activations and parameters
    for R, K, N in STEPS:
        x = torch.randn(R, K, device=dev, dtype=torch.bfloat16, requires_grad=True)
        dy = torch.randn(R, N, device=dev, dtype=torch.bfloat16)
        for norm in ("rms", "layer"):
            fn = (nn.RMSNorm(K, eps=1e-6) if norm == "rms" else nn.LayerNorm(K, eps=1e-6)).to(dev).to(torch.bfloat16)
            lin = nn.Linear(K, N).to(dev).to(torch.bfloat16)
            fused = qs.MXTrainNormLinear.from_float(fn, lin, norm_backward="fused")
            plain = qs.MXTrainNormLinear.from_float(fn, lin)
            comp = nn.Sequential(fn, qs.MXTrainLinear.from_linear(lin))

            def step(m):
                x.grad = None
                for p in m.parameters():
                    p.grad = None
                m(x).backward(dy)

            iters = max(2, args.iters // 4)
            rec = dict(case=f"train step {norm} [{R}, {K}] -> {N} bf16")
            fu, fs = timed(lambda: step(fused), iters)
            rec.update(fused_us=round(fu, 2), fused_spread_us=round(fs, 2))
            versus(rec, "torch_backward", fu, lambda: step(plain), iters)
            versus(rec, "norm_then_linear", fu, lambda: step(comp), iters)
            print(json.dumps(rec), flush=True)
            steps.append(rec)
    doc = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters,
               method="HIP events around `iters` calls (a quarter of them for a step); median of three runs after 5 warm-up calls; "
                      "spread = max - min of the three; every comparator in the same process",
               bar="comparator_us - fused_us > comparator_spread_us", kernels=kernels, steps=steps,
               kernel_beats_torch_chain_everywhere=all(r["beats_torch_chain"] for r in kernels),
               fused_step_beats_torch_backward_everywhere=all(r["beats_torch_backward"] for r in steps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
