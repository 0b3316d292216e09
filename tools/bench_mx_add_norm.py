#!/usr/bin/env python
"""The residual add fused into the MX norm quantizer and into its backward, against the compositions they replace.

Forward:  mx_add_norm_quantize(x, residual)              against  torch.add(residual, x) + mx_norm_quantize(h)
Backward: mx_norm_backward(..., dresidual=dh_in)         against  mx_norm_backward(...) + torch.add(dx, dh_in)   (float32 dxhat)
Step:     MXTrainAddNormLinear(x, residual) -> (y, h)    against  h = residual + x; MXTrainNormLinear(norm_backward="fused")(h)
          with a loss that uses y and h, so the stream's gradient reaches h in both.

Shapes [8192, 4096] and [50432, 768]; bfloat16 and float32; rms and layer; the forward with and without the col pair.  The fused call
and its comparator alternate inside every run (the machine is shared): HIP events around `--iters` calls of each, the median of three
such runs after a warm-up, the spread (max - min of the three) recorded.  The fraction of 8 TB/s is for the algorithmic bytes of the
fused call.  Writes profiles/mx_add_norm.json.  The bar per comparison: faster than the composition by more than the composition's own
spread."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import qsparse_amd as qs  # noqa: E402

SHAPES = ((8192, 4096), (50432, 768))
STEPS = ((8192, 4096, 4096), (50432, 768, 3072))
PEAK = 8.0e12


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def pair(rec, fused, comp, iters, warmup=5):
    """times `fused` and `comp` in alternating windows of `iters` calls, three of each; microseconds per call: median and spread"""
    for _ in range(warmup):
        fused()
        comp()
    f, c = [], []
    for _ in range(3):
        f.append(_window(fused, iters))
        c.append(_window(comp, iters))
    f.sort()
    c.sort()
    rec.update(fused_us=round(f[1], 2), fused_spread_us=round(f[2] - f[0], 2), composition_us=round(c[1], 2),
               composition_spread_us=round(c[2] - c[0], 2), ratio=round(c[1] / f[1], 3), beats_composition=bool(c[1] - f[1] > c[2] - c[0]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_add_norm.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_add_norm.py measures on the GPU: none found")
    dev = "cuda:0"
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    torch.manual_seed(0)
    forward, backward, steps = [], [], []
    for R, C in SHAPES:
        w, b = (torch.rand(C, device=dev) + 0.5), torch.randn(C, device=dev)
        dxhat = torch.randn(R, C, device=dev)
        for dtype in (torch.bfloat16, torch.float32):
            esz = 2 if dtype == torch.bfloat16 else 4
            x = torch.randn(R, C, device=dev).to(dtype)
            res = (torch.randn(R, C, device=dev) * 3 + 0.5).to(dtype)
            dres = torch.randn(R, C, device=dev).to(dtype)
            for norm in ("rms", "layer"):
                bias = b if norm == "layer" else None
                for col in (None, "mxfp8_e4m3"):
                    kw = dict(norm=norm, fmt="mxfp8_e4m3", col_fmt=col, return_stats=True)
                    rec = dict(case=f"forward {norm} [{R}, {C}] {str(dtype)[6:]}, {'two-way' if col else 'row pair'}")
                    pair(rec, lambda: qs.mx_add_norm_quantize(x, res, w, bias, **kw),
                         lambda: qs.mx_norm_quantize(torch.add(res, x), w, bias, **kw), args.iters)
                    # the fused call: x, residual read, h written, h read by the quantizing launch, the codes written
                    nbytes = R * C * (4 * esz + (2 if col else 1))
                    rec.update(algorithmic_bytes=nbytes, fraction_of_8TBps=round(nbytes / (rec["fused_us"] * 1e-6) / PEAK, 3))
                    print(json.dumps(rec), flush=True)
                    forward.append(rec)
                h = torch.add(res, x)
                rstd, mean = qs.mx_norm_quantize(h, w, bias, norm=norm, return_stats=True)[-2:]
                rec = dict(case=f"backward {norm} [{R}, {C}] x {str(dtype)[6:]}, dxhat float32")

                def composed():
                    dx, dw, db = qs.mx_norm_backward(dxhat, h, rstd, mean, w, norm=norm)
                    return torch.add(dx, dres), dw, db

                pair(rec, lambda: qs.mx_norm_backward(dxhat, h, rstd, mean, w, norm=norm, dresidual=dres), composed, args.iters)
                # dxhat and x read twice (statistics, apply), dresidual read, dx written
                nbytes = R * C * (2 * 4 + 2 * esz + 2 * esz)
                rec.update(algorithmic_bytes=nbytes, fraction_of_8TBps=round(nbytes / (rec["fused_us"] * 1e-6) / PEAK, 3))
                print(json.dumps(rec), flush=True)
                backward.append(rec)
                del h
        del dxhat, x, res, dres
    # the training step: forward + backward, bfloat16 activations and parameters, a loss that uses y and h
    for R, K, N in STEPS:
        x = torch.randn(R, K, device=dev, dtype=torch.bfloat16, requires_grad=True)
        res = torch.randn(R, K, device=dev, dtype=torch.bfloat16, requires_grad=True)
        dy = torch.randn(R, N, device=dev, dtype=torch.bfloat16)
        dh = torch.randn(R, K, device=dev, dtype=torch.bfloat16)
        for norm in ("rms", "layer"):
            fn = (nn.RMSNorm(K, eps=1e-6) if norm == "rms" else nn.LayerNorm(K, eps=1e-6)).to(dev).to(torch.bfloat16)
            lin = nn.Linear(K, N).to(dev).to(torch.bfloat16)
            fused = qs.MXTrainAddNormLinear.from_float(fn, lin)
            plain = qs.MXTrainNormLinear.from_float(fn, lin, norm_backward="fused")

            def step(m, add):
                x.grad = res.grad = None
                for p in m.parameters():
                    p.grad = None
                if add:
                    y, h = m(x, res)
                else:
                    h = res + x
                    y = m(h)
                torch.autograd.backward((y, h), (dy, dh))

            rec = dict(case=f"train step {norm} [{R}, {K}] -> {N} bf16")
            pair(rec, lambda: step(fused, True), lambda: step(plain, False), max(2, args.iters // 4))
            print(json.dumps(rec), flush=True)
            steps.append(rec)
    doc = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters,
               method="HIP events around `iters` calls (a quarter of them for a step); the fused call and the composition alternate, "
                      "three windows each after 5 warm-up calls; median and spread (max - min) of the three",
               bar="composition_us - fused_us > composition_spread_us", forward=forward, backward=backward, steps=steps,
               forward_beats_composition_everywhere=all(r["beats_composition"] for r in forward),
               backward_beats_composition_everywhere=all(r["beats_composition"] for r in backward),
               step_beats_composition_everywhere=all(r["beats_composition"] for r in steps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
