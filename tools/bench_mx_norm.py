#!/usr/bin/env python
"""mx_norm_quantize against the composition a user wrote before it -- F.rms_norm / F.layer_norm, then quantize_with_mx(...,
return_codes=True) (one-way) or mx_quantize_2way (two-way) -- and the MXTrainNormLinear step against norm module -> MXTrainLinear.
HIP events around `--iters` calls, the median of three such runs after a warm-up, the spread (max - min of the three) recorded.
Writes profiles/mx_norm.json.  The bar per case: fused faster than the composition by more than the composition's own spread."""
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

FMT = "mxfp8_e4m3"
SHAPES = ((8192, 4096), (50432, 768))


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


def case(name, fused, comp, iters):
    fu, fs = timed(fused, iters)
    cu, cs = timed(comp, iters)
    rec = dict(case=name, fused_us=round(fu, 2), fused_spread_us=round(fs, 2), composition_us=round(cu, 2),
               composition_spread_us=round(cs, 2), ratio=round(cu / fu, 3), meets_bar=bool(cu - fu > cs))
    print(json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_norm.json"))
    args = ap.parse_args()
    dev = "cuda:0"
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    torch.manual_seed(0)
    out = []
    for R, C in SHAPES:
        w, b = (torch.rand(C, device=dev) + 0.5), torch.randn(C, device=dev)
        for dtype in (torch.bfloat16, torch.float32):
            x = torch.randn(R, C, device=dev).to(dtype)
            wd, bd = w.to(dtype), b.to(dtype)
            for norm in ("rms", "layer"):
                fnorm = (lambda: F.rms_norm(x, (C,), wd, 1e-6)) if norm == "rms" else (lambda: F.layer_norm(x, (C,), wd, bd, 1e-6))
                bias = None if norm == "rms" else b
                for two in (False, True):
                    name = f"{norm} [{R}, {C}] {str(dtype)[6:]} {'two-way' if two else 'one-way'}"
                    if two:
                        out.append(case(name, lambda: qs.mx_norm_quantize(x, w, bias, norm=norm, fmt=FMT, col_fmt=FMT),
                                        lambda: qs.mx_quantize_2way(fnorm(), FMT, FMT), args.iters))
                    else:
                        out.append(case(name, lambda: qs.mx_norm_quantize(x, w, bias, norm=norm, fmt=FMT),
                                        lambda: qs.quantize_with_mx(fnorm(), FMT, -1, return_codes=True), args.iters))
    # the training step: forward + backward, [8192, 4096] -> 4096, bf16 activations and float32 parameters under autocast
    R, K, N = 8192, 4096, 4096
    x = torch.randn(R, K, device=dev, dtype=torch.bfloat16, requires_grad=True)
    dy = torch.randn(R, N, device=dev, dtype=torch.bfloat16)
    for norm in ("rms", "layer"):
        fn = (nn.RMSNorm(K, eps=1e-6) if norm == "rms" else nn.LayerNorm(K, eps=1e-6)).to(dev).to(torch.bfloat16)
        lin = nn.Linear(K, N).to(dev).to(torch.bfloat16)
        fused, comp = qs.MXTrainNormLinear.from_float(fn, lin), nn.Sequential(fn, qs.MXTrainLinear.from_linear(lin))

        def step(m):
            x.grad = None
            for p in m.parameters():
                p.grad = None
            m(x).backward(dy)

        out.append(case(f"train step {norm} [{R}, {K}] -> {N} bf16", lambda: step(fused), lambda: step(comp), max(2, args.iters // 4)))
    doc = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters, fmt=FMT,
               method="HIP events around `iters` calls; median of three runs after 5 warm-up calls; spread = max - min of the three",
               bar="composition_us - fused_us > composition_spread_us", cases=out,
               all_meet_bar=all(r["meets_bar"] for r in out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
