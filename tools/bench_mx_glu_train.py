#!/usr/bin/env python3
"""Time of the training half of the gated MX products next to the ways to get the same results without it.

    python3 tools/bench_mx_glu_train.py [--out profiles/mx_glu_train.json] [--iters 20] [--warmup 5] [--small] [--comparators-only]

One process.  Per case and operation: `warmup` calls, then HIP events around `iters` back-to-back calls, three times, the median kept
(all three recorded, and their spread).
  (a) the backward quantizer `mx_glu_backward_quantize` (E5M2 pairs, act silu; bf16 dh with float32 and with bf16 v) at T = 8192, H =
      11008 and at T = 8192, H = 4096, against the composition: dv in float32 by elementary torch ops, then `mx_quantize_2way`.  Also
      the bytes the fused call moves (dh, v, the four outputs, once each) over its time.
  (b) the forward that keeps v, `mx_glu_matmul(..., preact_dtype)` (float h), against `mx_matmul` to the same dtype plus the float
      epilogue (split, silu, multiply) by torch ops.
  (d) a forward + backward of `MXTrainGroupedGLULinear` at T = 8192, K = 1024, H = 4096 with 8 and 64 groups, balanced and skewed,
      against `MXTrainGroupedLinear` at N = 2 H followed by the float GLU under autograd.  A ratio, no bar.
THE BAR of (a) and (b): fused faster than the composition by more than the composition's own spread.  The compositions use only calls
that exist without this module, so `--comparators-only` runs on a checkout without it; it writes profiles/mx_glu_train_parent.json.
Needs a GPU: there is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_gemm import timed  # noqa: E402
from bench_mx_glu import halves, interleave, sizes_of  # noqa: E402

FMT = "mxfp8_e5m2"


def stat(ms, reps, nbytes=None):
    s = {"ms": ms, "reps_ms": reps, "spread_ms": max(reps) - min(reps)}
    if nbytes is not None:
        s["bytes"], s["tb_per_s"] = nbytes, nbytes / ms * 1e-9
    return s


def bench(args):
    import torch
    import torch.nn.functional as F
    from qsparse_amd import MXTrainGroupedLinear, mx_matmul, mx_quantize_2way, quantize_with_mx
    fused = not args.comparators_only
    if fused:
        from qsparse_amd import MXTrainGroupedGLULinear, mx_glu_backward_quantize, mx_glu_matmul
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "act": "silu",
           "fused_measured": fused, "cases": []}

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    def record(rec, fused_call, composition, equal=None, nbytes=None, bar=True):
        if fused:
            if equal is not None:
                assert equal(fused_call(), composition()), "the fused call differs from the composition"
            rec["fused"] = stat(*timed(fused_call, args.iters, args.warmup), nbytes)
        rec["composition"] = stat(*timed(composition, args.iters, args.warmup))
        if fused:
            c, f = rec["composition"], rec["fused"]
            rec["composition_over_fused"] = c["ms"] / f["ms"]
            if bar:
                rec["bar_met"] = bool(c["ms"] - f["ms"] > c["spread_ms"])
        out["cases"].append(rec)
        save()
        print(json.dumps(rec), flush=True)

    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g, dtype=torch.bfloat16)

    def dv_of(dh, v):
        gt, u = halves(v.to(torch.float32))
        d = dh.to(torch.float32)
        s = torch.sigmoid(gt)
        da = s * (1.0 + gt * (1.0 - s))
        dg, du = (d * u) * da, d * F.silu(gt)
        return torch.cat((dg.reshape(dg.shape[0], -1, 1, 32), du.reshape(du.shape[0], -1, 1, 32)), 2).reshape(dg.shape[0], -1)

    all_equal = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    # ---- (a) ----
    for T, H in ([(8192, 11008), (8192, 4096)] if not args.small else [(512, 256)]):
        dh = rnd(T, H)
        for vdt in (torch.float32, torch.bfloat16):
            v = (rnd(T, 2 * H) * 3).to(vdt)
            nbytes = dh.numel() * 2 + v.numel() * v.element_size() + 2 * (T * 2 * H + T * 2 * H // 32)
            record({"case": "a_backward_quantizer", "T": T, "H": H, "dh": "bfloat16", "v": str(vdt).replace("torch.", ""), "fmt": FMT},
                   lambda: mx_glu_backward_quantize(dh, v, act="silu", row_fmt=FMT, col_fmt=FMT),
                   lambda: mx_quantize_2way(dv_of(dh, v), FMT, FMT), all_equal, nbytes)
            del v
        del dh
    # ---- (b) ----
    M, K, H = (8192, 4096, 11008) if not args.small else (512, 256, 256)
    fa = fb = "mxfp8_e4m3"
    x, w = rnd(M, K) * 2, interleave(rnd(H, K), rnd(H, K)) / K ** 0.5
    (ac, asc), (bc, bsc) = quantize_with_mx(x, fa, -1, return_codes=True)[1:], quantize_with_mx(w, fb, -1, return_codes=True)[1:]
    del x, w
    for vdt in (torch.float32, torch.bfloat16):

        def composition():
            v = mx_matmul(ac, asc, fa, bc, bsc, fb, None, vdt)
            gt, u = halves(v.to(torch.float32))
            return (F.silu(gt) * u).to(torch.bfloat16), v

        record({"case": "b_forward_keeps_v", "M": M, "K": K, "H": H, "v": str(vdt).replace("torch.", ""), "h": "bfloat16"},
               lambda: mx_glu_matmul(ac, asc, fa, bc, bsc, fb, None, torch.bfloat16, act="silu", preact_dtype=vdt), composition,
               lambda a, b: torch.equal(a[1], b[1]) and (vdt is not torch.float32 or torch.equal(a[0], b[0])))      # (h from a ROUNDED v differs)
    del ac, asc, bc, bsc
    # ---- (d) ----
    T, K, H = (8192, 1024, 4096) if not args.small else (512, 256, 256)
    x, dh = rnd(T, K) * 2, rnd(T, H)
    for E in (8, 64):
        w = (interleave(rnd(E, H, K), rnd(E, H, K)) / K ** 0.5).to(torch.float32)
        plain = MXTrainGroupedLinear.from_float(w.clone().requires_grad_(True), None, out_dtype=torch.float32)
        gated = MXTrainGroupedGLULinear(w.clone(), None, out_dtype=torch.bfloat16) if fused else None
        for kind in ("balanced", "skewed"):
            offs = torch.tensor(sizes_of(kind, E, T)).cumsum(0).to(torch.int32).to(dev)

            def step_plain():
                xl = x.detach().requires_grad_(True)
                gt, u = halves(plain(xl, offs))
                return torch.autograd.grad((F.silu(gt) * u).to(torch.bfloat16), (xl, plain.weight), dh)

            def step_gated():
                xl = x.detach().requires_grad_(True)
                return torch.autograd.grad(gated(xl, offs), (xl, gated.weight), dh)

            record({"case": "d_grouped_step", "sizes": kind, "T": T, "K": K, "H": H, "E": E}, step_gated, step_plain, bar=False)
        del w, plain, gated
    if fused:
        out["bar_met_everywhere"] = all(c["bar_met"] for c in out["cases"] if "bar_met" in c)
    save()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--comparators-only", action="store_true")
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mx_glu_train_parent.json" if args.comparators_only else "mx_glu_train.json")
    bench(args)
