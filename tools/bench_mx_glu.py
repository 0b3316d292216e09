#!/usr/bin/env python3
"""Time of the gated products `mx_glu_matmul` / `mx_grouped_glu_matmul` with codes output (the hidden layer of a SwiGLU MLP handed to the
next product as MX codes, one launch) next to the ways to get the same bytes without them.

    python3 tools/bench_mx_glu.py [--out profiles/mx_glu.json] [--iters 20] [--warmup 5] [--small] [--comparators-only]

One process.  Per case and operation: `warmup` calls, then HIP events around `iters` back-to-back calls, three times, the median kept
(all three recorded, and their spread).  Cases: dense M = 8192, K = 4096, H = 11008; grouped T = 8192, K = 1024, H = 4096 at E = 8 and
E = 64, balanced and skewed (half the tokens in one group).  Formats FP8 E4M3 x FP8 E4M3 and FP4 x FP4, output FP8 E4M3, act silu.
  fused  `mx_glu_matmul` / `mx_grouped_glu_matmul` with `out_fmt`
  (a)    the composition the fused call is defined as: `mx_matmul` / `mx_grouped_matmul` to float32 on the interleaved weight, the
         split of the last axis, `F.silu(g) * u`, `quantize_with_mx`.  THE BAR: fused faster than (a) by more than (a)'s spread
  (b)    `mx_matmul` / `mx_grouped_matmul` with `out_fmt` and `act="relu"` at N = 2 H on the same operands: the same products behind the
         ungated quantizing epilogue, which writes twice the codes -- a floor for the loop, not a competitor
(a) and (b) use only calls that exist without the gated products (the interleave is spelled out here), so `--comparators-only` runs
on a checkout without them; it writes profiles/mx_glu_parent.json.  Needs a GPU: there is no fallback.  `--small` shrinks the shapes
for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_gemm import timed  # noqa: E402

FORMATS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1")]
OUT_FMT = "mxfp8_e4m3"


def interleave(gate, up):
    """[..., H, K] twice -> [..., 2 H, K] in runs of 32 rows: gate rows, then up rows"""
    *lead, H, K = gate.shape
    import torch
    return torch.cat((gate.reshape(*lead, H // 32, 1, 32, K), up.reshape(*lead, H // 32, 1, 32, K)), -3).reshape(*lead, 2 * H, K)


def halves(v):
    """[rows, 2 H] -> the gate and up columns [rows, H]"""
    c = v.reshape(v.shape[0], -1, 2, 32)
    return c[:, :, 0].reshape(v.shape[0], -1), c[:, :, 1].reshape(v.shape[0], -1)


def sizes_of(kind, E, T):
    if kind == "balanced":
        return [T // E] * (E - 1) + [T - T // E * (E - 1)]
    rest = (T - T // 2) // (E - 1)              # skewed: half the rows in group 0
    return [T // 2] + [rest] * (E - 2) + [T - T // 2 - rest * (E - 2)]


def stat(ms, reps, flop):
    return {"ms": ms, "reps_ms": reps, "tflops": flop / ms * 1e-9, "spread_ms": max(reps) - min(reps)}


def bench(args):
    import torch
    import torch.nn.functional as F
    from qsparse_amd import mx_grouped_matmul, mx_matmul, quantize_with_mx
    fused = not args.comparators_only
    if fused:
        from qsparse_amd import mx_glu_matmul, mx_grouped_glu_matmul
    dev = "cuda:0"
    dense = (8192, 4096, 11008) if not args.small else (512, 256, 256)
    T, K, H = (8192, 1024, 4096) if not args.small else (512, 256, 256)
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "act": "silu",
           "out_fmt": OUT_FMT, "fused_measured": fused, "cases": []}

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    def epilogue(v):
        g, u = halves(v)
        return quantize_with_mx(F.silu(g) * u, OUT_FMT, -1, return_codes=True)[1:]

    def record(rec, flop, fused_call, composition, floor):
        if fused:
            got, want = fused_call(), composition()
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "the fused call differs from the composition"
            rec["fused"] = stat(*timed(fused_call, args.iters, args.warmup), flop)
        rec["a_composition"] = stat(*timed(composition, args.iters, args.warmup), flop)
        rec["b_relu_codes_2H"] = stat(*timed(floor, args.iters, args.warmup), flop)
        if fused:
            a, b, f = rec["a_composition"], rec["b_relu_codes_2H"], rec["fused"]
            rec["a_over_fused"], rec["fused_over_b"] = a["ms"] / f["ms"], f["ms"] / b["ms"]
            rec["bar_met"] = bool(a["ms"] - f["ms"] > a["spread_ms"])
        out["cases"].append(rec)
        save()
        print(json.dumps(rec), flush=True)

    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g, dtype=torch.bfloat16)
    M, DK, DH = dense
    x, w = rnd(M, DK) * 2, interleave(rnd(DH, DK), rnd(DH, DK)) / DK ** 0.5
    for fa, fb in FORMATS:
        (ac, asc), (bc, bsc) = quantize_with_mx(x, fa, -1, return_codes=True)[1:], quantize_with_mx(w, fb, -1, return_codes=True)[1:]
        record({"case": "dense", "M": M, "K": DK, "H": DH, "a_fmt": fa, "b_fmt": fb}, 2.0 * M * 2 * DH * DK,
               lambda: mx_glu_matmul(ac, asc, fa, bc, bsc, fb, act="silu", out_fmt=OUT_FMT),
               lambda: epilogue(mx_matmul(ac, asc, fa, bc, bsc, fb)),
               lambda: mx_matmul(ac, asc, fa, bc, bsc, fb, out_fmt=OUT_FMT, act="relu"))
    del x, w
    x = rnd(T, K) * 2
    for E in (8, 64):
        w = interleave(rnd(E, H, K), rnd(E, H, K)) / K ** 0.5
        for kind in ("balanced", "skewed"):
            sizes = sizes_of(kind, E, T)
            assert sum(sizes) == T and min(sizes) >= 0
            offs = torch.tensor(sizes).cumsum(0).to(torch.int32).to(dev)
            for fa, fb in FORMATS:
                (ac, asc), (bc, bsc) = quantize_with_mx(x, fa, -1, return_codes=True)[1:], quantize_with_mx(w, fb, -1, return_codes=True)[1:]
                record({"case": "grouped", "sizes": kind, "T": T, "K": K, "H": H, "E": E, "a_fmt": fa, "b_fmt": fb}, 2.0 * T * 2 * H * K,
                       lambda: mx_grouped_glu_matmul(ac, asc, fa, bc, bsc, fb, offs, act="silu", out_fmt=OUT_FMT),
                       lambda: epilogue(mx_grouped_matmul(ac, asc, fa, bc, bsc, fb, offs)),
                       lambda: mx_grouped_matmul(ac, asc, fa, bc, bsc, fb, offs, out_fmt=OUT_FMT, act="relu"))
    if fused:
        out["bar_met_everywhere"] = all(c["bar_met"] for c in out["cases"])
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
        args.out = os.path.join(ROOT, "profiles", "mx_glu_parent.json" if args.comparators_only else "mx_glu.json")
    bench(args)
