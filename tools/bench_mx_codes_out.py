#!/usr/bin/env python3
"""Time of the MX products that write MX codes (`mx_matmul(..., out_fmt=)`, `mx_conv2d(..., out_fmt=)`) next to the composition they
replace: the float32 product followed by `quantize_with_mx(..., return_codes=True)`, with an in-place ReLU between the two where the
fused call applies one.

    python3 tools/bench_mx_codes_out.py [--out run.json] [--iters 50] [--warmup 10] [--small] [--parent-api] [--commit SHA]
    python3 tools/bench_mx_codes_out.py --merge run1.json run2.json --out profiles/mx_codes_out.json
    python3 tools/bench_mx_codes_out.py --compare profiles/mx_codes_out_parent.json profiles/mx_codes_out.json

One process per tree.  Per case and operation: `warmup` launches, then HIP events around `iters` back-to-back launches, three times,
the median kept (all three recorded).  THE BAR, per case: the fused call of this tree takes no longer than the composition ON THE PARENT
COMMIT, by more than the larger of 2 % and the parent's own repeat-to-repeat spread.  `--parent-api` times the composition and the bare
float32 product with nothing but the parent's API (it is also what a tree without `out_fmt` does by itself): copy this file into a
parent checkout and run it there, interleaved with this tree's runs (parent / this / parent / this); `--merge` folds the runs of one
tree into one file (per case the mean of the runs' medians, every repetition kept), `--compare` prints the table and the verdicts.
The fused call against the parent's bare float32 product is recorded without a bar: what the epilogue costs or saves.

Cases: [50432, 768] x [3072, 768], [50432, 3072] x [768, 3072] (the ViT-B MLP of bench.py's token-major configuration) and 4096^3;
the ResNet layers 56 x 56 64 -> 64 3x3, 28 x 28 128 -> 128 3x3 and 56 x 56 256 -> 64 1x1 of tools/bench_mx_conv.py at batch 256; inputs
E4M3 x E4M3 and FP4 x FP4, output E4M3 and FP4, ReLU on and off.  Needs a GPU: there is no fallback.  `--small` shrinks the shapes for
a functional rehearsal (its numbers mean nothing)."""
import argparse
import inspect
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IN_FORMATS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1")]
OUT_FORMATS = ["mxfp8_e4m3", "mxfp4_e2m1"]
GEMMS = [(50432, 3072, 768), (50432, 768, 3072), (4096, 4096, 4096)]
# H (= W), kernel, C, Cout, stride, padding
CONVS = [(56, 3, 64, 64, 1, 1), (28, 3, 128, 128, 1, 1), (56, 1, 256, 64, 1, 0)]
OPS = ("fused", "composition", "float_product")


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    reps = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        reps.append(a.elapsed_time(b) / iters)
    ms = statistics.median(reps)
    return {"ms": ms, "reps_ms": reps, "spread": (max(reps) - min(reps)) / ms}


def bench(args):
    import torch
    from qsparse_amd.mx_conv import mx_conv2d
    from qsparse_amd.mx_gemm import mx_matmul
    from qsparse_amd.quantize import quantize_with_mx
    dev = "cuda:0"
    fused_api = not args.parent_api and "out_fmt" in inspect.signature(mx_matmul).parameters
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup,
           "fused_api": fused_api, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)

    def composition(product, f, relu):
        y = product()
        if relu:
            y.relu_()
        return quantize_with_mx(y, f, -1, return_codes=True)

    def measure(rec, product, fused):
        """`product()`: the float32 call; `fused(f, act)`: the codes-out call"""
        rec["float_product"] = timed(product, args.iters, args.warmup)
        for f in OUT_FORMATS:
            for relu in (False, True):
                case = dict(rec, out_fmt=f, relu=relu)
                case["composition"] = timed(lambda: composition(product, f, relu), args.iters, args.warmup)
                if fused_api:
                    case["fused"] = timed(lambda: fused(f, "relu" if relu else None), args.iters, args.warmup)
                out["cases"].append(case)
                print(json.dumps(case), flush=True)
                with open(args.out, "w") as fh:          # (kept current after every case)
                    json.dump(out, fh, indent=1)
                    fh.write("\n")

    for M, N, K in (GEMMS if not args.small else [(512, 384, 256), (300, 130, 512)]):
        x = torch.randn(M, K, device=dev, generator=g, dtype=torch.bfloat16)
        w = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
        bias = torch.randn(N, device=dev, generator=g)
        for fa, fb in IN_FORMATS:
            _, ac, asc = quantize_with_mx(x, fa, -1, return_codes=True)
            _, bc, bsc = quantize_with_mx(w, fb, -1, return_codes=True)
            measure({"op": "matmul", "M": M, "N": N, "K": K, "a_fmt": fa, "b_fmt": fb},
                    lambda: mx_matmul(ac, asc, fa, bc, bsc, fb, bias),
                    lambda f, act: mx_matmul(ac, asc, fa, bc, bsc, fb, bias, out_fmt=f, act=act))
    B = 8 if args.small else 256
    for H, Kk, C, Cout, stride, padding in CONVS:
        x = torch.randn(B, H, H, C, device=dev, generator=g, dtype=torch.bfloat16)
        w = torch.randn(Cout, Kk, Kk, C, device=dev, generator=g) / (Kk * Kk * C) ** 0.5
        bias = torch.randn(Cout, device=dev, generator=g)
        for fx, fw in IN_FORMATS:
            _, xc, xs = quantize_with_mx(x, fx, -1, return_codes=True)
            _, wc, ws = quantize_with_mx(w, fw, -1, return_codes=True)
            measure({"op": "conv2d", "B": B, "H": H, "W": H, "C": C, "Cout": Cout, "kernel": Kk, "stride": stride, "padding": padding,
                     "a_fmt": fx, "b_fmt": fw},
                    lambda: mx_conv2d(xc, xs, fx, wc, ws, fw, bias, stride, padding),
                    lambda f, act: mx_conv2d(xc, xs, fx, wc, ws, fw, bias, stride, padding, out_fmt=f, act=act))
    print("wrote", args.out)


def _key(case):
    return tuple((k, case[k]) for k in sorted(case) if k not in OPS)


def merge(args):
    runs = [json.load(open(p)) for p in args.merge]
    out = dict(runs[0], runs=len(runs), cases=[])
    for cases in zip(*(r["cases"] for r in runs)):
        assert len({_key(c) for c in cases}) == 1, "the runs do not list the same cases"
        rec = {k: v for k, v in cases[0].items() if k not in OPS}
        for op in OPS:
            if op in cases[0]:
                reps = [r for c in cases for r in c[op]["reps_ms"]]
                ms = statistics.mean(c[op]["ms"] for c in cases)
                rec[op] = {"ms": ms, "reps_ms": reps, "spread": (max(reps) - min(reps)) / ms}
        out["cases"].append(rec)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


def compare(args):
    parent, this = (json.load(open(p)) for p in args.compare)
    theirs = {_key(c): c for c in parent["cases"]}
    print("| case | in | out | ReLU | parent composition ms (spread) | fused ms | fused / composition | bar | parent float32 ms | fused / float32 |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    missed = 0
    for c in this["cases"]:
        p = theirs[_key(c)]
        comp, flt, fused = p["composition"], p["float_product"], c["fused"]
        ok = fused["ms"] <= comp["ms"] * (1 + max(0.02, comp["spread"]))
        missed += not ok
        shape = f"{c['M']} x {c['N']} x {c['K']}" if c["op"] == "matmul" else f"{c['H']}^2 {c['C']}->{c['Cout']} {c['kernel']}x{c['kernel']}"
        fmt = lambda s: s.replace("mxfp8_", "").replace("mxfp4_", "fp4 ").upper()
        print(f"| {shape} | {fmt(c['a_fmt'])} | {fmt(c['out_fmt'])} | {'yes' if c['relu'] else 'no'} | {comp['ms']:.3f} ({100 * comp['spread']:.1f} %) | "
              f"{fused['ms']:.3f} | {fused['ms'] / comp['ms']:.2f} | {'met' if ok else 'MISSED'} | {flt['ms']:.3f} | {fused['ms'] / flt['ms']:.2f} |")
    print(f"{len(this['cases'])} cases, {missed} missed the bar")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent-api", action="store_true", help="time only what the parent commit's API offers: the composition and the float32 product")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit the figures were measured on")
    ap.add_argument("--merge", nargs="+", metavar="RUN", help="fold the runs of one tree into --out")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "THIS"), help="print the table of two merged files")
    args = ap.parse_args()
    if args.compare:
        return compare(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_codes_out_parent.json" if args.parent_api else "mx_codes_out.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.merge:
        return merge(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_codes_out.py measures on the GPU: none found")
    bench(args)


if __name__ == "__main__":
    main()
