#!/usr/bin/env python3
"""Time of `mx_matmul` (the block-scaled MFMA kernel on MX codes) next to what an MX layer costs without it.

    python3 tools/bench_mx_gemm.py [--out profiles/mx_gemm.json] [--iters 50] [--warmup 10] [--small]
    python3 tools/bench_mx_gemm.py --errors [--out profiles/mx_gemm_error.json]
    python3 tools/bench_mx_gemm.py --splitk [--out profiles/mx_splitk_gemm.json]

One process.  Per case and operation: `warmup` launches, then HIP events around `iters` back-to-back launches, three times, the
median kept (all three recorded).  Shapes: [50432, 768] x [3072, 768] and [50432, 3072] x [768, 3072] (the ViT-B MLP of bench.py's
token-major configuration) and 4096^3; formats FP8 E4M3 x FP8 E4M3, FP8 E4M3 x FP4, FP4 x FP4; float32 and bf16 output.  On the
same values, in the same process:
  (a) F.linear on the float32 de-quantized tensors -- what an MX layer costs today; THE BAR: mx_matmul alone no slower than (a),
      judged against the spread of (a)'s own three repetitions
  (b) F.linear on their bf16 images -- for orientation, no target
and the end-to-end figure quantize_with_mx(x) + mx_matmul (bf16 activations in).  `--errors`: the largest |y - y64| / S per format
pair (S = sum_k |a_k b_k|, float64 on the CPU) on quantizer-produced inputs, K = 4096 -- the slack under the tests' bound
2 K 2^-23.  `--splitk`: the three products of a linear layer's step on the same three layer shapes, in the formats and output
dtypes `mx_linear` uses (forward E4M3 x E4M3 and dgrad E5M2 x E4M3 to bf16, wgrad E5M2 x E4M3 to float32): each unsplit, and the
weight-gradient products also through `mx_matmul(..., split_k=S)` for S = "auto", 2, 3, 4, 6, 8 -- both launches of the split call
inside the timed window.  On a commit without split-K the tool finds no split call and times the unsplit products alone: that run is
the yardstick (THE BARS: the split call at the automatic S no slower than the yardstick's unsplit weight-gradient product; the unsplit
products no slower than the yardstick's by more than the larger of its repeat-to-repeat spread and 2 %).  Needs a GPU: there is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMATS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp8_e4m3", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp4_e2m1")]


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
    return statistics.median(reps), reps


def bench(args):
    import torch
    import torch.nn.functional as F
    from qsparse_amd import _hip
    from qsparse_amd.mx_gemm import mx_matmul
    from qsparse_amd.quantize import mx_dequantize, quantize_with_mx
    dev = "cuda:0"
    shapes = [(50432, 3072, 768), (50432, 768, 3072), (4096, 4096, 4096)] if not args.small else [(512, 384, 256), (256, 256, 512)]
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    for M, N, K in shapes:
        x = torch.randn(M, K, device=dev, generator=g, dtype=torch.bfloat16)
        w = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
        flop = 2.0 * M * N * K
        for fa, fb in FORMATS:
            _, ac, asc = quantize_with_mx(x, fa, -1, return_codes=True)
            _, bc, bsc = quantize_with_mx(w, fb, -1, return_codes=True)
            a32, b32 = mx_dequantize(ac, asc, fa), mx_dequantize(bc, bsc, fb)
            a16, b16 = a32.bfloat16(), b32.bfloat16()
            rec = {"M": M, "N": N, "K": K, "a_fmt": fa, "b_fmt": fb}
            ms_a, reps_a = timed(lambda: F.linear(a32, b32), args.iters, args.warmup)
            ms_b, reps_b = timed(lambda: F.linear(a16, b16), args.iters, args.warmup)
            rec["linear_f32"] = {"ms": ms_a, "reps_ms": reps_a, "tflops": flop / ms_a * 1e-9}
            rec["linear_bf16"] = {"ms": ms_b, "reps_ms": reps_b, "tflops": flop / ms_b * 1e-9}
            del a32, b32, a16, b16
            for dt in (torch.float32, torch.bfloat16):
                ms, reps = timed(lambda: mx_matmul(ac, asc, fa, bc, bsc, fb, None, dt), args.iters, args.warmup)
                assert _hip.mx_gemm_last_route == _hip.MX_GEMM_ROUTE_VEC

                def both():
                    _, c, s = quantize_with_mx(x, fa, -1, return_codes=True)
                    return mx_matmul(c, s, fa, bc, bsc, fb, None, dt)

                ms_e2e, reps_e2e = timed(both, args.iters, args.warmup)
                rec["mx_matmul_" + str(dt).split(".")[1]] = {
                    "ms": ms, "reps_ms": reps, "tflops": flop / ms * 1e-9, "ratio_to_linear_f32": ms / ms_a, "ratio_to_linear_bf16": ms / ms_b,
                    "no_slower_than_linear_f32": bool(ms <= max(reps_a)),
                    "with_quantize_ms": ms_e2e, "with_quantize_reps_ms": reps_e2e, "with_quantize_ratio_to_linear_f32": ms_e2e / ms_a}
            out["cases"].append(rec)
            print(json.dumps(rec), flush=True)
            with open(args.out, "w") as f:          # (kept current after every case)
                json.dump(out, f, indent=1)
                f.write("\n")
    print("wrote", args.out)


def splitk(args):
    import torch
    from qsparse_amd import _hip
    from qsparse_amd.mx_gemm import mx_matmul
    from qsparse_amd.quantize import quantize_with_mx
    dev = "cuda:0"
    layers = [(50432, 3072, 768), (50432, 768, 3072), (4096, 4096, 4096)] if not args.small else [(4224, 384, 256), (256, 256, 512)]
    has_split = hasattr(_hip, "mx_split_plan")
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup,
           "split_k_available": has_split, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    e4, e5 = "mxfp8_e4m3", "mxfp8_e5m2"
    for Ml, Nl, Kl in layers:
        # product, (rows of A, rows of B, contraction), formats, output dtype
        for name, (M, N, K), fa, fb, dt in (("forward", (Ml, Nl, Kl), e4, e4, torch.bfloat16), ("dgrad", (Ml, Kl, Nl), e5, e4, torch.bfloat16),
                                            ("wgrad", (Nl, Kl, Ml), e5, e4, torch.float32)):
            _, ac, asc = quantize_with_mx(torch.randn(M, K, device=dev, generator=g, dtype=torch.bfloat16), fa, -1, return_codes=True)
            _, bc, bsc = quantize_with_mx(torch.randn(N, K, device=dev, generator=g, dtype=torch.bfloat16), fb, -1, return_codes=True)
            flop = 2.0 * M * N * K
            rec = {"layer": [Ml, Nl, Kl], "product": name, "M": M, "N": N, "K": K, "a_fmt": fa, "b_fmt": fb, "out": str(dt).split(".")[1]}
            ms, reps = timed(lambda: mx_matmul(ac, asc, fa, bc, bsc, fb, None, dt), args.iters, args.warmup)
            assert _hip.mx_gemm_last_route == _hip.MX_GEMM_ROUTE_VEC
            rec["unsplit"] = {"ms": ms, "reps_ms": reps, "tflops": flop / ms * 1e-9, "spread": (max(reps) - min(reps)) / ms}
            if has_split:
                rec["auto_slices"] = _hip.mx_split_plan(M, N, K, 0)[0]
                if name == "wgrad":
                    y1 = mx_matmul(ac, asc, fa, bc, bsc, fb, None, dt)
                    for S in ("auto", 2, 3, 4, 6, 8):
                        y = mx_matmul(ac, asc, fa, bc, bsc, fb, None, dt, split_k=S)
                        slices = _hip.mx_gemm_last_split
                        err = float((y - y1).abs().max() / y1.abs().max())          # summation order only: a few float32 ulps
                        ms_s, reps_s = timed(lambda: mx_matmul(ac, asc, fa, bc, bsc, fb, None, dt, split_k=S), args.iters, args.warmup)
                        rec[f"split_{S}"] = {"slices": slices, "ms": ms_s, "reps_ms": reps_s, "tflops": flop / ms_s * 1e-9,
                                             "ratio_to_unsplit": ms_s / ms, "max_abs_diff_over_max_abs": err}
            out["cases"].append(rec)
            print(json.dumps(rec), flush=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
            del ac, asc, bc, bsc
    print("wrote", args.out)


def errors(args):
    import torch
    from qsparse_amd.mx_gemm import mx_matmul
    from qsparse_amd.quantize import MX_FORMATS, mx_dequantize, quantize_with_mx
    dev = "cuda:0"
    M, N, K = 256, 256, 4096
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "M": M, "N": N, "K": K, "bound_over_S": 2 * K * 2.0 ** -23, "pairs": {}}
    for fa in MX_FORMATS:
        for fb in MX_FORMATS:
            _, ac, asc = quantize_with_mx(x.to(dev), fa, -1, return_codes=True)
            _, bc, bsc = quantize_with_mx(w.to(dev), fb, -1, return_codes=True)
            y = mx_matmul(ac, asc, fa, bc, bsc, fb).cpu().double()
            a, b = mx_dequantize(ac.cpu(), asc.cpu(), fa, -1, torch.float64), mx_dequantize(bc.cpu(), bsc.cpu(), fb, -1, torch.float64)
            y64, S = a @ b.t(), a.abs() @ b.abs().t()
            out["pairs"][f"{fa} x {fb}"] = {"max_err_over_S": float(((y - y64).abs() / S).max())}
            print(fa, fb, out["pairs"][f"{fa} x {fb}"], flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--splitk", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit the figures were measured on")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_gemm.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_gemm_error.json" if args.errors else "mx_splitk_gemm.json" if args.splitk else "mx_gemm.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    (errors if args.errors else splitk if args.splitk else bench)(args)


if __name__ == "__main__":
    main()
