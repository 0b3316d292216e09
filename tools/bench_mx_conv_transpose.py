#!/usr/bin/env python3
"""Time of `mx_conv_transpose2d` / `mx_conv2d_input_grad` (the fractionally-strided implicit-GEMM kernel on MX codes) next to what a
transposed convolution of the same values costs without it.

    python3 tools/bench_mx_conv_transpose.py [--out profiles/mx_conv_transpose.json] [--iters 50] [--warmup 10] [--small]

One process.  Per case and operation: `warmup` launches, then HIP events around `iters` back-to-back launches, three times, the
median kept (all three recorded).  Shapes: the mirrors of tools/bench_mx_conv.py's -- for each of its convolutions (batch 256,
channels_last, ResNet-50 body) the transposed convolution that maps the convolution's output back onto its input, which is that
convolution's input gradient: x [B, O, O, Cout] -> y [B, H, H, C] with the weight [C, K, K, Cout] and the output padding the extents
imply; formats FP8 E4M3 x FP8 E4M3, FP8 E4M3 x FP4, FP4 x FP4; float32 and bf16 output.  On the same values, in the same process:
  (a) F.conv_transpose2d on the float32 de-quantized channels_last tensors, with the spread of its own three repetitions
  (b) F.conv_transpose2d on their bf16 images -- no MX semantics, for orientation
No speed bar is set: the ratios to (a) and (b) and (a)'s run-to-run spread are recorded.  A stride s spends s^2 - 1 of every s^2
products of the kernel on zero codes; `useful_tflops` counts the products of the definition only.  Needs a GPU: there is no
fallback.  `--small` shrinks the batch for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMATS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp8_e4m3", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp4_e2m1")]
# of the mirrored convolution: H (= W) of its input, kernel, C, Cout, stride, padding
SHAPES = [(56, 3, 64, 64, 1, 1), (28, 3, 128, 128, 1, 1), (14, 3, 256, 256, 1, 1), (56, 3, 128, 128, 2, 1), (56, 1, 256, 64, 1, 0)]


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
    from qsparse_amd.mx_conv_transpose import mx_conv2d_input_grad, mx_conv_transpose2d
    from qsparse_amd.quantize import mx_dequantize, quantize_with_mx
    dev = "cuda:0"
    B = 8 if args.small else 256
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "batch": B, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    for H, K, Cy, Cx, stride, padding in SHAPES:             # the contraction runs over the convolution's output channels Cx
        O = (H + 2 * padding - K) // stride + 1
        out_pad = H - ((O - 1) * stride - 2 * padding + K)
        x = torch.randn(B, Cx, O, O, device=dev, generator=g, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
        w = torch.randn(Cy, K, K, Cx, device=dev, generator=g) / (K * K * Cx) ** 0.5
        # the products of the definition: every input pixel meets every tap once (those cropped by the padding included: an upper bound)
        flop = 2.0 * B * O * O * Cy * K * K * Cx
        for fx, fw in FORMATS:
            _, xc, xs = quantize_with_mx(x.permute(0, 2, 3, 1), fx, -1, return_codes=True)
            _, wc, ws = quantize_with_mx(w, fw, -1, return_codes=True)
            rec = {"B": B, "H": O, "W": O, "C": Cx, "Cout": Cy, "OH": H, "OW": H, "kernel": K, "stride": stride, "padding": padding,
                   "output_padding": out_pad, "x_fmt": fx, "w_fmt": fw, "useful_gflop": flop * 1e-9,
                   "products_on_zero_codes": 1.0 - 1.0 / (stride * stride)}
            # (a), (b): NCHW-shaped channels_last views of the de-quantized tensors; the weight as conv_transpose2d wants it [C, Cout, K, K]
            x32 = mx_dequantize(xc, xs, fx).permute(0, 3, 1, 2)
            w32 = mx_dequantize(wc, ws, fw).permute(3, 0, 1, 2).contiguous(memory_format=torch.channels_last)
            assert x32.is_contiguous(memory_format=torch.channels_last)
            ms_a, reps_a = timed(lambda: F.conv_transpose2d(x32, w32, None, stride, padding, out_pad), args.iters, args.warmup)
            x16, w16 = x32.bfloat16(), w32.bfloat16()
            ms_b, reps_b = timed(lambda: F.conv_transpose2d(x16, w16, None, stride, padding, out_pad), args.iters, args.warmup)
            spread = max(reps_a) - min(reps_a)
            rec["conv_transpose2d_f32"] = {"ms": ms_a, "reps_ms": reps_a, "spread_ms": spread, "useful_tflops": flop / ms_a * 1e-9}
            rec["conv_transpose2d_bf16"] = {"ms": ms_b, "reps_ms": reps_b, "spread_ms": max(reps_b) - min(reps_b), "useful_tflops": flop / ms_b * 1e-9}
            # the kernel's result against (a) on a reduced batch: the two sum in float32 in different orders
            nb = min(B, 2)
            got = mx_conv_transpose2d(xc[:nb], xs[:nb], fx, wc, ws, fw, None, stride, padding, out_pad).permute(0, 3, 1, 2)
            ref = F.conv_transpose2d(x32[:nb].double(), w32.double(), None, stride, padding, out_pad)
            err = float((got.double() - ref).abs().max() / ref.abs().max())
            assert err < 1e-4, f"mx_conv_transpose2d is off the float64 transposed convolution by {err} of its largest value"
            rec["max_err_over_max_abs"] = err
            del x32, w32, x16, w16, got, ref
            for dt in (torch.float32, torch.bfloat16):
                name = str(dt).split(".")[1]
                ms, reps = timed(lambda: mx_conv_transpose2d(xc, xs, fx, wc, ws, fw, None, stride, padding, out_pad, 1, dt), args.iters, args.warmup)
                route = _hip.mx_conv_transpose_last_route
                assert route == (_hip.MX_CONV_ROUTE_GEMM if K == 1 else _hip.MX_CONV_ROUTE_VEC)
                ms_g, reps_g = timed(lambda: mx_conv2d_input_grad(xc, xs, fx, wc, ws, fw, (H, H), stride, padding, 1, dt), args.iters, args.warmup)

                def both():
                    _, c, s = quantize_with_mx(x.permute(0, 2, 3, 1), fx, -1, return_codes=True)
                    return mx_conv2d_input_grad(c, s, fx, wc, ws, fw, (H, H), stride, padding, 1, dt)

                ms_e2e, reps_e2e = timed(both, args.iters, args.warmup)
                rec["mx_conv_transpose2d_" + name] = {
                    "ms": ms, "reps_ms": reps, "route": route, "useful_tflops": flop / ms * 1e-9, "ratio_to_conv_transpose2d_f32": ms / ms_a,
                    "ratio_to_conv_transpose2d_bf16": ms / ms_b, "faster_than_f32_by_more_than_its_spread": bool(ms_a - ms > spread)}
                rec["mx_conv2d_input_grad_" + name] = {
                    "ms": ms_g, "reps_ms": reps_g, "ratio_to_conv_transpose2d_f32": ms_g / ms_a, "ratio_to_conv_transpose2d_bf16": ms_g / ms_b,
                    "with_quantize_ms": ms_e2e, "with_quantize_reps_ms": reps_e2e, "with_quantize_ratio_to_conv_transpose2d_f32": ms_e2e / ms_a}
            out["cases"].append(rec)
            print(json.dumps(rec), flush=True)
            with open(args.out, "w") as f:          # (kept current after every case)
                json.dump(out, f, indent=1)
                f.write("\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit the figures were measured on")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_conv_transpose.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_conv_transpose.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
