#!/usr/bin/env python3
"""Time of `mx_conv2d` (the implicit-GEMM kernel on MX codes) next to what an MX convolution costs without it.

    python3 tools/bench_mx_conv.py [--out profiles/mx_conv.json] [--iters 50] [--warmup 10] [--small]

One process.  Per case and operation: `warmup` launches, then HIP events around `iters` back-to-back launches, three times, the
median kept (all three recorded).  Shapes: batch 256, channels_last, from the ResNet-50 body -- 56x56 3x3 64->64, 28x28 3x3
128->128, 14x14 3x3 256->256, 56x56 3x3 128->128 stride 2, 56x56 1x1 256->64; formats FP8 E4M3 x FP8 E4M3, FP8 E4M3 x FP4, FP4 x
FP4; float32 and bf16 output.  On the same values, in the same process:
  (a) F.conv2d on the float32 de-quantized channels_last tensors -- what an MX convolution costs today; THE BAR: mx_conv2d alone no
      slower than (a), judged against the spread of (a)'s own three repetitions (a bar met by less than that spread is not met)
  (b) F.conv2d on their bf16 images -- no MX semantics, for orientation
  (c) an explicit im2col of the codes (written to memory) + mx_matmul -- for orientation: its extra bytes are what the implicit form
      saves; asserted equal to mx_conv2d, bit for bit, on a reduced batch
and the end-to-end figure quantize_with_mx(x) + mx_conv2d (bf16 channels_last activations in), plus mx_matmul alone on the im2col
operands (the same FLOPs through the GEMM kernel).  Needs a GPU: there is no fallback.  `--small` shrinks the batch for a functional
rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMATS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp8_e4m3", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp4_e2m1")]
# H (= W), kernel, C, Cout, stride, padding
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


def im2col(xc, xs, wc, ws, K, stride, padding):
    """the operands of the definition, in torch on the device: A [M, K'], SA, Wp [Cout, K'], SWp (C % 32 == 0 here)"""
    import torch
    import torch.nn.functional as F

    def windows(t, fill):
        B, H, W, E = t.shape
        O = (H + 2 * padding - K) // stride + 1
        tp = F.pad(t, (0, 0, padding, padding, padding, padding), value=fill)
        taps = [tp[:, kh: kh + (O - 1) * stride + 1: stride, kw: kw + (O - 1) * stride + 1: stride, :] for kh in range(K) for kw in range(K)]
        return torch.stack(taps, dim=3).reshape(B * O * O, K * K * E)

    Cout = wc.shape[0]
    return windows(xc, 0), windows(xs, 127), wc.reshape(Cout, -1), ws.reshape(Cout, -1)


def bench(args):
    import torch
    import torch.nn.functional as F
    from qsparse_amd import _hip
    from qsparse_amd.mx_conv import mx_conv2d
    from qsparse_amd.mx_gemm import mx_matmul
    from qsparse_amd.quantize import mx_dequantize, quantize_with_mx
    dev = "cuda:0"
    B = 8 if args.small else 256
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "batch": B, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    for H, K, C, Cout, stride, padding in SHAPES:
        x = torch.randn(B, C, H, H, device=dev, generator=g, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
        w = torch.randn(Cout, K, K, C, device=dev, generator=g) / (K * K * C) ** 0.5
        O = (H + 2 * padding - K) // stride + 1
        flop = 2.0 * B * O * O * Cout * K * K * C
        for fx, fw in FORMATS:
            _, xc, xs = quantize_with_mx(x.permute(0, 2, 3, 1), fx, -1, return_codes=True)
            _, wc, ws = quantize_with_mx(w, fw, -1, return_codes=True)
            rec = {"B": B, "H": H, "W": H, "C": C, "Cout": Cout, "kernel": K, "stride": stride, "padding": padding, "x_fmt": fx, "w_fmt": fw,
                   "gflop": flop * 1e-9}
            # (a), (b): NCHW-shaped channels_last views of the de-quantized tensors
            x32 = mx_dequantize(xc, xs, fx).permute(0, 3, 1, 2)
            w32 = mx_dequantize(wc, ws, fw).permute(0, 3, 1, 2)
            assert x32.is_contiguous(memory_format=torch.channels_last) and w32.is_contiguous(memory_format=torch.channels_last)
            ms_a, reps_a = timed(lambda: F.conv2d(x32, w32, None, stride, padding), args.iters, args.warmup)
            x16, w16 = x32.bfloat16(), w32.bfloat16()
            ms_b, reps_b = timed(lambda: F.conv2d(x16, w16, None, stride, padding), args.iters, args.warmup)
            rec["conv2d_f32"] = {"ms": ms_a, "reps_ms": reps_a, "spread_ms": max(reps_a) - min(reps_a), "tflops": flop / ms_a * 1e-9}
            rec["conv2d_bf16"] = {"ms": ms_b, "reps_ms": reps_b, "tflops": flop / ms_b * 1e-9}
            del x32, w32, x16, w16
            # (c): explicit im2col + mx_matmul, and the equality with mx_conv2d on a reduced batch
            nb = min(B, 4)
            ops = im2col(xc[:nb], xs[:nb], wc, ws, K, stride, padding)
            same = torch.equal(mx_matmul(ops[0], ops[1], fx, ops[2], ops[3], fw), mx_conv2d(xc[:nb], xs[:nb], fx, wc, ws, fw, None, stride, padding).reshape(-1, Cout))
            assert same, "mx_conv2d differs from mx_matmul on the im2col operands"
            del ops

            def explicit():
                A, SA, Wp, SWp = im2col(xc, xs, wc, ws, K, stride, padding)
                return mx_matmul(A, SA, fx, Wp, SWp, fw)

            ms_c, reps_c = timed(explicit, max(1, args.iters // 5), max(1, args.warmup // 5))
            A, SA, Wp, SWp = (t.contiguous() for t in im2col(xc, xs, wc, ws, K, stride, padding))
            ms_g, reps_g = timed(lambda: mx_matmul(A, SA, fx, Wp, SWp, fw), args.iters, args.warmup)
            rec["im2col_plus_mx_matmul"] = {"ms": ms_c, "reps_ms": reps_c, "im2col_bytes": A.numel() + SA.numel(), "x_bytes": xc.numel() + xs.numel()}
            rec["mx_matmul_on_im2col"] = {"ms": ms_g, "reps_ms": reps_g, "tflops": flop / ms_g * 1e-9}
            del A, SA, Wp, SWp
            for dt in (torch.float32, torch.bfloat16):
                ms, reps = timed(lambda: mx_conv2d(xc, xs, fx, wc, ws, fw, None, stride, padding, 1, dt), args.iters, args.warmup)
                route = _hip.mx_conv_last_route
                assert route == (_hip.MX_CONV_ROUTE_GEMM if K == 1 else _hip.MX_CONV_ROUTE_VEC)

                def both():
                    _, c, s = quantize_with_mx(x.permute(0, 2, 3, 1), fx, -1, return_codes=True)
                    return mx_conv2d(c, s, fx, wc, ws, fw, None, stride, padding, 1, dt)

                ms_e2e, reps_e2e = timed(both, args.iters, args.warmup)
                spread = max(reps_a) - min(reps_a)
                rec["mx_conv2d_" + str(dt).split(".")[1]] = {
                    "ms": ms, "reps_ms": reps, "route": route, "tflops": flop / ms * 1e-9, "ratio_to_conv2d_f32": ms / ms_a,
                    "ratio_to_conv2d_bf16": ms / ms_b, "ratio_to_mx_matmul_on_im2col": ms / ms_g,
                    "no_slower_than_conv2d_f32": bool(ms_a - ms > spread),      # the bar, met by more than (a)'s own spread
                    "with_quantize_ms": ms_e2e, "with_quantize_reps_ms": reps_e2e, "with_quantize_ratio_to_conv2d_f32": ms_e2e / ms_a}
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
        raise SystemExit("tools/bench_mx_conv.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_conv.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
