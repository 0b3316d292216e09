#!/usr/bin/env python3
"""Time of `mx_conv2d_weight_grad` (the batch-blocked implicit-GEMM kernel on MX codes, split along its contraction) and of a whole
forward + backward of `MXTrainConv2d`, next to what the same values cost without them.

    python3 tools/bench_mx_conv_train.py [--out profiles/mx_conv_train.json] [--iters 20] [--warmup 5] [--small] [--part a|b|ab]

One process.  Per case and operation: `warmup` launches, then HIP events around `iters` back-to-back launches, three times, the
median kept (all three recorded).  Shapes: tools/bench_mx_conv.py's five convolutions (batch 256, channels_last, ResNet-50 body);
formats FP8 E4M3 x FP8 E4M3, FP8 E4M3 x FP4, FP4 x FP4 (gradient x activation).
  (a) mx_conv2d_weight_grad at split_k in {1, 4, 16, 64, "auto"}, float32 output, against torch.nn.grad.conv2d_weight on the
      de-quantized channels_last tensors in float32 and on their bf16 images, in the same process.  Recorded per case: the slice
      count "auto" plans, whether "auto" is no slower than split_k = 1 beyond the spread of the repetitions (where the rule
      splits), and whether it is within that spread of the best fixed split_k measured.  The spread of a comparison is the larger
      of the two operations' max - min over their three repetitions.
  (b) forward + backward of MXTrainConv2d (E4M3 / E4M3 / E5M2 and the FP4 triple, bf16 channels_last input) against the simulated
      layer quantize(nn.Conv2d, callback=MXQuantizer(fmt, block_dim=1)) past its timeout on an MX-quantized input, and a plain
      bf16 nn.Conv2d.
No other speed bar is set.  Needs a GPU: there is no fallback.  `--small` shrinks the batch for a functional rehearsal (its numbers
mean nothing)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMATS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp8_e4m3", "mxfp4_e2m1"), ("mxfp4_e2m1", "mxfp4_e2m1")]      # (dy, x)
TRIPLES = [("mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp4_e2m1", "mxfp4_e2m1", "mxfp4_e2m1")]        # (x, w, dy)
# H (= W) of the input, kernel, C, Cout, stride, padding
SHAPES = [(56, 3, 64, 64, 1, 1), (28, 3, 128, 128, 1, 1), (14, 3, 256, 256, 1, 1), (56, 3, 128, 128, 2, 1), (56, 1, 256, 64, 1, 0)]
SPLITS = [1, 4, 16, 64, "auto"]


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


def spread(reps):
    return max(reps) - min(reps)


def part_a(args, out, save):
    import torch
    from qsparse_amd import _hip
    from qsparse_amd.mx_conv_train import mx_conv2d_weight_grad
    from qsparse_amd.mx_gemm import mx_quantize_2way
    from qsparse_amd.quantize import mx_dequantize
    dev = "cuda:0"
    B = 32 if args.small else 256
    g = torch.Generator(device=dev).manual_seed(0)
    for H, K, C, Cout, stride, padding in SHAPES:
        O = (H + 2 * padding - K) // stride + 1
        x = torch.randn(B, H, H, C, device=dev, generator=g, dtype=torch.bfloat16)
        dy = torch.randn(B, O, O, Cout, device=dev, generator=g, dtype=torch.bfloat16) / O
        flop = 2.0 * B * O * O * Cout * K * K * C
        for fg, fx in FORMATS:
            _, _, gc, gs = mx_quantize_2way(dy.view(B, -1), None, fg)
            _, _, xc, xs = mx_quantize_2way(x.view(B, -1), None, fx)
            gc, gs, xc, xs = gc.view(O, O, Cout, B), gs.view(O, O, Cout, -1), xc.view(H, H, C, B), xs.view(H, H, C, -1)
            rec = {"B": B, "H": H, "W": H, "C": C, "Cout": Cout, "OH": O, "OW": O, "kernel": K, "stride": stride, "padding": padding,
                   "dy_fmt": fg, "x_fmt": fx, "useful_gflop": flop * 1e-9, "tiles": -(-Cout // 128) * -(-K * K * C // 128),
                   "steps": -(-O * O * (-(-B // 32) * 32) // 128)}
            # the references: NCHW-shaped channels_last views of the de-quantized tensors
            x32 = mx_dequantize(xc, xs, fx).permute(3, 0, 1, 2).contiguous().permute(0, 3, 1, 2)
            g32 = mx_dequantize(gc, gs, fg).permute(3, 0, 1, 2).contiguous().permute(0, 3, 1, 2)
            assert x32.is_contiguous(memory_format=torch.channels_last) and g32.is_contiguous(memory_format=torch.channels_last)
            size = (Cout, C, K, K)
            ref = lambda a, b: torch.nn.grad.conv2d_weight(a, size, b, stride, padding)
            ms_a, reps_a = timed(lambda: ref(x32, g32), args.iters, args.warmup)
            x16, g16 = x32.bfloat16(), g32.bfloat16()
            ms_b, reps_b = timed(lambda: ref(x16, g16), args.iters, args.warmup)
            rec["conv2d_weight_f32"] = {"ms": ms_a, "reps_ms": reps_a, "spread_ms": spread(reps_a), "useful_tflops": flop / ms_a * 1e-9}
            rec["conv2d_weight_bf16"] = {"ms": ms_b, "reps_ms": reps_b, "spread_ms": spread(reps_b), "useful_tflops": flop / ms_b * 1e-9}
            got = mx_conv2d_weight_grad(gc, gs, fg, xc, xs, fx, K, stride, padding).permute(0, 3, 1, 2)
            want = ref(x32, g32)
            err = float((got.double() - want.double()).abs().max() / want.double().abs().max())
            assert err < 1e-3, f"mx_conv2d_weight_grad is off conv2d_weight by {err} of its largest value"
            rec["max_err_over_max_abs_vs_f32"] = err
            del x32, g32, x16, g16, got, want
            runs = {}
            for S in SPLITS:
                ms, reps = timed(lambda: mx_conv2d_weight_grad(gc, gs, fg, xc, xs, fx, K, stride, padding, 1, torch.float32, S), args.iters,
                                 args.warmup)
                assert _hip.mx_conv_wgrad_last_route == _hip.MX_CONV_ROUTE_VEC
                runs[S] = (ms, reps)
                rec[f"mx_conv2d_weight_grad_split_{S}"] = {
                    "ms": ms, "reps_ms": reps, "spread_ms": spread(reps), "slices": _hip.mx_conv_wgrad_last_split,
                    "useful_tflops": flop / ms * 1e-9, "ratio_to_conv2d_weight_f32": ms / ms_a, "ratio_to_conv2d_weight_bf16": ms / ms_b}
            auto, one = runs["auto"], runs[1]
            best = min((S for S in SPLITS if S != "auto"), key=lambda S: runs[S][0])
            rec["auto"] = {
                "slices": rec["mx_conv2d_weight_grad_split_auto"]["slices"], "best_fixed_split": best, "best_fixed_ms": runs[best][0],
                "no_slower_than_unsplit_beyond_spread": bool(auto[0] - one[0] <= max(spread(auto[1]), spread(one[1]))),
                "within_spread_of_best_fixed": bool(auto[0] - runs[best][0] <= max(spread(auto[1]), spread(runs[best][1])))}
            out["wgrad"].append(rec)
            print(json.dumps(rec), flush=True)
            save()


def part_b(args, out, save):
    import torch
    import torch.nn as nn
    import qsparse_amd as qs
    from qsparse_amd import _hip
    from qsparse_amd.quantize import MXQuantizer, quantize_with_mx
    dev = "cuda:0"
    B = 32 if args.small else 256
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    g = torch.Generator(device=dev).manual_seed(0)
    width = {"mxfp8_e4m3": 8, "mxfp4_e2m1": 4}

    def step_of(layer, inp, grad):
        inp = inp.detach().requires_grad_(True)

        def step():
            inp.grad = None
            for p in layer.parameters():
                p.grad = None
            layer(inp).backward(grad)
        return step

    for H, K, C, Cout, stride, padding in SHAPES:
        O = (H + 2 * padding - K) // stride + 1
        x = torch.randn(B, C, H, H, device=dev, generator=g, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dy = (torch.randn(B, Cout, O, O, device=dev, generator=g, dtype=torch.bfloat16) / O).contiguous(memory_format=torch.channels_last)
        torch.manual_seed(0)
        base = nn.Conv2d(C, Cout, K, stride, padding).to(dev).to(memory_format=torch.channels_last)
        conv16 = nn.Conv2d(C, Cout, K, stride, padding).to(dev).bfloat16().to(memory_format=torch.channels_last)
        ms_b, reps_b = timed(step_of(conv16, x, dy), args.iters, args.warmup)
        del conv16
        for fx, fw, fg in TRIPLES:
            rec = {"B": B, "H": H, "W": H, "C": C, "Cout": Cout, "kernel": K, "stride": stride, "padding": padding, "x_dtype": "bfloat16",
                   "fmts": [fx, fw, fg], "conv2d_bf16": {"ms": ms_b, "reps_ms": reps_b}}
            # the simulated layer past its timeout, on an MX-quantized (float32) input
            sim = qs.quantize(nn.Conv2d(C, Cout, K, stride, padding), bits=width[fw], timeout=1, callback=MXQuantizer(fw, block_dim=1))
            sim = sim.to(dev).to(memory_format=torch.channels_last).train()
            with torch.no_grad():
                sim.weight.copy_(base.weight), sim.bias.copy_(base.bias)
                xq = quantize_with_mx(x, fx, 1)
            sim(xq[:2]), sim(xq[:2])
            ms_a, reps_a = timed(step_of(sim, xq, dy.to(xq.dtype)), args.iters, args.warmup)
            rec["simulated_layer"] = {"ms": ms_a, "reps_ms": reps_a, "input_dtype": str(xq.dtype).split(".")[1]}
            del sim, xq
            layer = qs.MXTrainConv2d.from_conv(base, fx, fw, fg)
            ms, reps = timed(step_of(layer, x, dy), args.iters, args.warmup)
            rec["mx_train_conv2d"] = {"ms": ms, "reps_ms": reps, "wgrad_slices": _hip.mx_conv_wgrad_last_split,
                                      "ratio_to_simulated": ms / ms_a, "ratio_to_conv2d_bf16": ms / ms_b}
            out["layer"].append(rec)
            print(json.dumps(rec), flush=True)
            save()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
    ap.add_argument("--commit", default="", help="recorded in the output: the commit the figures were measured on")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_conv_train.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_conv_train.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup,
           "batch": 32 if args.small else 256, "wgrad": [], "layer": []}
    if os.path.exists(args.out) and args.part != "ab":       # the two parts may be measured in separate runs into one file
        with open(args.out) as f:
            old = json.load(f)
        out["wgrad"], out["layer"] = old.get("wgrad", []), old.get("layer", [])
        out["wgrad" if args.part == "a" else "layer"] = []

    def save():
        with open(args.out, "w") as f:                       # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    if "a" in args.part:
        part_a(args, out, save)
    if "b" in args.part:
        part_b(args, out, save)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
