#!/usr/bin/env python3
"""Time of `mx_grouped_weight_grad` (the ragged weight-gradient kernel on MX codes, group boundaries on the device) and of a forward +
backward of `MXTrainGroupedLinear`, next to the ways to get the same step without them.

    python3 tools/bench_mx_grouped_train.py [--out profiles/mx_grouped_train.json] [--iters 20] [--warmup 5] [--small]

One process.  Per case and operation: `warmup` runs, then HIP events around `iters` back-to-back runs, three times, the median kept
(all three recorded, and their spread).  Cases, all tokens x K x N = 8192 x 1024 x 4096: E = 8 and E = 64, balanced and skewed (half
the tokens in one group).  No ratio was promised for this kernel: the file states what was measured, against what.

Kernel (bf16 dW [E, N, K]; dy E5M2 x x E4M3, FP4 x FP4, E5M2 x FP6 E2M3), on the same values, in the same process:
  (a)  the loop of `mx_matmul` over the groups that have tokens, on the col pairs of every group's OWN rows, quantized outside the
       timed region, the sizes ALREADY on the host.  Its blocks start at the group's first token, so it computes mx_linear's dW, not
       the same bits; the products and the traffic are the same
  (a+) the same loop after the `offs.tolist()` a caller really needs: a device-to-host copy and a synchronisation per call
Layer (bf16 x [T, K], bf16 weight [E, N, K], float32 bias; E4M3 / E4M3 / E5M2), forward + backward with all three gradients:
  (b+) the loop of per-group `mx_linear` after the `offs.tolist()` it needs.  Every group's x and weight are leaves of their own, cut
       outside the timed region, so no slice's backward writes a tensor of the full size: the loop is timed at its best
  (c)  the same loop of float32 `F.linear` steps on float32 leaves.  The bf16 form is NOT run: SKIP_BF16 says why
Needs a GPU: there is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_gemm import timed  # noqa: E402
from bench_mx_grouped import sizes_of  # noqa: E402

KERNEL_FORMATS = [("mxfp8_e5m2", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp8_e5m2", "mxfp6_e2m3")]      # dy, x
LAYER_FORMATS = ("mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2")                                                         # x, W, dy
SKIP_BF16 = ("not run: tools/bench_mx_bmm.py records that bf16 torch.bmm on expert-sized operands ([8, 4096, 1024] x [8, 1024, 4096]) ended in "
             "an illegal memory access on the torch / ROCm build it was measured with, for a cause that was not found; a bf16 F.linear "
             "step per group goes through the same library on the same sizes and is left out rather than run into that again "
             "(tools/bench_mx_grouped.py leaves its bf16 comparator out for the same reason).  The float32 loop stands in")


def stat(ms, reps, flop):
    return {"ms": ms, "reps_ms": reps, "tflops": flop / ms * 1e-9, "spread": (max(reps) - min(reps)) / ms}


def bench(args):
    import torch
    import torch.nn.functional as F
    from qsparse_amd import MXTrainGroupedLinear, _hip, mx_grouped_weight_grad, mx_linear, mx_matmul, mx_quantize_2way
    dev = "cuda:0"
    T, K, N = (8192, 1024, 4096) if not args.small else (1024, 256, 256)
    cases = [("balanced", 8), ("skewed", 8), ("balanced", 64), ("skewed", 64)]
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "T": T, "K": K,
           "N": N, "bf16_linear_loop": SKIP_BF16, "kernel": [], "layer": []}

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    g = torch.Generator(device=dev).manual_seed(0)
    flop = 2.0 * T * N * K
    x = torch.randn(T, K, device=dev, generator=g, dtype=torch.bfloat16)
    dy = torch.randn(T, N, device=dev, generator=g, dtype=torch.bfloat16) / N
    for kind, E in cases:
        sizes = sizes_of(kind, E, T)
        assert sum(sizes) == T and min(sizes) >= 0
        ends = torch.tensor(sizes).cumsum(0)
        bounds = [(lo, hi) for lo, hi in zip([0] + ends.tolist(), ends.tolist()) if hi > lo]
        offs = ends.to(torch.int32).to(dev)
        for fg, fx in KERNEL_FORMATS:
            gt, gs = mx_quantize_2way(dy, None, fg)[2:]
            xt, xs = mx_quantize_2way(x, None, fx)[2:]
            rec = {"E": E, "sizes": kind, "largest_group": max(sizes), "g_fmt": fg, "x_fmt": fx, "out_dtype": "bfloat16"}
            ms, reps = timed(lambda: mx_grouped_weight_grad(gt, gs, fg, xt, xs, fx, offs, torch.bfloat16), args.iters, args.warmup)
            rec["route"] = _hip.mx_grouped_wgrad_last_route
            rec["mx_grouped_weight_grad"] = stat(ms, reps, flop)
            own = [mx_quantize_2way(dy[lo:hi], None, fg)[2:] + mx_quantize_2way(x[lo:hi], None, fx)[2:] for lo, hi in bounds]

            def loop():                         # (a): keeps the results, as the grouped call's one tensor does
                return [mx_matmul(a, sa, fg, b, sb, fx, None, torch.bfloat16) for a, sa, b, sb in own]

            def loop_from_device():             # (a+): the sizes come from the device first
                offs.tolist()
                return loop()

            ms_a, reps_a = timed(loop, args.iters, args.warmup)
            rec["matmul_loop"] = stat(ms_a, reps_a, flop)
            ms_p, reps_p = timed(loop_from_device, args.iters, args.warmup)
            rec["matmul_loop_with_tolist"] = stat(ms_p, reps_p, flop)
            rec["ratio_to_matmul_loop"], rec["ratio_to_matmul_loop_with_tolist"] = ms / ms_a, ms / ms_p
            out["kernel"].append(rec)
            print(json.dumps(rec), flush=True)
            save()
            del own, gt, gs, xt, xs

        # the layer: forward + backward, all three gradients
        fx, fw, fg = LAYER_FORMATS
        w = (torch.randn(E, N, K, device=dev, generator=g, dtype=torch.bfloat16) / K ** 0.5).requires_grad_(True)
        b = torch.randn(E, N, device=dev, generator=g).requires_grad_(True)
        layer = MXTrainGroupedLinear.from_float(w, b, x_fmt=fx, w_fmt=fw, grad_fmt=fg)
        xg = x.clone().requires_grad_(True)
        rec = {"E": E, "sizes": kind, "largest_group": max(sizes), "x_dtype": "bfloat16", "fmts": [fx, fw, fg]}
        ms, reps = timed(lambda: torch.autograd.grad(layer(xg, offs), (xg, layer.weight, layer.bias), dy), args.iters, args.warmup)
        rec["mx_train_grouped_linear"] = stat(ms, reps, 3 * flop)
        live = [e for e, n in enumerate(sizes) if n > 0]
        dys = [dy[lo:hi] for lo, hi in bounds]

        def leaves(dtype):
            return ([x[lo:hi].to(dtype).clone().requires_grad_(True) for lo, hi in bounds],
                    [w[e].detach().to(dtype).clone().requires_grad_(True) for e in live],
                    [b[e].detach().to(dtype).clone().requires_grad_(True) for e in live])

        xs_, ws_, bs_ = leaves(torch.bfloat16)

        def linear_loop():                      # (b+)
            offs.tolist()
            ys = [mx_linear(xe, we, be, fx, fw, fg) for xe, we, be in zip(xs_, ws_, bs_)]
            return torch.autograd.grad(ys, xs_ + ws_ + bs_, dys)

        ms_b, reps_b = timed(linear_loop, args.iters, args.warmup)
        rec["mx_linear_loop_with_tolist"] = stat(ms_b, reps_b, 3 * flop)
        del xs_, ws_, bs_
        x32, w32, b32 = leaves(torch.float32)
        dy32 = [t.float() for t in dys]

        def dense_loop():                       # (c)
            offs.tolist()
            ys = [F.linear(xe, we, be) for xe, we, be in zip(x32, w32, b32)]
            return torch.autograd.grad(ys, x32 + w32 + b32, dy32)

        ms_c, reps_c = timed(dense_loop, args.iters, args.warmup)
        rec["linear_f32_loop_with_tolist"] = stat(ms_c, reps_c, 3 * flop)
        rec["ratio_to_mx_linear_loop_with_tolist"], rec["ratio_to_linear_f32_loop_with_tolist"] = ms / ms_b, ms / ms_c
        out["layer"].append(rec)
        print(json.dumps(rec), flush=True)
        save()
        del x32, w32, b32, dy32, layer, w, b, xg
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit whose kernels were measured")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_grouped_train.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_grouped_train.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
