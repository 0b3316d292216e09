#!/usr/bin/env python3
"""Time of the two-way MX quantizer (`mx_quantize_2way`) and of one linear layer's training step through MX matrix products
(`MXTrainLinear`), next to what the same work costs without them.

    python3 tools/bench_mx_train.py [--out profiles/mx_train.json] [--iters 50] [--warmup 10] [--small] [--commit SHA]

One process.  Per case and operation: `warmup` launches, then HIP events around `iters` back-to-back launches, three times, the
median kept (all three recorded).  The yardsticks use nothing but `quantize_with_mx`, `quantize` and ATen, so the same script run on
a commit without the feature measures the yardsticks alone (and says so).

Two-way quantizer: bf16 [50432, 768], [50432, 3072], [4096, 4096]; E4M3 both ways and FP4 both ways; both pairs written.
  yardstick = the cheaper of the two ways to the same four tensors without the kernel:
    (t) quantize_with_mx(x, f, -1, True) + x.t().contiguous() + quantize_with_mx(xt, f, -1, True)
    (s) quantize_with_mx(x, f, -1, True) + the block_dim=0 strided call + .t().contiguous() of its codes and scales
  THE BAR: the two-way call no slower than the yardstick (its median against the yardstick's slowest repetition is recorded, with
  all repetitions, so any margin can be judged against the yardstick's own spread).  Also the fraction of the 8 TB/s roofline at the
  algorithmic 2 + 1 + 1 + 2/32 bytes per element (no target).
Layer step: forward + backward of one linear, (M, N, K) = the two ViT-B MLP shapes and 4096^3, bf16 input, E4M3 / E4M3 / E5M2.
  (a) the simulated layer, quantize(nn.Linear, callback=MXQuantizer("mxfp8_e4m3", block_dim=1)) past its timeout, on an
      MX-quantized input, forward + backward.  THE BAR: the MXTrainLinear step no slower than (a)
  (b) a plain bf16 nn.Linear, forward + backward -- for information
  and the step's launches one by one (HIP events around each): the four two-way calls and the three GEMMs.  On commits with
  split-K (`wgrad_split_k`) the step is the default one ("auto": the weight gradient of the two ViT shapes is split), the step with
  wgrad_split_k=1 is timed next to it, and the weight-gradient entry of the launch list is the split call, both launches.
  `--no-quantizer` skips the two-way quantizer section, `--no-layer` the layer step.
Stochastic rounding (commits that have it; `--no-stochastic` skips): the two-way call on a gradient-like bf16 tensor of the three
  quantizer shapes, E5M2 and FP4, both pairs, stochastic with a device step counter, next to the nearest-mode call and to the
  yardstick (t) / (s) above in that format.  THE BAR: the stochastic call no slower than the yardstick.  And the layer step with
  grad_fmt FP4 in nearest and in stochastic mode, with the dy call of each timed on its own.
Needs a GPU: there is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12


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


def bench_quantizer(args, out, save):
    import torch
    import qsparse_amd as qs
    from qsparse_amd import _hip
    from qsparse_amd.quantize import quantize_with_mx
    dev = "cuda:0"
    shapes = [(50432, 768), (50432, 3072), (4096, 4096)] if not args.small else [(512, 256), (256, 384)]
    g = torch.Generator(device=dev).manual_seed(0)
    for R, C in shapes:
        x = torch.randn(R, C, device=dev, generator=g, dtype=torch.bfloat16)
        for fmt in ("mxfp8_e4m3", "mxfp4_e2m1"):
            rec = {"R": R, "C": C, "fmt": fmt, "dtype": "bfloat16"}

            def via_transpose():
                _, rc, rs = quantize_with_mx(x, fmt, -1, return_codes=True)
                _, cc, cs = quantize_with_mx(x.t().contiguous(), fmt, -1, return_codes=True)
                return rc, rs, cc, cs

            def via_strided():
                _, rc, rs = quantize_with_mx(x, fmt, -1, return_codes=True)
                _, c, s = quantize_with_mx(x, fmt, 0, return_codes=True)
                return rc, rs, c.t().contiguous(), s.t().contiguous()

            with torch.no_grad():
                ms_t, reps_t = timed(via_transpose, args.iters, args.warmup)
                ms_s, reps_s = timed(via_strided, args.iters, args.warmup)
                rec["via_transpose"] = {"ms": ms_t, "reps_ms": reps_t}
                rec["via_strided"] = {"ms": ms_s, "reps_ms": reps_s}
                yard, yreps = (ms_t, reps_t) if ms_t <= ms_s else (ms_s, reps_s)
                rec["yardstick"] = {"which": "via_transpose" if ms_t <= ms_s else "via_strided", "ms": yard, "reps_ms": yreps,
                                    "spread": (max(yreps) - min(yreps)) / yard}
                if hasattr(qs, "mx_quantize_2way"):
                    want = via_transpose()
                    got = qs.mx_quantize_2way(x, fmt, fmt)
                    assert _hip.mx_quant2_last_route == _hip.MX_Q2_ROUTE_TILE_VEC
                    assert all(torch.equal(a, b) for a, b in zip(got, want)), "the two-way call and the yardstick disagree"
                    ms, reps = timed(lambda: qs.mx_quantize_2way(x, fmt, fmt), args.iters, args.warmup)
                    nbytes = R * C * (2 + 1 + 1 + 2 / 32)
                    rec["two_way"] = {"ms": ms, "reps_ms": reps, "ratio_to_yardstick": ms / yard, "no_slower_than_yardstick": bool(ms <= max(yreps)),
                                      "roofline_fraction": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S}
            out["quantizer"].append(rec)
            print(json.dumps(rec), flush=True)
            save()


def bench_layer(args, out, save):
    import torch
    import torch.nn as nn
    import qsparse_amd as qs
    from qsparse_amd import _hip
    from qsparse_amd.quantize import MXQuantizer, quantize_with_mx
    dev = "cuda:0"
    shapes = [(50432, 3072, 768), (50432, 768, 3072), (4096, 4096, 4096)] if not args.small else [(512, 384, 256), (256, 256, 512)]
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    g = torch.Generator(device=dev).manual_seed(0)
    for M, N, K in shapes:
        rec = {"M": M, "N": N, "K": K, "x_dtype": "bfloat16", "fmts": ["mxfp8_e4m3", "mxfp8_e4m3", "mxfp8_e5m2"]}
        x = torch.randn(M, K, device=dev, generator=g, dtype=torch.bfloat16)
        dy = torch.randn(M, N, device=dev, generator=g, dtype=torch.bfloat16) / N
        torch.manual_seed(0)
        base = nn.Linear(K, N).to(dev)

        def step_of(layer, inp, grad):
            inp = inp.detach().requires_grad_(True)

            def step():
                inp.grad = None
                for p in layer.parameters():
                    p.grad = None
                layer(inp).backward(grad)
            return step

        # (a) the simulated layer past its timeout, on an MX-quantized (float32) input
        sim = qs.quantize(nn.Linear(K, N), bits=8, timeout=1, callback=MXQuantizer("mxfp8_e4m3", block_dim=1)).to(dev).train()
        with torch.no_grad():
            sim.weight.copy_(base.weight), sim.bias.copy_(base.bias)
            xq = quantize_with_mx(x, "mxfp8_e4m3", -1)
        sim(xq), sim(xq)
        ms_a, reps_a = timed(step_of(sim, xq, dy.to(xq.dtype)), args.iters, args.warmup)
        rec["simulated_layer"] = {"ms": ms_a, "reps_ms": reps_a, "input_dtype": str(xq.dtype).split(".")[1]}
        del sim, xq
        # (b) plain bf16
        lin16 = nn.Linear(K, N).to(dev).bfloat16()
        ms_b, reps_b = timed(step_of(lin16, x, dy), args.iters, args.warmup)
        rec["linear_bf16"] = {"ms": ms_b, "reps_ms": reps_b}
        del lin16
        if hasattr(qs, "MXTrainLinear"):
            layer = qs.MXTrainLinear.from_linear(base)
            step = step_of(layer, x, dy)
            ms, reps = timed(step, args.iters, args.warmup)
            rec["mx_train_linear"] = {"ms": ms, "reps_ms": reps, "ratio_to_simulated": ms / ms_a, "ratio_to_linear_bf16": ms / ms_b,
                                      "no_slower_than_simulated": bool(ms <= max(reps_a))}
            if hasattr(layer, "wgrad_split_k"):
                rec["mx_train_linear"]["wgrad_slices"] = _hip.mx_split_plan(N, K, M, 0)[0]
                ms_1, reps_1 = timed(step_of(qs.MXTrainLinear.from_linear(base, wgrad_split_k=1), x, dy), args.iters, args.warmup)
                rec["mx_train_linear_wgrad_unsplit"] = {"ms": ms_1, "reps_ms": reps_1, "ratio_to_linear_bf16": ms_1 / ms_b}
            # the launches of a step one by one, in order: quantizer calls x (both pairs), W (row), dy (both), W (col); GEMMs
            # forward, dgrad, wgrad
            _hip.start_event_log()
            n = 5
            for _ in range(n):
                step()
            log = _hip.stop_event_log()
            q2 = [t for k, v in log.items() if k.startswith("mx_quant2") for t in v]
            mm = [t for k, v in log.items() if k.startswith("mx_matmul[") for t in v]
            wg = [t for k, v in log.items() if k.startswith("mx_matmul_splitk[") for t in v]
            if wg:                                  # a split weight gradient is logged under its own name: back into launch order
                assert len(mm) == 2 * n and len(wg) == n
                mm = [t for i in range(n) for t in (mm[2 * i], mm[2 * i + 1], wg[i])]
            assert len(q2) == 4 * n and len(mm) == 3 * n and len([k for k in log if k.startswith("mx_quant2")]) == 1
            for names, ts in ((("quant2_x_both", "quant2_w_row", "quant2_dy_both", "quant2_w_col"), q2), (("gemm_forward", "gemm_dgrad", "gemm_wgrad"), mm)):
                for i, name in enumerate(names):
                    rec["mx_train_linear"][name + "_ms"] = statistics.median(ts[i::len(names)])
            flop = 2.0 * M * N * K
            for name in ("gemm_forward", "gemm_dgrad", "gemm_wgrad"):
                rec["mx_train_linear"][name + "_tflops"] = flop / rec["mx_train_linear"][name + "_ms"] * 1e-9
        out["layer_step"].append(rec)
        print(json.dumps(rec), flush=True)
        save()


def bench_stochastic(args, out, save):
    import torch
    import qsparse_amd as qs
    from qsparse_amd import _hip
    from qsparse_amd.quantize import quantize_with_mx
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    step_t = torch.zeros(1, dtype=torch.int64, device=dev)
    shapes = [(50432, 768), (50432, 3072), (4096, 4096)] if not args.small else [(512, 256), (256, 384)]
    for R, C in shapes:
        x = torch.randn(R, C, device=dev, generator=g, dtype=torch.bfloat16) / C
        for fmt in ("mxfp8_e5m2", "mxfp4_e2m1"):
            rec = {"R": R, "C": C, "fmt": fmt, "dtype": "bfloat16"}

            def via_transpose():
                _, rc, rs = quantize_with_mx(x, fmt, -1, return_codes=True)
                _, cc, cs = quantize_with_mx(x.t().contiguous(), fmt, -1, return_codes=True)
                return rc, rs, cc, cs

            def via_strided():
                _, rc, rs = quantize_with_mx(x, fmt, -1, return_codes=True)
                _, c, s = quantize_with_mx(x, fmt, 0, return_codes=True)
                return rc, rs, c.t().contiguous(), s.t().contiguous()

            with torch.no_grad():
                ms_t, reps_t = timed(via_transpose, args.iters, args.warmup)
                ms_s, reps_s = timed(via_strided, args.iters, args.warmup)
                yard, yreps = (ms_t, reps_t) if ms_t <= ms_s else (ms_s, reps_s)
                rec["yardstick"] = {"which": "via_transpose" if ms_t <= ms_s else "via_strided", "ms": yard, "reps_ms": yreps,
                                    "spread": (max(yreps) - min(yreps)) / yard}
                ms_n, reps_n = timed(lambda: qs.mx_quantize_2way(x, fmt, fmt), args.iters, args.warmup)
                rec["two_way_nearest"] = {"ms": ms_n, "reps_ms": reps_n}
                # the stochastic call is its own one-way composition, bit for bit (streams 0 / 1), before it is timed
                got = qs.mx_quantize_2way(x, fmt, fmt, "stochastic", 7, step_t)
                assert _hip.mx_quant2_last_route == _hip.MX_Q2_ROUTE_TILE_VEC
                want = (quantize_with_mx(x, fmt, -1, True, "stochastic", 7, step_t, 0)[1:]
                        + quantize_with_mx(x.t().contiguous(), fmt, -1, True, "stochastic", 7, step_t, 1)[1:])
                assert all(torch.equal(a, b) for a, b in zip(got, want)), "the stochastic two-way call and its one-way composition disagree"
                ms, reps = timed(lambda: qs.mx_quantize_2way(x, fmt, fmt, "stochastic", 7, step_t), args.iters, args.warmup)
                nbytes = R * C * (2 + 1 + 1 + 2 / 32)
                rec["two_way_stochastic"] = {"ms": ms, "reps_ms": reps, "ratio_to_nearest": ms / ms_n, "ratio_to_yardstick": ms / yard,
                                             "no_slower_than_yardstick": bool(ms <= max(yreps)),
                                             "roofline_fraction": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S}
            out["stochastic_quantizer"].append(rec)
            print(json.dumps(rec), flush=True)
            save()
    import torch.nn as nn
    shapes = [(50432, 3072, 768), (50432, 768, 3072), (4096, 4096, 4096)] if not args.small else [(512, 384, 256), (256, 256, 512)]
    for M, N, K in shapes:
        rec = {"M": M, "N": N, "K": K, "x_dtype": "bfloat16", "fmts": ["mxfp8_e4m3", "mxfp8_e4m3", "mxfp4_e2m1"]}
        x = torch.randn(M, K, device=dev, generator=g, dtype=torch.bfloat16).requires_grad_(True)
        dy = torch.randn(M, N, device=dev, generator=g, dtype=torch.bfloat16) / N
        torch.manual_seed(0)
        base = nn.Linear(K, N).to(dev)
        for mode in ("nearest", "stochastic"):
            layer = qs.MXTrainLinear.from_linear(base, grad_fmt="mxfp4_e2m1", grad_rounding=mode, seed=3)

            def step():
                x.grad = None
                for p in layer.parameters():
                    p.grad = None
                layer(x).backward(dy)

            ms, reps = timed(step, args.iters, args.warmup)
            _hip.start_event_log()
            for _ in range(5):
                step()
            log = _hip.stop_event_log()
            q2 = [t for k, v in log.items() if k.startswith("mx_quant2") for t in v]
            assert len(q2) == 20
            rec[mode] = {"ms": ms, "reps_ms": reps, "quant2_dy_both_ms": statistics.median(q2[2::4])}
        rec["stochastic"]["ratio_to_nearest"] = rec["stochastic"]["ms"] / rec["nearest"]["ms"]
        out["stochastic_layer_step"].append(rec)
        print(json.dumps(rec), flush=True)
        save()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit the figures were measured on")
    ap.add_argument("--no-stochastic", action="store_true", help="skip the stochastic-rounding cases")
    ap.add_argument("--no-quantizer", action="store_true", help="skip the two-way quantizer cases")
    ap.add_argument("--no-layer", action="store_true", help="skip the layer step (and the stochastic cases, which time it too)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_train.py measures on the GPU: none found")
    import qsparse_amd as qs
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_train.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup,
           "has_two_way": hasattr(qs, "mx_quantize_2way"), "quantizer": [], "layer_step": []}
    if not out["has_two_way"]:
        print("this commit has no mx_quantize_2way / MXTrainLinear: measuring the yardsticks alone", flush=True)

    def save():                                     # (kept current after every case)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if not args.no_quantizer:
        bench_quantizer(args, out, save)
    if not args.no_layer:
        bench_layer(args, out, save)
    import inspect
    if not args.no_layer and out["has_two_way"] and "rounding" in inspect.signature(qs.mx_quantize_2way).parameters and not args.no_stochastic:
        out["stochastic_quantizer"], out["stochastic_layer_step"] = [], []
        bench_stochastic(args, out, save)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
