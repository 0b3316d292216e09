#!/usr/bin/env python3
"""Time of the fused MoE routing -- `mx_moe_route`, `mx_moe_dispatch_quantize`, `mx_moe_combine` -- next to the chains of torch ops they
replace in `MXMoEFeedForward.forward`, on the same tensors, and of the two blocks with `routing="fused"` next to `routing="torch"`.

    python3 tools/bench_mx_moe_route.py [--out profiles/mx_moe_route.json] [--target-ms 100] [--small]

One process.  Per case the operations ALTERNATE (tools/bench_mx_prefill.py's protocol: one untimed launch each, three rounds timed by HIP
events around `iters` back-to-back launches, the median kept and all three recorded with the spread).
Shapes: those of tools/bench_mx_grouped.py (T = 8192 tokens, D = 1024, H = 4096, top 2 of 8 and of 64 experts, balanced and with half
the tokens' first pick on one expert) and decoding batches of T = 8 and 64 with 64 experts, top 8.  bf16 tokens, FP8 E4M3.
THE BAR: every repetition of the fused block faster than every repetition of the default block (`met`), for both blocks.  Needs a GPU:
there is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_flash import stat  # noqa: E402
from bench_mx_prefill import alternate  # noqa: E402

FMT = "mxfp8_e4m3"


def bench(args):
    import torch
    from qsparse_amd import (MXGatedMoEFeedForward, MXMoEFeedForward, mx_moe_combine, mx_moe_dispatch_quantize, mx_moe_route,
                             quantize_with_mx)
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "target_ms": args.target_ms, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    D, H = (1024, 4096) if not args.small else (64, 64)
    cases = [(8192, 8, 2, False), (8192, 8, 2, True), (8192, 64, 2, False), (8192, 64, 2, True), (8, 64, 8, False), (64, 64, 8, False)]
    if args.small:
        cases = [(200, 8, 2, True), (8, 64, 8, False)]
    for T, E, k, skewed in cases:
        w = [torch.randn(s, device=dev, generator=g) * 0.05 for s in ((E, D), (E, H, D), (E, H, D), (E, D, H))]
        x = torch.randn(T, D, device=dev, generator=g).bfloat16()
        if skewed:                      # half the tokens pick expert 0 first
            x[::2] += 4 * w[0][0].bfloat16() / w[0][0].norm() * D ** 0.5
        build = {"plain": lambda r: MXMoEFeedForward.from_float(w[0], w[1], None, w[3], None, k, routing=r),
                 "gated": lambda r: MXGatedMoEFeedForward.from_float(w[0], w[1], None, w[2], None, w[3], None, k, routing=r)}
        logits = x.float() @ w[0].t()
        gates, experts, offs, order, inv = mx_moe_route(logits, k)
        y = torch.randn(T * k, D, device=dev, generator=g)
        ar = torch.arange(E, device=dev)

        def route_torch():
            top, ex = torch.topk(logits, k, -1)
            ids = ex.reshape(-1)
            o = torch.argsort(ids, stable=True)
            return torch.softmax(top, -1), o, (ids.unsqueeze(1) == ar).sum(0).cumsum(0).to(torch.int32)

        fns = {"route": lambda: mx_moe_route(logits, k), "route_torch": route_torch,
               "dispatch": lambda: mx_moe_dispatch_quantize(x, inv, FMT),
               "dispatch_torch": lambda: quantize_with_mx(x[torch.div(order, k, rounding_mode="floor")], FMT, -1, return_codes=True),
               "combine": lambda: mx_moe_combine(y, inv, gates),
               "combine_torch": lambda: (y[torch.argsort(order)].reshape(-1, k, D) * gates.unsqueeze(-1)).sum(1)}
        blocks = {f"{name}_{r}": make(r) for name, make in build.items() for r in ("fused", "torch")}
        for name, moe in blocks.items():
            fns[name] = (lambda m: lambda: m(x))(moe)
        assert bool((offs == route_torch()[2]).all()), "the two routings disagree on the group sizes"
        res, iters = alternate(fns, args.target_ms)
        rec = {"T": T, "E": E, "k": k, "D": D, "H": H, "skewed": skewed, "iters": iters, **{n: stat(*r) for n, r in res.items()}}
        for name in ("route", "dispatch", "combine", "plain", "gated"):
            new, old = (name, name + "_torch") if name in fns else (name + "_fused", name + "_torch")
            rec[f"ratio_{name}"] = rec[new]["ms"] / rec[old]["ms"]
            rec[f"met_{name}"] = bool(max(rec[new]["reps_ms"]) < min(rec[old]["reps_ms"]))
        rec["met"] = rec["met_plain"] and rec["met_gated"]
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:                   # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")
        del w, blocks, fns
    print("wrote", args.out, "bar met in every case:", all(r["met"] for r in out["cases"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--target-ms", type=float, default=100.0)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit whose kernels were measured")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_moe_route.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_moe_route.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
