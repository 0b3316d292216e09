#!/usr/bin/env python3
"""Forward time of the MX block-scaled quantizer next to the tensor-wise ScalerQuantization forward on the same tensors.

    python3 tools/bench_mx.py [--out profiles/mx_forward.json] [--iters 50] [--warmup 10] [--small]

One process.  Per case and kernel: `warmup` launches, then HIP events around `iters` back-to-back launches (repeated three times,
the median is kept).  The tensors are far larger than the 256 MB Infinity Cache (0.9 - 1.2 GB read + written per launch), the output
is float32, no codes: 6 bytes per element for a bf16 input (read 2, write 4) for both quantizers, which is what the fraction of the
8 TB/s roofline is computed from.  Cases: 256 x 197 x 3072 bf16 along the last dim (innermost-axis kernel), 256 x 256 x 56 x 56
bf16 channels_last along C (innermost-axis kernel) and the same tensor NCHW along C (strided-axis kernel).  Needs a GPU: there
is no fallback.  `--small` shrinks the tensors for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8.0e12
BYTES_PER_ELEM = 6          # bf16 in, float32 out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_forward.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit the figures were measured on")
    args = ap.parse_args()
    import torch
    from qsparse_amd import _hip
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx.py measures on the GPU: none found")
    dev = "cuda:0"
    tok, img = ((256, 197, 3072), (256, 256, 56, 56)) if not args.small else ((8, 197, 3072), (8, 256, 56, 56))
    g = torch.Generator(device=dev).manual_seed(0)
    x_tok = torch.randn(tok, device=dev, generator=g, dtype=torch.bfloat16)
    x_img = torch.randn(img, device=dev, generator=g, dtype=torch.bfloat16)
    cases = [("token_major_last_dim", x_tok, -1, _hip.MX_ROUTE_INNER_VEC, True),
             ("channels_last_along_C", x_img.contiguous(memory_format=torch.channels_last), 1, _hip.MX_ROUTE_INNER_VEC, True),
             ("nchw_along_C", x_img, 1, _hip.MX_ROUTE_STRIDED, False)]
    scale = torch.full((1,), 0.05, device=dev)
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup,
           "bytes_per_element_assumed": BYTES_PER_ELEM, "roofline_bytes_per_s": PEAK_BYTES_PER_S, "target_ratio_innermost": 1.10,
           "cases": []}
    for name, x, dim, route, has_target in cases:
        nbytes = x.numel() * BYTES_PER_ELEM
        rec = {"case": name, "shape": list(x.shape), "dtype": "bfloat16", "block_dim": dim, "bytes": nbytes}
        ms, reps = timed(lambda: _hip.quant_fwd("scaler", x, scale, -1, torch.float32), args.iters, args.warmup)
        rec["scaler_fwd"] = {"ms": ms, "reps_ms": reps, "fraction_of_roofline": nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S}
        for fmt in ("mxfp8_e4m3", "mxfp4_e2m1"):
            ms_mx, reps = timed(lambda: _hip.mx_quant_fwd(x, fmt, dim, torch.float32, False), args.iters, args.warmup)
            assert _hip.mx_last_route == route, (name, _hip.mx_last_route)
            rec[fmt] = {"ms": ms_mx, "reps_ms": reps, "fraction_of_roofline": nbytes / (ms_mx * 1e-3) / PEAK_BYTES_PER_S,
                        "ratio_to_scaler_fwd": ms_mx / ms, "route": route}
            if has_target:
                rec[fmt]["meets_target"] = bool(ms_mx / ms <= 1.10)
        out["cases"].append(rec)
        print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
