#!/usr/bin/env python3
"""Time of the batched two-way MX quantizer (`mx_quantize_2way_batched`) and of an attention training step on MX codes
(`mx_attention_train`), next to what the same work costs without them, and the gradient error of that step.

    python3 tools/bench_mx_bmm_train.py [--out profiles/mx_bmm_train.json] [--iters 20] [--warmup 5] [--small] [--commit SHA]

One process.  Per operation: `warmup` calls, then HIP events around `iters` back-to-back calls, three times, the median kept (all three
recorded), as tools/bench_mx_bmm.py does.

(1) Quantizer: [3072, 197, 64] and [3072, 197, 197], bf16 and float32, E4M3, both pairs.
    (a) the loop of mx_quantize_2way over the slices (one repetition of three calls: it is G launches)
    (b) the cheapest composition of existing calls that yields the same four tensors: quantize_with_mx(x) + x.transpose(-1,
        -2).contiguous() + quantize_with_mx of that
    THE BAR: faster than (b) by more than (b)'s own spread (max - min of its three repetitions).
(2) Attention step: forward + backward of mx_attention_train at [256, 12, 197, 64] bf16, next to bf16
    F.scaled_dot_product_attention forward + backward and to the same composition with the quantizer replaced by (b).  No bar.
(3) Error record: the gradients of mx_attention_train against float64 attention on the same float inputs, max and rms relative to the
    reference's rms, formats all E4M3 (gradients E5M2) and all FP4.  A record, not a test.
Needs a GPU: there is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup, reps=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return {"ms": statistics.median(out), "reps_ms": out}


def via_existing(x, row_fmt, col_fmt, rounding="nearest", seed=0, step=None):
    """(b): the four tensors of mx_quantize_2way_batched from calls that existed before it"""
    from qsparse_amd.quantize import quantize_with_mx
    rc = rs = cc = cs = None
    if row_fmt is not None:
        _, rc, rs = quantize_with_mx(x.detach(), row_fmt, -1, True, rounding, seed, step, 0)
    if col_fmt is not None:
        _, cc, cs = quantize_with_mx(x.detach().transpose(-1, -2).contiguous(), col_fmt, -1, True, rounding, seed, step, 1)
    return rc, rs, cc, cs


def bench_quantizer(args, out, save):
    import torch
    import qsparse_amd as qs
    dev, fmt = "cuda:0", "mxfp8_e4m3"
    shapes = [(3072, 197, 64), (3072, 197, 197)] if not args.small else [(24, 45, 64), (24, 45, 45)]
    g = torch.Generator(device=dev).manual_seed(0)
    for shape in shapes:
        for dtype in (torch.bfloat16, torch.float32):
            x = torch.randn(shape, device=dev, generator=g, dtype=dtype)
            rec = {"shape": list(shape), "dtype": str(dtype).split(".")[1], "fmt": fmt}
            with torch.no_grad():
                want = via_existing(x, fmt, fmt)
                got = qs.mx_quantize_2way_batched(x, fmt, fmt)
                assert all(torch.equal(a, b) for a, b in zip(got, want)), "the batched call and (b) disagree"
                rec["route"] = qs._hip.mx_quant2_batched_last_route
                rec["batched"] = timed(lambda: qs.mx_quantize_2way_batched(x, fmt, fmt), args.iters, args.warmup)
                rec["b_existing_calls"] = b = timed(lambda: via_existing(x, fmt, fmt), args.iters, args.warmup)
                rec["a_slice_loop"] = timed(lambda: [qs.mx_quantize_2way(x[s], fmt, fmt) for s in range(shape[0])], 3, 1, reps=1)
            b["spread_ms"] = max(b["reps_ms"]) - min(b["reps_ms"])
            rec["ratio_to_b"] = rec["batched"]["ms"] / b["ms"]
            rec["faster_than_b_by_more_than_its_spread"] = bool(rec["batched"]["ms"] < b["ms"] - b["spread_ms"])
            out["quantizer"].append(rec)
            print(json.dumps(rec), flush=True)
            save()


def bench_attention(args, out, save):
    import torch
    import torch.nn.functional as F
    import qsparse_amd as qs
    import qsparse_amd.mx_batched_train as M
    dev = "cuda:0"
    shape = (256, 12, 197, 64) if not args.small else (4, 2, 45, 64)
    g = torch.Generator(device=dev).manual_seed(1)
    q, k, v = (torch.randn(shape, device=dev, generator=g, dtype=torch.bfloat16).requires_grad_(True) for _ in range(3))
    do = torch.randn(shape, device=dev, generator=g, dtype=torch.bfloat16)

    def step_of(fn):
        def step():
            q.grad = k.grad = v.grad = None
            fn(q, k, v).backward(do)
        return step

    rec = {"shape": list(shape), "dtype": "bfloat16", "fmts": "mxfp8_e4m3 x3, grad mxfp8_e5m2"}
    rec["mx_attention_train"] = timed(step_of(qs.mx_attention_train), args.iters, args.warmup)
    rec["sdpa_bf16"] = timed(step_of(F.scaled_dot_product_attention), args.iters, args.warmup)
    real = M.mx_quantize_2way_batched
    M.mx_quantize_2way_batched = via_existing
    try:
        rec["composition_with_b"] = timed(step_of(qs.mx_attention_train), args.iters, args.warmup)
    finally:
        M.mx_quantize_2way_batched = real
    rec["ratio_to_sdpa_bf16"] = rec["mx_attention_train"]["ms"] / rec["sdpa_bf16"]["ms"]
    rec["ratio_to_composition_with_b"] = rec["mx_attention_train"]["ms"] / rec["composition_with_b"]["ms"]
    out["attention_step"].append(rec)
    print(json.dumps(rec), flush=True)
    save()


def error_record(args, out, save):
    import torch
    import qsparse_amd as qs
    dev = "cuda:0"
    shape = (4, 12, 197, 64) if not args.small else (2, 2, 45, 64)
    g = torch.Generator(device=dev).manual_seed(2)
    q, k, v = (torch.randn(shape, device=dev, generator=g).requires_grad_(True) for _ in range(3))
    do = torch.randn(shape, device=dev, generator=g)
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    o64 = torch.softmax(q64 @ k64.transpose(-1, -2) * shape[-1] ** -0.5, -1) @ v64
    ref = (o64.detach(),) + torch.autograd.grad(o64, (q64, k64, v64), do.double())
    for name, fmts in (("e4m3", dict(qk_fmt="mxfp8_e4m3", p_fmt="mxfp8_e4m3", v_fmt="mxfp8_e4m3", grad_fmt="mxfp8_e5m2")),
                       ("fp4", dict(qk_fmt="mxfp4_e2m1", p_fmt="mxfp4_e2m1", v_fmt="mxfp4_e2m1", grad_fmt="mxfp4_e2m1"))):
        o = qs.mx_attention_train(q, k, v, **fmts)
        got = (o.detach(),) + torch.autograd.grad(o, (q, k, v), do)
        rec = {"shape": list(shape), "dtype": "float32", "formats": name}
        for what, a, b in zip(("o", "dq", "dk", "dv"), got, ref):
            err, rms = (a.double() - b).abs(), b.square().mean().sqrt()
            rec[what] = {"max_over_ref_rms": float(err.max() / rms), "rms_over_ref_rms": float(err.square().mean().sqrt() / rms)}
        out["gradient_error"].append(rec)
        print(json.dumps(rec), flush=True)
        save()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit the figures were measured on")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_bmm_train.py measures on the GPU: none found")
    import qsparse_amd as qs
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_bmm_train.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "small": args.small,
           "quantizer": [], "attention_step": [], "gradient_error": []}

    def save():                                     # (kept current after every case)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    bench_quantizer(args, out, save)
    bench_attention(args, out, save)
    error_record(args, out, save)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
