#!/usr/bin/env python3
"""Time of `mx_bmm` (the batched block-scaled MFMA kernel on MX codes) next to the ways to get the same products without it, and of
`mx_attention` next to bf16 `F.scaled_dot_product_attention`.

    python3 tools/bench_mx_bmm.py [--out profiles/mx_bmm.json] [--iters 50] [--warmup 10] [--small]

One process.  Per case and operation: `warmup` launches, then HIP events around `iters` back-to-back launches, three times, the
median kept (all three recorded).  Cases (ViT-B attention at batch 256 with 12 heads, and an expert-style one): G = 3072 of 197 x 197
x 64 (Q . K^T), G = 3072 of 197 x 64 x 197 (P . V), G = 8 of 4096 x 4096 x 1024; formats FP8 E4M3 x FP8 E4M3, FP4 x FP4 and FP8 E4M3 x
FP6 E2M3 (the pair with the most registers); float32 output.  On the same values, in the same process:
  (a) the loop of `mx_matmul` over the G slices -- existing code, what a user writes today; THE BAR: mx_bmm faster than (a).  The loop
      costs G launches per repetition, so for G > 64 it is timed over `--loop-iters` repetitions after `--loop-warmup`.  The loop KEEPS
      its G results, as `mx_bmm`'s one tensor does.  A loop that drops each `y` at once is timed too, for the record
      (`matmul_loop_discarding_results`): the caching allocator then hands the same block to every slice, the stores of 8 x 4096 x 4096
      float32 land on one 64 MiB block instead of 512 MiB, and the very same launches take 11 % less -- that loop computes nothing a
      caller can use
  (b) torch.bmm in float32 on the de-quantized operands -- what an MX model pays today; reported
  (c) torch.bmm on their bf16 images -- for orientation.  A case of CASES may name a reason to leave (c) out, which is recorded in
      its place: the expert-style case does (SKIP_BF16_EXPERTS)
then `mx_attention` on bf16 q, k, v [256, 12, 197, 64] against F.scaled_dot_product_attention on the same tensors, and -- a record, not a
test -- the relative error of `mx_attention` against float64 attention on the float inputs (the first 8 images).  Needs a GPU: there
is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_gemm import timed  # noqa: E402

FORMATS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp8_e4m3", "mxfp6_e2m3")]
SKIP_BF16_EXPERTS = ("not run: torch.bmm in bf16 on [8, 4096, 1024] x [8, 1024, 4096] ended in an illegal memory access on the torch / ROCm "
                     "build first measured with, after mx_bmm, the mx_matmul loop and the float32 torch.bmm had each synchronised clean on "
                     "the same case; the cause is supposed to lie in the library and was not found")
# G, M, N, K, and None or the reason baseline (c) is left out of the case
CASES = [(3072, 197, 197, 64, None), (3072, 197, 64, 197, None), (8, 4096, 4096, 1024, SKIP_BF16_EXPERTS)]
SMALL_CASES = [(24, 197, 197, 64, None), (2, 256, 256, 256, None)]


def stat(ms, reps, flop):
    return {"ms": ms, "reps_ms": reps, "tflops": flop / ms * 1e-9, "spread": (max(reps) - min(reps)) / ms}


def bench(args):
    import torch
    import torch.nn.functional as F
    from qsparse_amd import _hip, mx_attention, mx_bmm, mx_matmul
    from qsparse_amd.quantize import mx_dequantize, quantize_with_mx
    dev = "cuda:0"
    cases = CASES if not args.small else SMALL_CASES
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup,
           "loop_iters": args.loop_iters, "loop_warmup": args.loop_warmup, "cases": []}

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    g = torch.Generator(device=dev).manual_seed(0)
    for G, M, N, K, skip_bf16 in cases:
        x = torch.randn(G, M, K, device=dev, generator=g, dtype=torch.bfloat16)
        w = torch.randn(G, N, K, device=dev, generator=g, dtype=torch.bfloat16)
        flop = 2.0 * G * M * N * K
        for fa, fb in FORMATS:
            _, ac, asc = quantize_with_mx(x, fa, -1, return_codes=True)
            _, bc, bsc = quantize_with_mx(w, fb, -1, return_codes=True)
            rec = {"G": G, "M": M, "N": N, "K": K, "a_fmt": fa, "b_fmt": fb}
            ms, reps = timed(lambda: mx_bmm(ac, asc, fa, bc, bsc, fb), args.iters, args.warmup)
            rec["route"] = _hip.mx_bmm_last_route
            rec["mx_bmm"] = stat(ms, reps, flop)

            def loop():                         # keeps the G results, as mx_bmm's one tensor does: G M N elements of output
                return [mx_matmul(ac[s], asc[s], fa, bc[s], bsc[s], fb) for s in range(G)]

            def loop_discarding():              # every y dies at once and the allocator hands the same block to the next slice
                for s in range(G):
                    mx_matmul(ac[s], asc[s], fa, bc[s], bsc[s], fb)

            li, lw = (args.iters, args.warmup) if G <= 64 else (args.loop_iters, args.loop_warmup)
            ms_a, reps_a = timed(loop, li, lw)
            rec["matmul_loop"] = dict(stat(ms_a, reps_a, flop), iters=li, warmup=lw)
            ms_d, reps_d = timed(loop_discarding, li, lw)
            rec["matmul_loop_discarding_results"] = dict(stat(ms_d, reps_d, flop), iters=li, warmup=lw)
            a32, b32 = mx_dequantize(ac, asc, fa), mx_dequantize(bc, bsc, fb)
            bt32 = b32.transpose(1, 2)
            ms_b, reps_b = timed(lambda: torch.bmm(a32, bt32), args.iters, args.warmup)
            rec["bmm_f32"] = stat(ms_b, reps_b, flop)
            if skip_bf16 is None:
                a16, bt16 = a32.bfloat16(), b32.bfloat16().transpose(1, 2)
                ms_c, reps_c = timed(lambda: torch.bmm(a16, bt16), args.iters, args.warmup)
                rec["bmm_bf16"] = stat(ms_c, reps_c, flop)
                del a16, bt16
            else:
                ms_c, rec["bmm_bf16"] = None, skip_bf16
            del a32, b32, bt32
            rec["ratio_to_matmul_loop"], rec["ratio_to_bmm_f32"] = ms / ms_a, ms / ms_b
            rec["ratio_to_bmm_bf16"] = None if ms_c is None else ms / ms_c
            rec["faster_than_matmul_loop"] = bool(ms < min(reps_a))
            out["cases"].append(rec)
            print(json.dumps(rec), flush=True)
            save()
        del x, w

    B, h, T, d = (256, 12, 197, 64) if not args.small else (4, 3, 197, 64)
    q, k, v = (torch.randn(B, h, T, d, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(3))
    ms_s, reps_s = timed(lambda: F.scaled_dot_product_attention(q, k, v), args.iters, args.warmup)
    att = {"B": B, "heads": h, "T": T, "d": d, "dtype": "bfloat16", "sdpa_bf16": {"ms": ms_s, "reps_ms": reps_s}}
    for fmt in ("mxfp8_e4m3", "mxfp4_e2m1"):
        kw = dict(qk_fmt=fmt, p_fmt=fmt, v_fmt=fmt, out_dtype=torch.bfloat16)
        ms, reps = timed(lambda: mx_attention(q, k, v, **kw), max(3, args.iters // 5), max(1, args.warmup // 5))
        n = min(B, 8)
        q64, k64, v64 = (t[:n].double() for t in (q, k, v))
        ref = torch.softmax(q64 @ k64.transpose(-1, -2) * d ** -0.5, -1) @ v64
        got = mx_attention(q[:n].float(), k[:n].float(), v[:n].float(), qk_fmt=fmt, p_fmt=fmt, v_fmt=fmt).double()
        att[fmt] = {"ms": ms, "reps_ms": reps, "ratio_to_sdpa_bf16": ms / ms_s,
                    "rel_err_vs_float64": {"max_abs_err_over_max_abs": float((got - ref).abs().max() / ref.abs().max()),
                                           "rms_err_over_rms": float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())}}
        print(json.dumps({fmt: att[fmt]}), flush=True)
    out["attention"] = att
    save()
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--loop-iters", type=int, default=5)
    ap.add_argument("--loop-warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit whose kernels were measured")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_bmm.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_bmm.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
