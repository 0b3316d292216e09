#!/usr/bin/env python3
"""Time of the training side of the fused softmax next to the unfused torch chains it replaces, and of the existing kernels it builds on.

    python3 tools/bench_mx_softmax_train.py [--out profiles/mx_softmax_train.json] [--iters 30] [--warmup 5] [--small] [--parent]

One process, the protocol of tools/bench_mx_softmax.py.  Per case and operation: `warmup` launches, then HIP events around `iters`
back-to-back launches, three times, the median kept (all three recorded, `spread` = (max - min) / median).  On float32 scores
[3072, 197, 197] (ViT-B attention at batch 256 with 12 heads; PLAIN) and [3072, 256, 256] (VEC), without a mask and causal:
  forward   `mx_softmax_quantize(s, scale, is_causal, fmt, col_fmt=fmt, return_stats=True)` against `s * scale`, `+ mask` (built by
            `_attention_mask` inside the timed region, as `mx_attention_train` builds it), `torch.softmax`, `mx_quantize_2way_batched(p)`
  backward  `mx_softmax_backward_quantize(dp, s, m, Z, ...)` against ATen's softmax backward on the kept float32 p
            (`torch._softmax_backward_data`), `* scale`, `mx_quantize_2way_batched(ds)`
then a forward + backward step of `mx_attention_train` on bf16 q, k, v [256, 12, 197, 64] with `softmax="torch"` and `"fused"`.  THE BAR:
fused faster than its chain by more than the chain's spread (`faster_beyond_spread`: the slowest fused repetition under the fastest of
the chain).  Last, the existing `mx_softmax_quantize`, `mx_norm_quantize` and `mx_quantize_2way_batched` on fixed tensors: `--parent`
measures only those (the new calls do not exist on the parent commit), for profiles/mx_softmax_train_parent.json.  Needs a GPU: there is
no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_gemm import timed  # noqa: E402

CASES = [(3072, 197, 197), (3072, 256, 256)]
SMALL_CASES = [(24, 197, 197), (8, 64, 64)]
FMT, GFMT, SCALE = "mxfp8_e4m3", "mxfp8_e5m2", 0.125


def stat(ms, reps):
    return {"ms": ms, "reps_ms": reps, "spread": (max(reps) - min(reps)) / ms}


def versus(fused, chain):
    return {"fused": stat(*fused), "torch_chain": stat(*chain), "ratio_to_chain": fused[0] / chain[0],
            "faster_beyond_spread": bool(max(fused[1]) < min(chain[1]))}


def bench(args):
    import torch
    import qsparse_amd as qs
    from qsparse_amd.mx_bmm import _attention_mask
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup}

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    g = torch.Generator(device=dev).manual_seed(0)
    cases = CASES if not args.small else SMALL_CASES
    if not args.parent:
        out["softmax"] = []
        for G, T, S in cases:
            s = torch.randn(G, T, S, device=dev, generator=g) * 3
            dp = torch.randn(G, T, S, device=dev, generator=g)
            for causal in (False, True):
                rec = {"G": G, "T": T, "S": S, "dtype": "float32", "fmt": FMT, "grad_fmt": GFMT, "causal": causal}
                kw = dict(scale=SCALE, is_causal=causal)
                fused = timed(lambda: qs.mx_softmax_quantize(s, fmt=FMT, col_fmt=FMT, return_stats=True, **kw), args.iters, args.warmup)
                rec["forward_route"] = qs._hip.mx_softmax_quant2_last_route

                def fwd_chain():
                    m = _attention_mask(None, causal, T, S, s.device)
                    u = s * SCALE
                    if m is not None:
                        u = u + m
                    p = torch.softmax(u, -1)
                    return p, qs.mx_quantize_2way_batched(p, FMT, FMT)

                rec["forward"] = versus(fused, timed(fwd_chain, args.iters, args.warmup))
                p = fwd_chain()[0]
                m, Z = qs.mx_softmax_quantize(s, fmt=FMT, return_stats=True, **kw)[2:]
                fused = timed(lambda: qs.mx_softmax_backward_quantize(dp, s, m, Z, row_fmt=GFMT, col_fmt=GFMT, **kw), args.iters, args.warmup)
                rec["backward_route"] = qs._hip.mx_softmax_bwd_last_route
                bwd_chain = lambda: qs.mx_quantize_2way_batched(torch._softmax_backward_data(dp, p, -1, torch.float32) * SCALE, GFMT, GFMT)
                rec["backward"] = versus(fused, timed(bwd_chain, args.iters, args.warmup))
                a, b = qs.mx_softmax_backward_quantize(dp[:8], s[:8], m[:8], Z[:8], row_fmt=GFMT, col_fmt=GFMT, **kw), \
                    qs.mx_quantize_2way_batched(torch._softmax_backward_data(dp[:8], p[:8], -1, torch.float32) * SCALE, GFMT, GFMT)
                rec["ds_row_codes_differing_from_torch"] = float((a[0] != b[0]).float().mean())
                # the same with +0 and -0 counted as equal (E5M2: bit 7 is the sign): where p = 0 the two expressions sign their zero differently
                zeros = ((a[0] & 0x7F) == 0) & ((b[0] & 0x7F) == 0)
                rec["ds_row_codes_differing_beyond_the_sign_of_zero"] = float(((a[0] != b[0]) & ~zeros).float().mean())
                out["softmax"].append(rec)
                print(json.dumps(rec), flush=True)
                save()
                del p, m, Z
            del s, dp

        B, h, T, d = (256, 12, 197, 64) if not args.small else (4, 3, 197, 64)
        q, k, v = (torch.randn(B, h, T, d, device=dev, generator=g, dtype=torch.bfloat16).requires_grad_(True) for _ in range(3))
        do = torch.randn(B, h, T, d, device=dev, generator=g, dtype=torch.bfloat16)
        iters, warmup = max(3, args.iters // 3), max(1, args.warmup // 2)
        att = {"B": B, "heads": h, "T": T, "d": d, "dtype": "bfloat16", "iters": iters, "warmup": warmup}

        def step(sm, causal):
            o = qs.mx_attention_train(q, k, v, is_causal=causal, softmax=sm)
            torch.autograd.grad(o, (q, k, v), do)

        for causal in (False, True):
            t = timed(lambda: step("torch", causal), iters, warmup)
            f = timed(lambda: step("fused", causal), iters, warmup)
            rec = {"torch": stat(*t), "fused": stat(*f), "ratio_fused_to_torch": f[0] / t[0], "faster_beyond_spread": bool(max(f[1]) < min(t[1]))}
            att["causal" if causal else "plain"] = rec
            print(json.dumps({"attention_train": rec, "causal": causal}), flush=True)
        out["attention_train"] = att
        save()
        del q, k, v, do

    # the existing kernels, for the comparison with the parent commit
    G, T, S = cases[0]
    s = torch.randn(G, T, S, device=dev, generator=g) * 3
    x = torch.randn(G * T // 4, 768, device=dev, generator=g, dtype=torch.bfloat16)
    w = torch.ones(768, device=dev)
    ex = {}
    ex["mx_softmax_quantize"] = stat(*timed(lambda: qs.mx_softmax_quantize(s, scale=SCALE, fmt=FMT), args.iters, args.warmup))
    ex["mx_softmax_quantize_causal"] = stat(*timed(lambda: qs.mx_softmax_quantize(s, scale=SCALE, is_causal=True, fmt=FMT), args.iters, args.warmup))
    ex["mx_norm_quantize_two_way"] = stat(*timed(lambda: qs.mx_norm_quantize(x, w, None, norm="rms", fmt=FMT, col_fmt=FMT), args.iters, args.warmup))
    ex["mx_quantize_2way_batched"] = stat(*timed(lambda: qs.mx_quantize_2way_batched(s, FMT, FMT), args.iters, args.warmup))
    ex["mx_quantize_2way_batched_sr"] = stat(*timed(lambda: qs.mx_quantize_2way_batched(s, GFMT, GFMT, "stochastic", 1), args.iters, args.warmup))
    out["existing"] = {"shape": [G, T, S], "norm_shape": list(x.shape), **ex}
    print(json.dumps(out["existing"]), flush=True)
    save()
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent", action="store_true", help="only the kernels that exist on the parent commit")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit whose kernels were measured")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_softmax_train.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_softmax_train_parent.json" if args.parent else "mx_softmax_train.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
