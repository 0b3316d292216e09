#!/usr/bin/env python3
"""Time of `mx_softmax_quantize` (scale, mask, softmax and the MX quantizer in one launch) next to the unfused torch chain it replaces
and a copy of the same bytes, and of `mx_attention` with `softmax="torch"` and `softmax="fused"`.

    python3 tools/bench_mx_softmax.py [--out profiles/mx_softmax.json] [--iters 50] [--warmup 10] [--small]

One process, the protocol of tools/bench_mx_bmm.py.  Per case and operation: `warmup` launches, then HIP events around `iters`
back-to-back launches, three times, the median kept (all three recorded).  Cases: float32 scores [3072, 197, 197] (ViT-B attention at
batch 256 with 12 heads; S = 197 takes the PLAIN route) and [3072, 256, 256] (the VEC route), in FP8 E4M3 and FP4, with no mask, with a
float32 [T, S] mask and with the causal limit.  On the same tensors, in the same process:
  (a) the unfused chain, steps 3 - 6 of `mx_attention`: `s * scale`, `+ mask` (for the causal case the [T, S] mask is built by
      `_attention_mask` inside the timed region, as `mx_attention(softmax="torch")` builds it on every call), `torch.softmax`,
      `quantize_with_mx(p, fmt, -1, return_codes=True)`.  THE BAR: the fused call faster than (a) on every case
  (b) `torch.Tensor.copy_` of a uint8 tensor of half the bytes the fused kernel must move (it reads 4 bytes and writes 1 + 1 / 32 per
      element; the copy reads and writes that many in total): the ceiling.  `ratio_to_copy` is fused / copy
then `mx_attention` on bf16 q, k, v [256, 12, 197, 64] with `softmax="torch"` and with `softmax="fused"`, both measured here; the bar is
"fused" faster than "torch" by more than the spread of the three repetitions.  Needs a GPU: there is no fallback.  `--small` shrinks
the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_gemm import timed  # noqa: E402

FORMATS = ("mxfp8_e4m3", "mxfp4_e2m1")
CASES = [(3072, 197, 197), (3072, 256, 256)]
SMALL_CASES = [(24, 197, 197), (8, 64, 64)]
MODES = ("none", "mask_ts", "causal")


def stat(ms, reps, nbytes):
    return {"ms": ms, "reps_ms": reps, "gbps": nbytes / ms * 1e-6, "spread": (max(reps) - min(reps)) / ms}


def bench(args):
    import torch
    from qsparse_amd import _hip, mx_attention, mx_softmax_quantize
    from qsparse_amd.mx_bmm import _attention_mask
    from qsparse_amd.quantize import quantize_with_mx
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "cases": []}

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    g = torch.Generator(device=dev).manual_seed(0)
    for G, T, S in (CASES if not args.small else SMALL_CASES):
        s = torch.randn(G, T, S, device=dev, generator=g) * 3
        fmask = torch.randn(T, S, device=dev, generator=g)
        scale = 0.125
        n = G * T * S
        nbytes = 4 * n + n + G * T * ((S + 31) // 32)              # what the fused kernel must read and write
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ms_c, reps_c = timed(lambda: dst.copy_(src), args.iters, args.warmup)
        for fmt in FORMATS:
            for mode in MODES:
                mask, causal = (fmask if mode == "mask_ts" else None), mode == "causal"
                rec = {"G": G, "T": T, "S": S, "dtype": "float32", "fmt": fmt, "mode": mode, "bytes": nbytes}
                ms, reps = timed(lambda: mx_softmax_quantize(s, mask, scale=scale, is_causal=causal, fmt=fmt), args.iters, args.warmup)
                rec["route"] = _hip.mx_softmax_last_route
                rec["fused"] = stat(ms, reps, nbytes)

                def chain():
                    m = _attention_mask(mask, causal, T, S, s.device)
                    u = s * scale
                    if m is not None:
                        u = u + m
                    return quantize_with_mx(torch.softmax(u, -1), fmt, -1, return_codes=True)

                ms_a, reps_a = timed(chain, args.iters, args.warmup)
                rec["torch_chain"] = stat(ms_a, reps_a, nbytes)
                rec["copy_same_bytes"] = stat(ms_c, reps_c, nbytes)
                rec["ratio_to_chain"], rec["ratio_to_copy"] = ms / ms_a, ms / ms_c
                rec["faster_than_chain"] = bool(max(reps) < min(reps_a))
                fc, fs = mx_softmax_quantize(s[:8], mask, scale=scale, is_causal=causal, fmt=fmt)
                _, tc, ts = quantize_with_mx(torch.softmax(chain_input(s[:8], scale, mask, causal, T, S, _attention_mask), -1), fmt, -1,
                                             return_codes=True)
                rec["codes_differing_from_torch_softmax"] = float((fc != tc).float().mean())
                rec["scale_bytes_differing_from_torch_softmax"] = float((fs != ts).float().mean())
                out["cases"].append(rec)
                print(json.dumps(rec), flush=True)
                save()
        del s, src, dst

    B, h, T, d = (256, 12, 197, 64) if not args.small else (4, 3, 197, 64)
    q, k, v = (torch.randn(B, h, T, d, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(3))
    att = {"B": B, "heads": h, "T": T, "d": d, "dtype": "bfloat16"}
    iters, warmup = max(3, args.iters // 5), max(1, args.warmup // 5)
    for fmt in FORMATS:
        for causal in (False, True):
            kw = dict(qk_fmt=fmt, p_fmt=fmt, v_fmt=fmt, out_dtype=torch.bfloat16, is_causal=causal)
            rec = {"iters": iters, "warmup": warmup}
            for sm in ("torch", "fused"):
                ms, reps = timed(lambda: mx_attention(q, k, v, softmax=sm, **kw), iters, warmup)
                rec[sm] = {"ms": ms, "reps_ms": reps, "spread": (max(reps) - min(reps)) / ms}
            rec["ratio_fused_to_torch"] = rec["fused"]["ms"] / rec["torch"]["ms"]
            rec["faster_beyond_spread"] = bool(max(rec["fused"]["reps_ms"]) < min(rec["torch"]["reps_ms"]))
            a, b = mx_attention(q[:8], k[:8], v[:8], softmax="torch", **kw).float(), mx_attention(q[:8], k[:8], v[:8], softmax="fused", **kw).float()
            rec["outputs_differing"] = float((a != b).float().mean())
            att[f"{fmt}{'_causal' if causal else ''}"] = rec
            print(json.dumps({fmt: rec, "causal": causal}), flush=True)
    out["attention"] = att
    save()
    print("wrote", args.out)


def chain_input(s, scale, mask, causal, T, S, attention_mask):
    """`s * scale + mask` as the unfused chain forms it"""
    m = attention_mask(mask, causal, T, S, s.device)
    u = s * scale
    return u if m is None else u + m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit whose kernels were measured")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_softmax.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_softmax.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
