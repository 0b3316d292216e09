#!/usr/bin/env python3
"""Time of `mx_kv_append` (new tokens into the MX KV cache, one launch, the write position read on the device) next to what the project
offered before it for the case most favourable to that: the length `L` known on the HOST and equal for all sequences.

    python3 tools/bench_mx_kv_append.py [--out profiles/mx_kv_append.json] [--iters 20] [--warmup 5] [--small]

One process, the protocol of tools/bench_mx_decode.py: per case and operation `warmup` launches, then HIP events around `iters`
back-to-back launches, three times, the median kept (all three recorded) with the spread.  `kv_len` is not advanced between launches, so
every launch does the same work.
Cases: Hq / Hkv = 32 / 8 (q is not passed: the comparator has no use for it), d = dv = 128, bf16 tokens, FP8 E4M3 and FP4.  Decode: T = 1,
B in {1, 8, 64}, L = 4095 in a cache of S = 4096 (the token closes a block of vt: 31 values come from the tail) and L = 4111 in a cache
of S = 8192 (mid-block; 4096 columns cannot hold it).  Prefill: T = 4096, L = 0, S = 4096, B in {1, 8}.
The comparator, from public functions only -- K: `mx_rope_quantize` with the table slice, `copy_` into the cache; V: `cat(tail floats,
v_new)` transposed, `quantize_with_mx(..., -1)`, `copy_`.  It keeps no tail.  THE BAR: the new launch faster than the comparator by more
than the larger of the two spreads -- `faster_beyond_spread` -- in every case.  `gb_s` is the bytes the append reads and writes (tokens,
tail columns, codes and scale bytes of the rows and blocks touched) per second of the new call, to be read next to the copy rate
bench.py prints.  Needs a GPU: there is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean
nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_flash import compare, stat  # noqa: E402
from bench_mx_gemm import timed  # noqa: E402

FORMATS = ("mxfp8_e4m3", "mxfp4_e2m1")
HKV, D = 8, 128
CASES = [(B, 1, L, S) for L, S in ((4095, 4096), (4111, 8192)) for B in (1, 8, 64)] + [(B, 4096, 0, 4096) for B in (1, 8)]      # (B, T, L, S)
SMALL = [(2, 1, 95, 96), (2, 1, 111, 192), (2, 96, 0, 96)]


def bench(args):
    import torch
    from qsparse_amd import MXKVCache, mx_kv_append, mx_rope_quantize, mx_rope_table, quantize_with_mx
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    for B, T, L, S in (CASES if not args.small else SMALL):
        cos, sin = mx_rope_table(S, D, device=dev)
        k_new, v_new = (torch.randn(B, HKV, T, D, device=dev, generator=g).bfloat16() for _ in range(2))
        for fmt in FORMATS:
            c = MXKVCache(B, HKV, S, D, D, fmt, fmt, dev)
            c.v_tail.copy_(torch.randn(c.v_tail.shape, device=dev, generator=g))
            c.kv_len += L
            lo = L // 32 * 32

            def new():
                mx_kv_append(c.k_codes, c.k_scales, fmt, c.vt_codes, c.vt_scales, fmt, c.v_tail, c.kv_len, k_new, v_new, rope=(cos, sin))

            def old():
                kc, ks = mx_rope_quantize(k_new, cos[L:L + T], sin[L:L + T], row_fmt=fmt)[:2]
                c.k_codes[:, :, L:L + T].copy_(kc)
                c.k_scales[:, :, L:L + T].copy_(ks)
                hist = torch.cat((c.v_tail[..., :L - lo], v_new.transpose(-1, -2).float()), -1)
                vc, vs = quantize_with_mx(hist, fmt, -1, return_codes=True)[1:]
                c.vt_codes[..., lo:L + T].copy_(vc)
                c.vt_scales[..., lo // 32:-(-(L + T) // 32)].copy_(vs)

            rec = {"B": B, "Hkv": HKV, "T": T, "S": S, "kv_len": L, "d": D, "dv": D, "fmt": fmt, "dtype": "bfloat16"}
            rec["host_length_route"] = stat(*timed(old, args.iters, args.warmup))
            rec["append"] = stat(*timed(new, args.iters, args.warmup))
            blocks, stays = -(-(L + T) // 32) - L // 32, (L + T) % 32
            moved = B * HKV * (T * 2 * D * 2 + T * (D + D // 32) + D * blocks * 33 + D * 4 * (L - lo + (min(stays, T) if stays else 0)))
            rec["append"]["gb_s"] = moved / rec["append"]["ms"] / 1e6
            compare(rec, "append", "host_length_route")
            out["cases"].append(rec)
            print(json.dumps(rec), flush=True)
            with open(args.out, "w") as f:          # (kept current after every case)
                json.dump(out, f, indent=1)
                f.write("\n")
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
        raise SystemExit("tools/bench_mx_kv_append.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_kv_append.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
