#!/usr/bin/env python3
"""Time of `mx_flash_decode_paged(shared=...)` -- a batch whose sequences begin with the same pages, the prefix read once per 16 query rows
of the batch -- next to `flat`: the same call without `shared` on tables that name the same pages, which reads the prefix once per
sequence and is the route the project had before.

    python3 tools/bench_mx_decode_shared.py [--out profiles/mx_decode_shared.json] [--iters 20] [--warmup 5] [--small]

One process.  Per case the two routes ALTERNATE: after `warmup` launches of each, three rounds of (shared, flat), each timed by HIP events
around `iters` back-to-back launches; the median of the three is kept, all three recorded with the spread.  Cases: Hq / Hkv = 32 / 8, d =
dv = 128, T = 1, bf16 output, E4M3 and FP4, B in {8, 64}, a shared prefix of {4096, 16384} keys, {256, 2048} own keys behind it, page in
{32, 128}, both split counts "auto".  Recorded per case: the times, the bytes of K, vt and their scales that each route must move
(computed from the shapes: the flat route B times the prefix per kv head, the shared route ceil(B R / 16) times), the ratio of the times,
whether every repetition of the shared call beat every repetition of the flat one, and the largest difference of the two outputs (they are
the same recurrence cut at other chunks).  NO RATIO IS PROMISED.  The keys of the output file that this tool does not write are kept.
Needs a GPU: there is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_flash import stat  # noqa: E402
from bench_mx_paged import alternate, pages_of  # noqa: E402

HQ, HKV, D = 32, 8, 128


def bench(args):
    import torch
    from qsparse_amd import mx_flash_decode_paged, quantize_with_mx
    dev = "cuda:0"
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    out["bench"] = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    kw = dict(scale=D ** -0.5, out_dtype=torch.bfloat16)
    R, per_key = HQ // HKV, D + D // 32 + D + D // 32            # bytes of a key's K row, vt column and their scale bytes, per kv head
    small = args.small
    for fmt in ("mxfp8_e4m3", "mxfp4_e2m1"):
        for prefix in ((4096, 16384) if not small else (256,)):
            for own in ((256, 2048) if not small else (128,)):
                S = prefix + own
                one = sum((quantize_with_mx(torch.randn(shape, device=dev, generator=g), fmt, -1, return_codes=True)[1:]
                           for shape in ((1, HQ, 1, D), (1, HKV, S, D), (1, HKV, D, S))), ())
                for page in (32, 128):
                    NP, NPs = S // page, prefix // page
                    pages = [pages_of(t, axis, NP) for t, axis in zip(one[2:], (2, 2, 3, 3))]
                    for B in ((8, 64) if not small else (5,)):
                        # the pool: the prefix's pages once, every sequence's own pages behind them, all scattered by `perm`
                        P = NPs + B * (NP - NPs)
                        perm = torch.randperm(P, device=dev, generator=g)
                        shared_table = perm[:NPs].to(torch.int32)
                        table = torch.cat((shared_table.expand(B, NPs), perm[NPs:].view(B, NP - NPs).to(torch.int32)), 1).contiguous()
                        pools = []
                        for t in pages:
                            pool = torch.empty((P,) + t.shape[1:], dtype=torch.uint8, device=dev)
                            pool[perm] = torch.cat((t[:NPs], t[NPs:].repeat(B, 1, 1, 1)))
                            pools.append(pool)
                        qc, qs = (t.repeat(B, 1, 1, 1) for t in one[:2])
                        kv_len = torch.full((B,), S, dtype=torch.int32, device=dev)
                        shared = (shared_table, torch.tensor([prefix], dtype=torch.int32, device=dev))
                        fns = {"shared": lambda: mx_flash_decode_paged(qc, qs, fmt, *pools, fmt, table, kv_len, shared=shared, **kw),
                               "flat": lambda: mx_flash_decode_paged(qc, qs, fmt, *pools, fmt, table, kv_len, **kw)}
                        diff = (fns["shared"]().float() - fns["flat"]().float()).abs().max().item()
                        res = alternate(fns, args.iters, args.warmup)
                        rec = {"fmt": fmt, "B": B, "prefix": prefix, "own": own, "page": page, **{name: stat(*r) for name, r in res.items()},
                               "bytes_flat": B * HKV * S * per_key, "bytes_shared": HKV * (-(-B * R // 16) * prefix + B * own) * per_key,
                               "max_abs_diff": diff}
                        rec["ratio_shared_to_flat"] = rec["shared"]["ms"] / rec["flat"]["ms"]
                        rec["faster_beyond_spread"] = bool(max(rec["shared"]["reps_ms"]) < min(rec["flat"]["reps_ms"]))
                        out["bench"]["cases"].append(rec)
                        print(json.dumps(rec), flush=True)
                        with open(args.out, "w") as f:          # (kept current after every case)
                            json.dump(out, f, indent=1)
                            f.write("\n")
                        del pools, qc, qs
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
        raise SystemExit("tools/bench_mx_decode_shared.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_decode_shared.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
