#!/usr/bin/env python3
"""Time of `mx_flash_decode_paged` (split-KV GQA decoding through a block table) next to the two things the project had before it:
(a) `gather` -- the only earlier route to a pool: the live pages gathered into a contiguous cache with torch indexing, then
`mx_flash_decode`, the gather counted because that route pays it every step; (b) `contiguous` -- `mx_flash_decode` on an already
contiguous cache of the same contents, the ceiling.

    python3 tools/bench_mx_paged.py [--out profiles/mx_paged.json] [--iters 20] [--warmup 5] [--small]

One process.  Per case the three operations ALTERNATE: after `warmup` launches of each, three rounds of (paged, gather, contiguous), each
timed by HIP events around `iters` back-to-back launches; the median of the three is kept, all three recorded with the spread.
Cases: Hq / Hkv = 32 / 8, d = dv = 128, T = 1, bf16 output, FP8 E4M3, B in {1, 8, 64}, S in {4096, 32768} with kv_len in {S, S / 2}, page
in {32, 128}, a random table, `kv_splits="auto"`.  THE BAR: every repetition of the paged call faster than every repetition of (a) --
`faster_than_gather` -- in every case.  `ratio_to_contiguous` is reported, not promised.  The paged append of one token is timed once
per page size against `mx_kv_append` on the contiguous cache; only the ratio is reported.  Needs a GPU: there is no fallback.  `--small`
shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_flash import stat  # noqa: E402

FMT, HQ, HKV, D = "mxfp8_e4m3", 32, 8, 128


def alternate(fns, iters, warmup):
    """{name: (median ms, [ms of each round])} of the operations `fns`, timed in turn, round by round"""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    reps = {name: [] for name in fns}
    for _ in range(3):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            reps[name].append(a.elapsed_time(b) / iters)
    return {name: (statistics.median(r), r) for name, r in reps.items()}


def pages_of(t, axis, NP):
    """[1, Hkv, ...] with NP page on `axis` as NP pages [NP, Hkv, ...]"""
    t = t.unflatten(axis, (NP, -1))
    return (t.permute(0, 2, 1, 3, 4) if axis == 2 else t.permute(0, 3, 1, 2, 4))[0].contiguous()


def bench(args):
    import torch
    from qsparse_amd import mx_flash_decode, mx_flash_decode_paged, mx_kv_append, mx_kv_append_paged, quantize_with_mx
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "cases": [],
           "append": []}
    g = torch.Generator(device=dev).manual_seed(0)
    kw = dict(scale=D ** -0.5, out_dtype=torch.bfloat16)

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    for S in ((4096, 32768) if not args.small else (640,)):
        one = sum((quantize_with_mx(torch.randn(shape, device=dev, generator=g), FMT, -1, return_codes=True)[1:]
                   for shape in ((1, HQ, 1, D), (1, HKV, S, D), (1, HKV, D, S))), ())
        for page in (32, 128):
            NP = S // page
            for B in ((1, 8, 64) if not args.small else (2,)):
                P = B * NP
                perm = torch.randperm(P, device=dev, generator=g)
                table = perm.view(B, NP).to(torch.int32)
                pools = []
                for t, axis in zip(one[2:], (2, 2, 3, 3)):       # one quantized sequence tiled over B, its pages scattered by `perm`
                    pool = torch.empty((P,) + pages_of(t, axis, NP).shape[1:], dtype=torch.uint8, device=dev)
                    pool[perm] = pages_of(t, axis, NP).repeat(B, 1, 1, 1)
                    pools.append(pool)
                qc, qs = (t.repeat(B, 1, 1, 1) for t in one[:2])
                flat = tuple(t.repeat(B, 1, 1, 1) for t in one[2:])
                for L in (S, S // 2):
                    kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
                    live = table[:, :-(-L // page)].reshape(-1).long()

                    def gather():
                        pg = [t.index_select(0, live).unflatten(0, (B, -1)) for t in pools]
                        k, ks = (t.permute(0, 2, 1, 3, 4).flatten(2, 3) for t in pg[:2])
                        vt, vts = (t.permute(0, 2, 3, 1, 4).flatten(3, 4) for t in pg[2:])
                        return mx_flash_decode(qc, qs, FMT, k, ks, vt, vts, FMT, kv_len, **kw)

                    res = alternate({"paged": lambda: mx_flash_decode_paged(qc, qs, FMT, *pools, FMT, table, kv_len, **kw),
                                     "gather": gather,
                                     "contiguous": lambda: mx_flash_decode(qc, qs, FMT, *flat, FMT, kv_len, **kw)}, args.iters, args.warmup)
                    rec = {"B": B, "S": S, "kv_len": L, "page": page, **{name: stat(*r) for name, r in res.items()}}
                    rec["faster_than_gather"] = bool(max(rec["paged"]["reps_ms"]) < min(rec["gather"]["reps_ms"]))
                    rec["ratio_to_gather"] = rec["paged"]["ms"] / rec["gather"]["ms"]
                    rec["ratio_to_contiguous"] = rec["paged"]["ms"] / rec["contiguous"]["ms"]
                    out["cases"].append(rec)
                    print(json.dumps(rec), flush=True)
                    save()
                if B == (8 if not args.small else 2) and S == (4096 if not args.small else 640):      # one token appended at S / 2
                    kv_len = torch.full((B,), S // 2, dtype=torch.int32, device=dev)
                    k, v = (torch.randn(B, HKV, 1, D, device=dev, generator=g).bfloat16() for _ in range(2))
                    tail = torch.zeros(B, HKV, D, 32, device=dev)
                    res = alternate({"paged": lambda: mx_kv_append_paged(*pools[:2], FMT, *pools[2:], FMT, tail, table, kv_len, k, v),
                                     "contiguous": lambda: mx_kv_append(*flat[:2], FMT, *flat[2:], FMT, tail, kv_len, k, v)},
                                    args.iters, args.warmup)
                    rec = {"B": B, "S": S, "page": page, **{name: stat(*r) for name, r in res.items()}}
                    rec["ratio_to_contiguous"] = rec["paged"]["ms"] / rec["contiguous"]["ms"]
                    out["append"].append(rec)
                    print(json.dumps(rec), flush=True)
                    save()
                del pools, flat, qc, qs
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
        raise SystemExit("tools/bench_mx_paged.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_paged.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
