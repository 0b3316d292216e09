#!/usr/bin/env python3
"""Time of `mx_flash_prefill` / `mx_flash_prefill_paged` (GQA attention of a chunk of new tokens on the MX KV cache) next to the only
route the project had before it: the live pages gathered, the cache sliced with a HOST-known length and `repeat_interleave`d r times, a
float32 `[T, L]` additive mask for the bottom-right limit, then `mx_flash_attention(rows="streamed")`.

    python3 tools/bench_mx_prefill.py [--out profiles/mx_prefill.json] [--target-ms 100] [--small]

One process.  Per case three operations ALTERNATE (the protocol of tools/bench_mx_paged.py): `prefill` (the new call), `streamed` (the
comparator's streamed launch ALONE, on a repeated cache and a mask prepared outside the timing) and `route` (the comparator whole:
gather, slice, repeat, mask, launch).  After one untimed launch of each, three rounds, each timed by HIP events around `iters`
back-to-back launches; `iters` is chosen per operation from a first timed launch so that a round takes about `--target-ms` (1 .. 20).
The median of the three is kept, all three recorded with the spread.
Cases: Hq / Hkv = 32 / 8, d = dv = 128, bf16 output, causal; T in {512, 2048} behind a prefix of 0, 4096 or 30720 keys (L = prefix + T),
B in {1, 8}, the cache contiguous or in pages of 32 or 128 (a random table), FP8 E4M3 and FP4.  THE BAR: every repetition of `prefill`
faster than every repetition of `streamed` -- `faster_than_streamed_launch` -- in every case.  `cache_gb_s` is the bytes of cache (codes
and scales of the L live keys of every kv head, once) over the new call's time.  A second set, `square`, has prefix 0 and r = 1, where
the streamed kernel's own `is_causal` applies and no mask is needed: the ratio is reported, with no bar.  Needs a GPU: there is no
fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_flash import stat  # noqa: E402
from bench_mx_paged import pages_of  # noqa: E402

FORMATS, HQ, HKV, D = ("mxfp8_e4m3", "mxfp4_e2m1"), 32, 8, 128


def alternate(fns, target_ms):
    """{name: (median ms, [ms of each round])} of the operations `fns`, timed in turn, round by round"""
    import torch

    def run(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    iters = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        iters[name] = max(1, min(20, int(target_ms / max(run(fn, 1), 1e-3))))
    reps = {name: [] for name in fns}
    for _ in range(3):
        for name, fn in fns.items():
            reps[name].append(run(fn, iters[name]))
    return {name: (statistics.median(r), r) for name, r in reps.items()}, iters


def bench(args):
    import torch
    from qsparse_amd import mx_flash_attention, mx_flash_prefill, mx_flash_prefill_paged, quantize_with_mx
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "target_ms": args.target_ms, "cases": [], "square": []}
    g = torch.Generator(device=dev).manual_seed(0)
    kw = dict(scale=D ** -0.5, out_dtype=torch.bfloat16)

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    def codes(shape, fmt):
        return quantize_with_mx(torch.randn(shape, device=dev, generator=g), fmt, -1, return_codes=True)[1:]

    Ts, prefixes, Bs = ((512, 2048), (0, 4096, 30720), (1, 8)) if not args.small else ((70,), (0, 186), (2,))
    for fmt in FORMATS:
        for T in Ts:
            for prefix in prefixes:
                L = prefix + T
                S = -(-L // 128) * 128                            # the cache's capacity: whole pages of either size
                one = codes((1, HQ, T, D), fmt) + codes((1, HKV, S, D), fmt) + codes((1, HKV, D, S), fmt)
                j, t = torch.arange(L, device=dev)[None, :], torch.arange(T, device=dev)[:, None]
                for B in Bs:
                    qc, qs = (x.repeat(B, 1, 1, 1) for x in one[:2])
                    flat = tuple(x.repeat(B, 1, 1, 1) for x in one[2:])
                    kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
                    for page in (0, 32, 128):                    # 0: the contiguous cache
                        if page:
                            NP = S // page
                            perm = torch.randperm(B * NP, device=dev, generator=g)
                            table, pools = perm.view(B, NP).to(torch.int32), []
                            for x, axis in zip(one[2:], (2, 2, 3, 3)):
                                pool = torch.empty((B * NP,) + pages_of(x, axis, NP).shape[1:], dtype=torch.uint8, device=dev)
                                pool[perm] = pages_of(x, axis, NP).repeat(B, 1, 1, 1)
                                pools.append(pool)
                            live = table[:, :-(-L // page)].reshape(-1).long()
                            new = lambda: mx_flash_prefill_paged(qc, qs, fmt, *pools, fmt, table, kv_len, is_causal=True, **kw)
                        else:
                            new = lambda: mx_flash_prefill(qc, qs, fmt, *flat, fmt, kv_len, is_causal=True, **kw)

                        def prepare():
                            """the parent's operands: gathered, sliced to the host-known L, repeated; the bottom-right mask"""
                            if page:
                                pg = [x.index_select(0, live).unflatten(0, (B, -1)) for x in pools]
                                c = [x.permute(0, 2, 1, 3, 4).flatten(2, 3) for x in pg[:2]] + [x.permute(0, 2, 3, 1, 4).flatten(3, 4) for x in pg[2:]]
                            else:
                                c = list(flat)
                            c = (c[0][:, :, :L], c[1][:, :, :L], c[2][..., :L], c[3][..., :-(-L // 32)])
                            mask = torch.zeros(T, L, device=dev).masked_fill_(j > L - T + t, float("-inf"))
                            return tuple(x.repeat_interleave(HQ // HKV, 1) for x in c), mask

                        rep, mask = prepare()
                        launch = lambda rep=rep, mask=mask: mx_flash_attention(qc, qs, fmt, *rep, fmt, mask, rows="streamed", **kw)
                        assert torch.equal(new().view(torch.int16), launch().view(torch.int16)), "the two routes disagree"
                        res, iters = alternate({"prefill": new, "streamed": launch, "route": lambda: launch(*prepare())}, args.target_ms)
                        rec = {"fmt": fmt, "B": B, "T": T, "prefix": prefix, "page": page, "iters": iters,
                               **{name: stat(*r) for name, r in res.items()}}
                        rec["faster_than_streamed_launch"] = bool(max(rec["prefill"]["reps_ms"]) < min(rec["streamed"]["reps_ms"]))
                        rec["ratio_to_streamed_launch"] = rec["prefill"]["ms"] / rec["streamed"]["ms"]
                        rec["ratio_to_route"] = rec["prefill"]["ms"] / rec["route"]["ms"]
                        rec["cache_gb_s"] = B * HKV * L * (2 * D + D // 32 + D / 32) / rec["prefill"]["ms"] / 1e6
                        out["cases"].append(rec)
                        print(json.dumps(rec), flush=True)
                        save()
                        del rep, mask
                        if page:
                            del pools
        for T in Ts:                                             # r = 1, no prefix: the streamed kernel's own top-left limit is the same limit
            for B in Bs:
                ops = codes((B, HKV, T, D), fmt) + codes((B, HKV, T, D), fmt) + codes((B, HKV, D, T), fmt)
                res, iters = alternate({"prefill": lambda: mx_flash_prefill(*ops[:2], fmt, *ops[2:], fmt, is_causal=True, **kw),
                                        "streamed": lambda: mx_flash_attention(*ops[:2], fmt, *ops[2:], fmt, is_causal=True, rows="streamed",
                                                                               **kw)}, args.target_ms)
                rec = {"fmt": fmt, "B": B, "T": T, "iters": iters, **{name: stat(*r) for name, r in res.items()}}
                rec["ratio_to_streamed_launch"] = rec["prefill"]["ms"] / rec["streamed"]["ms"]
                out["square"].append(rec)
                print(json.dumps(rec), flush=True)
                save()
    out["bar_met_in_every_case"] = all(c["faster_than_streamed_launch"] for c in out["cases"])
    save()
    print("wrote", args.out, "bar met in every case:", out["bar_met_in_every_case"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--target-ms", type=float, default=100.0)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit whose kernels were measured")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_prefill.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_prefill.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
