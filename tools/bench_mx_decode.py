#!/usr/bin/env python3
"""Time of `mx_flash_decode` (split-KV grouped-query attention on MX codes) next to the only route the project had for a decoding step:
`mx_flash_attention(rows="streamed")` on the cache `repeat_interleave`d over the query heads of each group.

    python3 tools/bench_mx_decode.py [--out profiles/mx_flash_decode.json] [--iters 20] [--warmup 5] [--small]

One process, the protocol of tools/bench_mx_flash.py: per case and operation `warmup` launches, then HIP events around `iters`
back-to-back launches, three times, the median kept (all three recorded) with the spread.
Cases: B in {1, 8, 64}, Hq / Hkv = 32 / 8, d = dv = 128, T = 1, S in {4096, 32768}, FP8 E4M3 and FP4 (one quantized sequence tiled over
B); `kv_splits` 1 and "auto", `kv_len` = S and S / 2.  The comparator runs on the cache repeated and, for S / 2, sliced beforehand; the
repeat is timed on its own (`repeat`) and NOT counted against it.  THE BAR: the new launch(es) faster than the comparator by more than
the larger of the two spreads -- `faster_beyond_spread` -- in every case.  `cache_gb_s` is the bytes of cache codes and scales the
sequences see (up to `kv_len`) per second of the new call, to be read next to the copy rate bench.py prints.  Needs a GPU: there is
no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
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
HQ, HKV, D = 32, 8, 128


def bench(args):
    import torch
    from qsparse_amd import mx_flash_attention, mx_flash_decode, quantize_with_mx
    from qsparse_amd.mx_flash import _decode_splits
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    r = HQ // HKV
    for S in ((4096, 32768) if not args.small else (640,)):
        for fmt in FORMATS:
            one = sum((quantize_with_mx(torch.randn(shape, device=dev, generator=g), fmt, -1, return_codes=True)[1:]
                       for shape in ((1, HQ, 1, D), (1, HKV, S, D), (1, HKV, D, S))), ())
            for B in ((1, 8, 64) if not args.small else (2,)):
                qc, qs, kc, ks, vc, vs = (t.repeat(B, 1, 1, 1) for t in one)
                kw = dict(scale=D ** -0.5, p_fmt=fmt, out_dtype=torch.bfloat16)
                for L in (S, S // 2):
                    kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
                    rec = {"B": B, "Hq": HQ, "Hkv": HKV, "T": 1, "S": S, "kv_len": L, "d": D, "dv": D, "fmt": fmt,
                           "auto_splits": _decode_splits(B * HKV, -(-S // 128))}
                    rec["repeat"] = stat(*timed(lambda: [t.repeat_interleave(r, 1) for t in (kc, ks, vc, vs)], args.iters, args.warmup))
                    rep = [t.repeat_interleave(r, 1) for t in (kc[:, :, :L], ks[:, :, :L], vc[..., :L], vs[..., :L // 32])]
                    rep = [t.reshape((B * HQ,) + t.shape[2:]).contiguous() for t in rep]
                    q3 = (qc.reshape(B * HQ, 1, D), qs.reshape(B * HQ, 1, -1))
                    rec["streamed_repeated"] = stat(*timed(lambda: mx_flash_attention(*q3, fmt, *rep, fmt, rows="streamed", **kw),
                                                           args.iters, args.warmup))
                    del rep
                    seen = B * HKV * L * (2 * D + D // 32) + B * HKV * D * (L // 32)
                    for name, splits in (("decode_1", 1), ("decode_auto", "auto")):
                        rec[name] = stat(*timed(lambda: mx_flash_decode(qc, qs, fmt, kc, ks, vc, vs, fmt, kv_len, kv_splits=splits, **kw),
                                                args.iters, args.warmup))
                        rec[name]["cache_gb_s"] = seen / rec[name]["ms"] / 1e6
                        compare(rec, name, "streamed_repeated", f"{name}_faster_beyond_spread")
                    out["cases"].append(rec)
                    print(json.dumps(rec), flush=True)
                    with open(args.out, "w") as f:          # (kept current after every case)
                        json.dump(out, f, indent=1)
                        f.write("\n")
                del qc, qs, kc, ks, vc, vs
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
        raise SystemExit("tools/bench_mx_decode.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_flash_decode.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
