#!/usr/bin/env python3
"""Time of `mx_flash_attention` (Q . K^T, the softmax quantizer and P . V on MX codes in one launch) next to the chain it is defined as,
`mx_bmm` -> `mx_softmax_quantize` -> `mx_bmm` on the same codes, of its streamed form (`rows="streamed"`, any S; a third column) and of
`mx_attention(softmax="fused")` with both `impl` values.

    python3 tools/bench_mx_flash.py [--out profiles/mx_flash_stream.json] [--iters 50] [--warmup 10] [--small]

One process, the protocol of tools/bench_mx_bmm.py.  Per case and operation: `warmup` launches, then HIP events around `iters`
back-to-back launches, three times, the median kept (all three recorded) with the spread.
Cases: codes of q, k [G, T, d] and v^T [G, d, T] for [3072, 197, 64] and [3072, 256, 64] (ViT-B attention at batch 256 with 12 heads;
197 takes the PLAIN route) in FP8 E4M3 and FP4, plain and causal, [1024, 512, 128] (the wide kernel) and, past the resident kernel's
range, [256, 2048, 128] and [64, 8192, 128] in E4M3 (chain and streamed only).  THE BAR: the one launch faster than the chain by more
than the chain's spread -- `faster_beyond_spread` for the resident kernel, `streamed_faster_beyond_spread` for the streamed one -- in
every case; `outputs_equal` is the identity at the timed size (the streamed kernel has numerics of its own: `streamed_max_diff` is its
largest distance from the chain's output, for the record).  Then `mx_attention` on bf16 q, k, v [256, 12, 197, 64] with `impl="composed"` and `impl="flash"`, and bf16
`F.scaled_dot_product_attention` on the same tensors for the record.  Needs a GPU: there is no fallback.  `--small` shrinks the
shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_gemm import timed  # noqa: E402

FORMATS = ("mxfp8_e4m3", "mxfp4_e2m1")
CASES = [(3072, 197, 64, FORMATS), (3072, 256, 64, FORMATS), (1024, 512, 128, FORMATS[:1]), (256, 2048, 128, FORMATS[:1]),
         (64, 8192, 128, FORMATS[:1])]
SMALL_CASES = [(24, 197, 64, FORMATS), (8, 512, 128, FORMATS[:1]), (2, 640, 128, FORMATS[:1])]


def stat(ms, reps):
    return {"ms": ms, "reps_ms": reps, "spread": (max(reps) - min(reps)) / ms}


def compare(rec, new, old, key="faster_beyond_spread"):
    rec[f"ratio_{new}_to_{old}"] = rec[new]["ms"] / rec[old]["ms"]
    rec[key] = bool(max(rec[new]["reps_ms"]) < min(rec[old]["reps_ms"]))


def bench(args):
    import torch
    import torch.nn.functional as F
    from qsparse_amd import _hip, mx_attention, mx_bmm, mx_flash_attention, mx_softmax_quantize, quantize_with_mx
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "cases": []}

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    g = torch.Generator(device=dev).manual_seed(0)
    for G, T, d, formats in (CASES if not args.small else SMALL_CASES):
        q, k = (torch.randn(G, T, d, device=dev, generator=g) for _ in range(2))
        vt = torch.randn(G, d, T, device=dev, generator=g)
        for fmt in formats:
            (qc, qs), (kc, ks), (vc, vs) = (quantize_with_mx(t, fmt, -1, return_codes=True)[1:] for t in (q, k, vt))
            for causal in (False, True):
                kw = dict(scale=d ** -0.5, is_causal=causal)

                def flash(rows="resident"):
                    return mx_flash_attention(qc, qs, fmt, kc, ks, vc, vs, fmt, p_fmt=fmt, out_dtype=torch.bfloat16, rows=rows, **kw)

                def streamed():
                    return flash("streamed")

                def chain():
                    pc, ps = mx_softmax_quantize(mx_bmm(qc, qs, fmt, kc, ks, fmt), fmt=fmt, **kw)
                    return mx_bmm(pc, ps, fmt, vc, vs, fmt, None, torch.bfloat16)

                rec = {"G": G, "T": T, "S": T, "d": d, "dv": d, "fmt": fmt, "causal": causal}
                resident = T <= _hip.MX_FLASH_MAX_S
                for name, fn in (("chain", chain),) + ((("flash", flash),) if resident else ()) + (("streamed", streamed),):
                    rec[name] = stat(*timed(fn, args.iters, args.warmup))
                rec["route"] = _hip.mx_flash_last_route
                want = chain()
                if resident:
                    compare(rec, "flash", "chain")
                    rec["outputs_equal"] = bool(torch.equal(flash().view(torch.int16), want.view(torch.int16)))
                compare(rec, "streamed", "chain", "streamed_faster_beyond_spread")
                rec["streamed_max_diff"] = (streamed().float() - want.float()).abs().max().item()
                del want
                out["cases"].append(rec)
                print(json.dumps(rec), flush=True)
                save()
        del q, k, vt

    B, h, T, d = (256, 12, 197, 64) if not args.small else (4, 3, 197, 64)
    q, k, v = (torch.randn(B, h, T, d, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(3))
    att = {"B": B, "heads": h, "T": T, "d": d, "dtype": "bfloat16"}
    iters, warmup = max(3, args.iters // 5), max(1, args.warmup // 5)
    for fmt in FORMATS:
        for causal in (False, True):
            kw = dict(qk_fmt=fmt, p_fmt=fmt, v_fmt=fmt, out_dtype=torch.bfloat16, is_causal=causal, softmax="fused")
            rec = {"iters": iters, "warmup": warmup}
            for impl in ("composed", "flash"):
                rec[impl] = stat(*timed(lambda: mx_attention(q, k, v, impl=impl, **kw), iters, warmup))
            compare(rec, "flash", "composed")
            rec["sdpa_bf16"] = stat(*timed(lambda: F.scaled_dot_product_attention(q, k, v, is_causal=causal), iters, warmup))
            a, b = (mx_attention(q[:8], k[:8], v[:8], impl=impl, **kw) for impl in ("composed", "flash"))
            rec["outputs_equal"] = bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))
            att[f"{fmt}{'_causal' if causal else ''}"] = rec
            print(json.dumps({fmt: rec, "causal": causal}), flush=True)
    out["attention"] = att
    save()
    print("wrote", args.out)


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
        raise SystemExit("tools/bench_mx_flash.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_flash_stream.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
