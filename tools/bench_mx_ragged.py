#!/usr/bin/env python3
"""Time of one ragged step on the paged MX KV cache -- `mx_kv_append_ragged_paged` + `mx_flash_prefill_ragged_paged`, two launches for
any mix of lengths -- next to the only route the project had before them: the sequences grouped by their `T`, and per group one
`mx_kv_append_paged` and one `mx_flash_prefill_paged`, with the slicing of `v_tail`, `kv_len` and `block_table`, the scatter of `v_tail`
back, and the transposes from the projection's token-major layout to head-major and back INSIDE the timing.

    python3 tools/bench_mx_ragged.py [--out profiles/mx_ragged.json] [--target-ms 100] [--small]

One process.  Per case the operations ALTERNATE (tools/bench_mx_prefill.py's protocol: one untimed launch each, three rounds timed by HIP
events around `iters` back-to-back launches, the median kept and all three recorded with the spread).  `ragged`: the two new launches;
`route`: the comparator whole; `ragged_attn` / `prefill_alone`: the attention launches alone (the comparator's on q codes transposed
outside the timing; only for a uniform batch, where it is one launch).
Operands: Hq / Hkv = 32 / 8, d = dv = 128, bf16 tokens and output, FP8 E4M3, causal, pages of 32 and 128, prefixes of 0 and 4096 keys.
Batches: 63 decodes + one chunk of 512; 32 decodes + four chunks of 256; a uniform 8 x 512.  THE BAR, mixed batches: every repetition of
`ragged` faster than every repetition of `route` (`met`).  Uniform batch: `ragged_attn` no slower than the slowest repetition of
`prefill_alone` -- inside the comparator's spread; the only extra work is the scan.  Both routes' outputs are compared byte for byte
before they are timed.  Needs a GPU: there is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean
nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_flash import stat  # noqa: E402
from bench_mx_prefill import alternate  # noqa: E402

FMT, HQ, HKV, D = "mxfp8_e4m3", 32, 8, 128


def bench(args):
    import torch
    from qsparse_amd import (MXPagedKVCache, mx_flash_prefill_paged, mx_flash_prefill_ragged_paged, mx_kv_append_paged,
                             mx_kv_append_ragged_paged)
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "target_ms": args.target_ms, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    kw = dict(scale=D ** -0.5, is_causal=True, out_dtype=torch.bfloat16)
    batches = {"63x1+512": [1] * 63 + [512], "32x1+4x256": [1] * 32 + [256] * 4, "8x512": [512] * 8}
    prefixes = (0, 4096)
    if args.small:
        batches, prefixes = {"5x1+40": [1] * 5 + [40], "3x40": [40] * 3}, (0, 70)
    for name, Ts in batches.items():
        for prefix in prefixes:
            for page in (32, 128):
                B, Ttot, NP = len(Ts), sum(Ts), -(-(prefix + max(Ts)) // page)
                c = MXPagedKVCache(B * NP, B, NP, HKV, page, D, D, FMT, FMT, device=dev)
                c.block_table[:] = torch.randperm(B * NP, device=dev, generator=g).view(B, NP)
                for pool, hi in ((c.k_pool, 0x78), (c.vt_pool, 0x78), (c.k_pool_scales, 0), (c.vt_pool_scales, 0)):
                    pool.copy_(torch.randint(0, hi, pool.shape, device=dev, generator=g) if hi else
                               torch.randint(118, 124, pool.shape, device=dev, generator=g))        # finite codes, scales near 2^-6
                c.v_tail.normal_(generator=g)
                c.kv_len.fill_(prefix)
                pools = (c.k_pool, c.k_pool_scales, FMT, c.vt_pool, c.vt_pool_scales, FMT)
                k, v, q = (torch.randn(Ttot, h, D, device=dev, generator=g).bfloat16() for h in (HKV, HKV, HQ))
                cu = torch.tensor([0] + Ts, device=dev).cumsum(0).to(torch.int32)
                after = c.kv_len + (cu[1:] - cu[:-1])
                groups = []                                      # per distinct T: (T, its sequences, its flat tokens), known to a scheduler
                for T in sorted(set(Ts)):
                    idx = torch.tensor([b for b, t in enumerate(Ts) if t == T], device=dev)
                    groups.append((T, idx, (cu[idx].long()[:, None] + torch.arange(T, device=dev)).reshape(-1)))

                def ragged():
                    qc = mx_kv_append_ragged_paged(*pools, c.v_tail, c.block_table, c.kv_len, k, v, cu, q_new=q)
                    return mx_flash_prefill_ragged_paged(*qc, FMT, *pools[:2], *pools[3:], c.block_table, after, cu, **kw)

                def route():
                    y = torch.empty(Ttot, HQ, D, dtype=torch.bfloat16, device=dev)
                    for T, idx, tok in groups:
                        kg, vg, qg = (x[tok].view(len(idx), T, -1, D).transpose(1, 2) for x in (k, v, q))
                        tail, table = c.v_tail[idx], c.block_table[idx]
                        qc = mx_kv_append_paged(*pools, tail, table, c.kv_len[idx], kg, vg, q_new=qg)
                        c.v_tail[idx] = tail
                        yg = mx_flash_prefill_paged(*qc, FMT, *pools[:2], *pools[3:], table, after[idx], **kw)
                        y[tok] = yg.transpose(1, 2).reshape(-1, HQ, D)
                    return y

                tail0 = c.v_tail.clone()
                a = ragged()
                tail1 = c.v_tail.clone()
                c.v_tail.copy_(tail0)
                assert torch.equal(a.view(torch.int16), route().view(torch.int16)) and torch.equal(c.v_tail, tail1), "the two routes disagree"
                fns = {"ragged": ragged, "route": route}
                if len(groups) == 1:                             # a uniform batch: the attention launches alone
                    qc = mx_kv_append_ragged_paged(*pools, c.v_tail, c.block_table, c.kv_len, k, v, cu, q_new=q)
                    qh = tuple(x.view(B, Ts[0], HQ, -1).transpose(1, 2).contiguous() for x in qc)
                    fns["ragged_attn"] = lambda: mx_flash_prefill_ragged_paged(*qc, FMT, *pools[:2], *pools[3:], c.block_table, after, cu, **kw)
                    fns["prefill_alone"] = lambda: mx_flash_prefill_paged(*qh, FMT, *pools[:2], *pools[3:], c.block_table, after, **kw)
                res, iters = alternate(fns, args.target_ms)
                rec = {"batch": name, "B": B, "Ttot": Ttot, "prefix": prefix, "page": page, "groups": len(groups), "iters": iters,
                       **{n: stat(*r) for n, r in res.items()}}
                rec["ratio_to_route"] = rec["ragged"]["ms"] / rec["route"]["ms"]
                if len(groups) == 1:
                    rec["ratio_attn_to_prefill_alone"] = rec["ragged_attn"]["ms"] / rec["prefill_alone"]["ms"]
                    rec["met"] = bool(rec["ragged_attn"]["ms"] <= max(rec["prefill_alone"]["reps_ms"]))
                else:
                    rec["met"] = bool(max(rec["ragged"]["reps_ms"]) < min(rec["route"]["reps_ms"]))
                out["cases"].append(rec)
                print(json.dumps(rec), flush=True)
                with open(args.out, "w") as f:                   # (kept current after every case)
                    json.dump(out, f, indent=1)
                    f.write("\n")
                del c, pools
    print("wrote", args.out, "bar met in every case:", all(r["met"] for r in out["cases"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--target-ms", type=float, default=100.0)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit whose kernels were measured")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_ragged.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_ragged.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
