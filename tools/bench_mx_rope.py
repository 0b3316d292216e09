#!/usr/bin/env python3
"""Time of the rotary embedding in front of the MX quantizer (`mx_rope_quantize`, `mx_rope`) next to the torch chains it replaces.

    python3 tools/bench_mx_rope.py [--out profiles/mx_rope.json] [--iters 20] [--warmup 3] [--small]

One process, the protocol of tools/bench_mx_softmax_train.py.  Per case and operation: `warmup` launches, then HIP events around `iters`
back-to-back launches, three times, the median kept (all three recorded, `spread` = (max - min) / median).  On bf16 and float32 x
[256 * 12, 197, 64] (ViT-B heads at batch 256; PLAIN with a col pair, T % 16 != 0) and [32 * 32, 2048, 128] (a Llama block; VEC), FP8, both
layouts, with and without the col pair:
  fused   `mx_rope_quantize(x, cos, sin, row_fmt, col_fmt)`
  (a)     the torch-ops definition `mx_rope(..., out_dtype=float32)` (the CPU path's expression, run on the device) followed by
          `mx_quantize_2way_batched`: the same bits
  (b)     the usual user form `x * cos + rotate_half(x) * sin` in x.dtype followed by the same quantizer: other bits, time only
  floor   `mx_quantize_2way_batched(x)` alone on the same tensor: what the new kernel can approach; `ratio_to_floor` is what the
          rotation and the table loads cost
`mx_rope` alone is timed against (a) and (b) without the quantizer.  THE BAR: fused faster than (a) by more than (a)'s own spread
(`faster_beyond_spread`: the slowest fused repetition under the fastest of the chain).  Last, a forward + backward step of
`mx_attention_train(softmax="fused")` on bf16 [256, 12, 197, 64] with `rope=` against rotating q and k by (b) in front of it.  Needs a
GPU: there is no fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_gemm import timed  # noqa: E402

CASES = [(256 * 12, 197, 64), (32 * 32, 2048, 128)]
SMALL_CASES = [(24, 197, 64), (4, 256, 128)]
FMT = "mxfp8_e4m3"


def stat(ms, reps):
    return {"ms": ms, "reps_ms": reps, "spread": (max(reps) - min(reps)) / ms}


def versus(fused, a, b, floor=None):
    rec = {"fused": stat(*fused), "chain_a_definition": stat(*a), "chain_b_user_form": stat(*b), "ratio_to_a": fused[0] / a[0],
           "ratio_to_b": fused[0] / b[0], "faster_beyond_spread": bool(max(fused[1]) < min(a[1]))}
    if floor is not None:
        rec["floor_quantizer_alone"] = stat(*floor)
        rec["ratio_to_floor"] = fused[0] / floor[0]
    return rec


def bench(args):
    import torch
    import qsparse_amd as qs
    from qsparse_amd.mx_rope import _rope_def
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "quantize": [],
           "rope": []}

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    def user_form(x, cos_d, sin_d, interleaved):
        """`x * cos + rotate_half(x) * sin` in x.dtype; cos_d / sin_d are the [T, d] tables in x.dtype a model keeps"""
        if interleaved:
            rot = torch.stack((-x[..., 1::2], x[..., 0::2]), -1).flatten(-2)
        else:
            h = x.shape[-1] // 2
            rot = torch.cat((-x[..., h:], x[..., :h]), -1)
        return x * cos_d + rot * sin_d

    g = torch.Generator(device=dev).manual_seed(0)
    it, wu = args.iters, args.warmup
    for G, T, d in (CASES if not args.small else SMALL_CASES):
        cos, sin = qs.mx_rope_table(T, d, device=dev)
        for dtype in (torch.bfloat16, torch.float32):
            x = torch.randn(G, T, d, device=dev, generator=g).to(dtype)
            for interleaved in (False, True):
                rep = (lambda t: t.repeat_interleave(2, -1)) if interleaved else (lambda t: torch.cat((t, t), -1))
                cos_d, sin_d = rep(cos).to(dtype), rep(sin).to(dtype)
                base = {"shape": [G, T, d], "dtype": str(dtype).replace("torch.", ""), "interleaved": interleaved}
                for col in (None, FMT):
                    fused = timed(lambda: qs.mx_rope_quantize(x, cos, sin, row_fmt=FMT, col_fmt=col, interleaved=interleaved), it, wu)
                    route = qs._hip.mx_rope_quant2_last_route
                    a = timed(lambda: qs.mx_quantize_2way_batched(_rope_def(x.float(), cos, sin, interleaved, False), FMT, col), it, wu)
                    b = timed(lambda: qs.mx_quantize_2way_batched(user_form(x, cos_d, sin_d, interleaved), FMT, col), it, wu)
                    floor = timed(lambda: qs.mx_quantize_2way_batched(x, FMT, col), it, wu)
                    rec = dict(base, col_pair=col is not None, route=route, **versus(fused, a, b, floor))
                    out["quantize"].append(rec)
                    print(json.dumps(rec), flush=True)
                    save()
                fused = timed(lambda: qs.mx_rope(x, cos, sin, interleaved=interleaved), it, wu)
                route = qs._hip.mx_rope_last_route
                a = timed(lambda: _rope_def(x.float(), cos, sin, interleaved, False).to(dtype), it, wu)
                b = timed(lambda: user_form(x, cos_d, sin_d, interleaved), it, wu)
                rec = dict(base, route=route, **versus(fused, a, b))
                out["rope"].append(rec)
                print(json.dumps(rec), flush=True)
                save()
            del x

    # a training step of the fused attention: rope= against rotating q and k by the user form in front of it
    B, H, T, d = (256, 12, 197, 64) if not args.small else (2, 2, 197, 64)
    q, k, v = (torch.randn(B, H, T, d, device=dev, generator=g).bfloat16().requires_grad_(True) for _ in range(3))
    do = torch.randn(B, H, T, d, device=dev, generator=g).bfloat16()
    cos, sin = qs.mx_rope_table(T, d, device=dev)
    cos_d, sin_d = torch.cat((cos, cos), -1).bfloat16(), torch.cat((sin, sin), -1).bfloat16()

    def step(keyword):
        if keyword:
            o = qs.mx_attention_train(q, k, v, softmax="fused", rope=(cos, sin))
        else:
            o = qs.mx_attention_train(user_form(q, cos_d, sin_d, False), user_form(k, cos_d, sin_d, False), v, softmax="fused")
        torch.autograd.grad(o, (q, k, v), do)

    iters, warmup = max(3, it // 4), max(1, wu // 2)
    t = timed(lambda: step(False), iters, warmup)
    f = timed(lambda: step(True), iters, warmup)
    out["attention_train"] = {"shape": [B, H, T, d], "dtype": "bfloat16", "iters": iters, "rope_keyword": stat(*f), "user_form_in_front": stat(*t),
                              "ratio": f[0] / t[0], "faster_beyond_spread": bool(max(f[1]) < min(t[1]))}
    print(json.dumps(out["attention_train"]), flush=True)
    save()
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit whose kernels were measured")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mx_rope.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_rope.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
