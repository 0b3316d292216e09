#!/usr/bin/env python3
"""Time of `mx_grouped_matmul` (the ragged block-scaled MFMA kernel on MX codes, group boundaries on the device) next to the ways to
get the same products without it.

    python3 tools/bench_mx_grouped.py [--out profiles/mx_grouped.json] [--iters 50] [--warmup 10] [--small]

One process.  Per case and operation: `warmup` launches, then HIP events around `iters` back-to-back launches, three times, the
median kept (all three recorded).  Cases, all rows x K x N = 8192 x 1024 x 4096: E = 8 balanced; E = 8 skewed, half the rows in one
group; E = 64 with 128 rows per group; E = 64 with random sizes, every eighth group empty.  Formats FP8 E4M3 x FP8 E4M3, FP4 x FP4
and FP8 E4M3 x FP6 E2M3; float32 output.  On the same values, in the same process, all from code that exists without the kernel:
  (a)  the loop of `mx_matmul` over the groups that have rows, the sizes ALREADY on the host, the results kept
  (a+) the same loop after the `offs.tolist()` a caller really needs to get the sizes: a device-to-host copy and a synchronisation per
       call.  THE BAR: mx_grouped_matmul faster than (a+) on every case, and faster than (a) at E = 64
  (b)  `mx_bmm` on operands padded to the largest group; the pad copy (a gather of codes and scales through a precomputed row index)
       is timed separately and `mx_bmm` alone
  (c)  float32 dense products on the de-quantized operands, group by group.  The bf16 form is NOT run: SKIP_BF16 says why
then the cost of the index decode: all rows in the FIRST of E groups against all rows in the LAST one (the same tiles and the same
products; the walk over offs ends at once or runs to its end), E = 8, 64, 1024, at 8192 x 1024 x 512.  Needs a GPU: there is no
fallback.  `--small` shrinks the shapes for a functional rehearsal (its numbers mean nothing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mx_gemm import timed  # noqa: E402

FORMATS = [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4_e2m1", "mxfp4_e2m1"), ("mxfp8_e4m3", "mxfp6_e2m3")]
SKIP_BF16 = ("not run: tools/bench_mx_bmm.py records that bf16 torch.bmm on expert-sized operands ([8, 4096, 1024] x [8, 1024, 4096]) ended in "
             "an illegal memory access on the torch / ROCm build it was measured with, for a cause that was not found; the bf16 product "
             "per group goes through the same library on the same sizes and is left out rather than run into that again")


def sizes_of(kind, E, T):
    import torch
    if kind == "balanced":
        return [T // E] * (E - 1) + [T - T // E * (E - 1)]
    if kind == "skewed":                        # half the rows in group 0
        rest = (T - T // 2) // (E - 1)
        return [T // 2] + [rest] * (E - 2) + [T - T // 2 - rest * (E - 2)]
    w = torch.rand(E, generator=torch.Generator().manual_seed(E))
    w[::8] = 0                                  # every eighth group is empty
    n = (w / w.sum() * T).floor().long().tolist()
    n[-1] += T - sum(n)
    return n


def stat(ms, reps, flop):
    return {"ms": ms, "reps_ms": reps, "tflops": flop / ms * 1e-9, "spread": (max(reps) - min(reps)) / ms}


def bench(args):
    import torch
    from qsparse_amd import _hip, mx_bmm, mx_grouped_matmul, mx_matmul
    from qsparse_amd.quantize import mx_dequantize, quantize_with_mx
    dev = "cuda:0"
    T, K, N = (8192, 1024, 4096) if not args.small else (1024, 256, 256)
    cases = [("balanced", 8), ("skewed", 8), ("balanced", 64), ("random", 64)]
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "iters": args.iters, "warmup": args.warmup, "T": T, "K": K,
           "N": N, "bf16_dense": SKIP_BF16, "cases": []}

    def save():
        with open(args.out, "w") as f:          # (kept current after every case)
            json.dump(out, f, indent=1)
            f.write("\n")

    g = torch.Generator(device=dev).manual_seed(0)
    flop = 2.0 * T * N * K
    x = torch.randn(T, K, device=dev, generator=g, dtype=torch.bfloat16)
    for kind, E in cases:
        sizes = sizes_of(kind, E, T)
        assert sum(sizes) == T and min(sizes) >= 0
        ends = torch.tensor(sizes).cumsum(0)
        bounds = list(zip([0] + ends.tolist(), ends.tolist()))
        offs = ends.to(torch.int32).to(dev)
        w = torch.randn(E, N, K, device=dev, generator=g, dtype=torch.bfloat16)
        for fa, fb in FORMATS:
            _, ac, asc = quantize_with_mx(x, fa, -1, return_codes=True)
            _, bc, bsc = quantize_with_mx(w, fb, -1, return_codes=True)
            rec = {"E": E, "sizes": kind, "largest_group": max(sizes), "empty_groups": sizes.count(0), "a_fmt": fa, "b_fmt": fb}
            ms, reps = timed(lambda: mx_grouped_matmul(ac, asc, fa, bc, bsc, fb, offs), args.iters, args.warmup)
            rec["route"] = _hip.mx_grouped_last_route
            rec["mx_grouped_matmul"] = stat(ms, reps, flop)

            def loop(bounds=bounds):            # (a): keeps the results, as the grouped call's one tensor does
                return [mx_matmul(ac[lo:hi], asc[lo:hi], fa, bc[e], bsc[e], fb) for e, (lo, hi) in enumerate(bounds) if hi > lo]

            def loop_from_device():             # (a+): the sizes come from the device first
                e = offs.tolist()
                return loop(list(zip([0] + e, e)))

            ms_a, reps_a = timed(loop, args.iters, args.warmup)
            rec["matmul_loop"] = stat(ms_a, reps_a, flop)
            ms_p, reps_p = timed(loop_from_device, args.iters, args.warmup)
            rec["matmul_loop_with_tolist"] = stat(ms_p, reps_p, flop)

            # (b): pad every group to the largest one through a row index (row T of the extended operand is zeros)
            cap = max(sizes)
            index = torch.full((E, cap), T, dtype=torch.int64)
            for e, (lo, hi) in enumerate(bounds):
                index[e, :hi - lo] = torch.arange(lo, hi)
            index = index.reshape(-1).to(dev)
            ac_ext, asc_ext = torch.cat([ac, ac.new_zeros(1, K)]), torch.cat([asc, asc.new_full((1, asc.shape[1]), 127)])

            def pad():
                return ac_ext[index].view(E, cap, K), asc_ext[index].view(E, cap, -1)

            ms_c, reps_c = timed(pad, args.iters, args.warmup)
            pc, ps = pad()
            ms_b, reps_b = timed(lambda: mx_bmm(pc, ps, fa, bc, bsc, fb), args.iters, args.warmup)
            rec["padded_bmm"] = dict(stat(ms_b, reps_b, 2.0 * E * cap * N * K), padded_rows=E * cap)
            rec["pad_copy"] = {"ms": ms_c, "reps_ms": reps_c}
            del pc, ps, ac_ext, asc_ext, index

            a32, b32 = mx_dequantize(ac, asc, fa), mx_dequantize(bc, bsc, fb)

            def dense():
                return [a32[lo:hi] @ b32[e].t() for e, (lo, hi) in enumerate(bounds) if hi > lo]

            ms_d, reps_d = timed(dense, args.iters, args.warmup)
            rec["dense_f32_loop"] = stat(ms_d, reps_d, flop)
            del a32, b32
            rec["ratio_to_matmul_loop"], rec["ratio_to_matmul_loop_with_tolist"] = ms / ms_a, ms / ms_p
            rec["ratio_to_padded_bmm_with_pad"], rec["ratio_to_dense_f32_loop"] = ms / (ms_b + ms_c), ms / ms_d
            rec["faster_than_matmul_loop"], rec["faster_than_matmul_loop_with_tolist"] = bool(ms < min(reps_a)), bool(ms < min(reps_p))
            out["cases"].append(rec)
            print(json.dumps(rec), flush=True)
            save()
        del w

    # the decode: the same tiles whether the rows are the first group's or the last one's; only the walk over offs differs
    Nd = 512 if not args.small else 128
    fa, fb = FORMATS[0]
    _, ac, asc = quantize_with_mx(x, fa, -1, return_codes=True)
    out["decode"] = []
    for E in (8, 64, 1024):
        w = torch.randn(E, Nd, K, device=dev, generator=g, dtype=torch.bfloat16)
        _, bc, bsc = quantize_with_mx(w, fb, -1, return_codes=True)
        first = torch.full((E,), T, dtype=torch.int32, device=dev)
        last = torch.zeros(E, dtype=torch.int32, device=dev)
        last[-1] = T
        ms_f, reps_f = timed(lambda: mx_grouped_matmul(ac, asc, fa, bc, bsc, fb, first), args.iters, args.warmup)
        ms_l, reps_l = timed(lambda: mx_grouped_matmul(ac, asc, fa, bc, bsc, fb, last), args.iters, args.warmup)
        rec = {"E": E, "T": T, "N": Nd, "K": K, "work_groups": (T + 127 * (E + 1)) // 128 * -(-Nd // 128),
               "rows_in_first_group": {"ms": ms_f, "reps_ms": reps_f}, "rows_in_last_group": {"ms": ms_l, "reps_ms": reps_l},
               "full_walk_minus_none_us": (ms_l - ms_f) * 1e3}
        out["decode"].append(rec)
        print(json.dumps(rec), flush=True)
        save()
        del w, bc, bsc
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
        raise SystemExit("tools/bench_mx_grouped.py measures on the GPU: none found")
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_grouped.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bench(args)


if __name__ == "__main__":
    main()
