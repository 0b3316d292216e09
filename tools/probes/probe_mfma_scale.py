#!/usr/bin/env python3
"""GPU probe of v_mfma_scale_f32_16x16x128_f8f6f4 (gfx950): one wave, one instruction per problem, exact data.

    hipcc --offload-arch=gfx950 -O2 -shared -fPIC tools/probes/probe_mfma_scale.hip -o tools/probes/libprobe_mfma_scale.so
    python3 tools/probes/probe_mfma_scale.py [--out profiles/mx_mfma_scale_probe.txt]

The host builds the register images, so the packing of the operands is part of what is tested.  HYPOTHESIS (H): D = A . B with
lane l = 16 g + i holding row i of A and column i of B;
  FP6 / FP4: k = 32 g + j, j = 0..31, element j in bits [w j, w j + w) of the lane's operand registers read as one little-endian
             bit string (w = 6 / 4);
  FP8:       registers 0..3 k = 16 g + j, registers 4..7 k = 64 + 16 g + j, j = 0..15, one byte each (a first run of this probe
             with the FP6 / FP4 map assumed for FP8 as well failed on every pair with an FP8 side and passed on the others);
  scale:     byte `opsel` of lane l's scale register is the E8M0 byte of the 32 elements k = 32 g .. 32 g + 31 of row / column i
             (2^(byte - 127)) -- for FP8 these sit in two lanes' registers;
  C / D:     col = l & 15, row = 4 (l >> 4) + register.
Questions: 1 the lane map (random asymmetric data for all 25 format pairs, one-hot sweeps), 2 opsel and the scale's meaning at
0 and 254, 3 scale byte 0xFF, 4 what the accumulation keeps of exact terms spanning more than 24 bits."""
import argparse
import ctypes
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FORMATS = [("fp8_e4m3", 4, 3, 7, 448.0), ("fp8_e5m2", 5, 2, 15, 57344.0), ("fp6_e2m3", 2, 3, 1, 7.5), ("fp6_e3m2", 3, 2, 3, 28.0),
           ("fp4_e2m1", 2, 1, 1, 6.0)]
DEV = "cuda:0"
P, I = ctypes.c_void_p, ctypes.c_int
out_lines = []


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out_lines.append(line)


def table(f):
    """value of every code of format f (float64); codes past the largest normal are marked NaN"""
    _, eb, mb, bias, top = FORMATS[f]
    c = torch.arange(1 << (1 + eb + mb))
    E, M = (c >> mb) & ((1 << eb) - 1), c & ((1 << mb) - 1)
    mag = torch.where(E == 0, M.double() * 2.0 ** (1 - bias - mb), (1 + M.double() * 2.0 ** -mb) * torch.pow(2.0, (E - bias).double()))
    mag = torch.where(mag > top, torch.full_like(mag, float("nan")), mag)
    return torch.where((c >> (eb + mb)) == 1, -mag, mag)


def width(f):
    return 1 + FORMATS[f][1] + FORMATS[f][2]


def code_of(f, value):
    t = table(f)
    return int((t == value).nonzero()[0])


def pack(codes, f):
    """codes [n, 64, 32] (ints) -> register images [n, 64, 8] int32 under (H): element j at bit w * j"""
    w = width(f)
    n = codes.shape[0]
    regs = torch.zeros(n, 64, 8, dtype=torch.int64)
    for j in range(32):
        bit = w * j
        r, s = bit // 32, bit % 32
        v = codes[:, :, j].to(torch.int64) << s
        regs[:, :, r] |= v & 0xFFFFFFFF
        if s + w > 32:
            regs[:, :, r + 1] |= v >> 32
    return (regs - ((regs >> 31) << 32)).to(torch.int32)          # (two's complement image of the unsigned dword)


def place(f, k):
    """(lane group g, element slot j) of k under (H)"""
    if width(f) == 8:
        return (k % 64) // 16, k % 16 + 16 * (k // 64)
    return k // 32, k % 32


def lanes_from_matrix(a, f):
    """a [n, 16, 128] (row or column index, k) -> [n, 64, 32] under (H)"""
    n = a.shape[0]
    if width(f) == 8:
        return a.reshape(n, 16, 2, 4, 16).permute(0, 3, 1, 2, 4).reshape(n, 64, 32)        # [row, half, g, 16] -> [g, row, half, 16]
    return a.reshape(n, 16, 4, 32).permute(0, 2, 1, 3).reshape(n, 64, 32)


def d_to_matrix(d):
    """d [n, 64, 4] -> D [n, 16 rows, 16 cols] under (H): col = l & 15, row = 4 (l >> 4) + reg"""
    n = d.shape[0]
    return d.reshape(n, 4, 16, 4).permute(0, 1, 3, 2).reshape(n, 16, 16)


def run(lib, fa, fb, a, b, sa, sb, c=None, oa=0, ob=0):
    n = a.shape[0]
    c = torch.zeros(n, 64, 4) if c is None else c
    ad, bd, cd = a.contiguous().to(DEV), b.contiguous().to(DEV), c.float().contiguous().to(DEV)
    sad, sbd = sa.to(torch.int32).contiguous().to(DEV), sb.to(torch.int32).contiguous().to(DEV)
    d = torch.empty(n, 64, 4, device=DEV)
    st = lib.probe_mfma_scale(fa, fb, oa, ob, n, ad.data_ptr(), bd.data_ptr(), cd.data_ptr(), sad.data_ptr(), sbd.data_ptr(), d.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    return d.cpu()


def small_codes(f, g, shape, limit):
    """random codes of f whose values are multiples of 0.5 with |value| <= limit"""
    t = table(f)
    ok = (~t.isnan() & (t.abs() <= limit) & (t * 2 == (t * 2).round())).nonzero().reshape(-1)
    return ok[torch.randint(0, len(ok), shape, generator=g)]


def q1_random(lib):
    say("== 1a. hypothesis (H) on random asymmetric data, every format pair, per-lane scales in a window of 4: bit-for-bit vs float64")
    g = torch.Generator().manual_seed(0)
    n = 8
    allok = True
    for fa in range(5):
        for fb in range(5):
            A = small_codes(fa, g, (n, 16, 128), 4.0)
            B = small_codes(fb, g, (n, 16, 128), 4.0)        # B as [col, k]
            sA = torch.randint(125, 129, (n, 16, 4), generator=g)
            sB = torch.randint(125, 129, (n, 16, 4), generator=g)
            va = table(fa)[A] * torch.pow(2.0, (sA - 127).double()).repeat_interleave(32, -1)
            vb = table(fb)[B] * torch.pow(2.0, (sB - 127).double()).repeat_interleave(32, -1)
            want = va @ vb.transpose(1, 2)                   # exact: |terms| <= 2^6, multiples of 2^-6, 128 of them
            d = run(lib, fa, fb, pack(lanes_from_matrix(A, fa), fa), pack(lanes_from_matrix(B, fb), fb),
                    sA.permute(0, 2, 1).reshape(n, 64), sB.permute(0, 2, 1).reshape(n, 64))
            got = d_to_matrix(d).double()
            ok = torch.equal(got, want)
            allok &= ok
            say(f"  A {FORMATS[fa][0]:9s} B {FORMATS[fb][0]:9s}: {'EQUAL' if ok else 'DIFFERENT'}"
                + ("" if ok else f"  ({int((got != want).sum())} of {want.numel()} differ; transposed-D equal: {torch.equal(got.transpose(1, 2), want)})"))
    say("  (H) holds for all 25 pairs" if allok else "  (H) FAILS for at least one pair")


def q1_onehot(lib):
    say("== 1b. one-hot sweeps (value 1.0 in ONE element slot of ONE lane, the other operand 1.0 everywhere, scales 127)")
    for f in (0, 2, 4):
        one = code_of(f, 1.0)
        ones8 = pack(torch.full((1, 64, 32), code_of(0, 1.0)), 0)
        n = 64 * 32
        hot = torch.zeros(n, 64, 32, dtype=torch.int64)
        idx = torch.arange(n)
        hot[idx, idx // 32, idx % 32] = one
        s = torch.full((n, 64), 127)
        for side in ("A", "B"):
            if side == "A":
                d = run(lib, f, 0, pack(hot, f), ones8.expand(n, 64, 8), s, s)
            else:
                d = run(lib, 0, f, ones8.expand(n, 64, 8), pack(hot, f), s, s)
            D = d_to_matrix(d)                                # [n, row, col] if the C/D part of (H) holds
            good = True
            for p in range(n):
                lane = p // 32
                want = torch.zeros(16, 16)
                if side == "A":
                    want[lane & 15, :] = 1.0
                else:
                    want[:, lane & 15] = 1.0
                good &= torch.equal(D[p], want)
            say(f"  {FORMATS[f][0]} on {side}: every (lane, slot) lights exactly {'row' if side == 'A' else 'column'} lane & 15 with 1.0: {good}")
            if not good:
                for p in (0, 1, 31, 32, 17 * 32, 63 * 32 + 31):
                    nz = D[p].nonzero().tolist()
                    say(f"    lane {p // 32} slot {p % 32}: nonzero D (row, col) {nz[:6]}{'...' if len(nz) > 6 else ''} values {sorted(set(D[p][D[p] != 0].tolist()))[:4]}")
    say("== 1c. k pairing: A one-hot at the place (H) gives ka x B one-hot at the place (H) gives kb, row 0 x column 0: D[0][0] != 0 iff ka == kb")
    for fa, fb in ((0, 0), (2, 2), (4, 4), (0, 4), (3, 1)):
        n = 128 * 128
        ka, kb = torch.arange(n) // 128, torch.arange(n) % 128
        A = torch.zeros(n, 64, 32, dtype=torch.int64)
        B = torch.zeros(n, 64, 32, dtype=torch.int64)
        ga, ja = place(fa, ka)
        gb, jb = place(fb, kb)
        A[torch.arange(n), 16 * ga, ja] = code_of(fa, 1.0)
        B[torch.arange(n), 16 * gb, jb] = code_of(fb, 1.0)
        s = torch.full((n, 64), 127)
        d = run(lib, fa, fb, pack(A, fa), pack(B, fb), s, s)
        got = d[:, 0, 0].reshape(128, 128)
        rest = d.clone()
        rest[:, 0, 0] = 0
        say(f"  A {FORMATS[fa][0]} B {FORMATS[fb][0]}: D[0][0] is the 128 x 128 identity: {torch.equal(got, torch.eye(128))}; nothing else written: {not bool(rest.any())}")


def q2_scale(lib):
    say("== 2. opsel and the meaning of the scale byte (FP8 E4M3 both sides; A = 1.0 in lane 0 slot 0, B = 1.0 in lane 0 slot 0: D[0][0] = 2^(sa - 127) 2^(sb - 127))")
    one = code_of(0, 1.0)
    A = torch.zeros(1, 64, 32, dtype=torch.int64)
    A[0, 0, 0] = one
    a = pack(A, 0)
    word = 128 | (130 << 8) | (133 << 16) | (137 << 24)      # bytes 0..3 -> 2^1, 2^3, 2^6, 2^10
    plain = torch.full((1, 64), 127)
    for o in range(4):
        da = run(lib, 0, 0, a, a, torch.full((1, 64), word), plain, oa=o, ob=0)[0, 0, 0].item()
        db = run(lib, 0, 0, a, a, plain, torch.full((1, 64), word), oa=0, ob=o)[0, 0, 0].item()
        say(f"  scale register 0x{word:08x}, opsel {o}: on A D = {da} ; on B D = {db}   (bytes 0..3 would give 2, 8, 64, 1024)")
    for sa, sb in ((0, 254), (254, 0), (0, 127), (1, 127), (127, 0), (254, 127), (127, 254), (254, 128), (0, 0), (200, 190), (64, 60), (254, 254)):
        d = run(lib, 0, 0, a, a, torch.full((1, 64), sa), torch.full((1, 64), sb))[0, 0, 0].item()
        want = 2.0 ** (sa - 127) * 2.0 ** (sb - 127)
        say(f"  sa {sa:3d} sb {sb:3d}: D = {d!r}   2^(sa + sb - 254) = {want!r} (float32: {torch.tensor(want, dtype=torch.float64).float().item()!r})")
    say("  upper bytes of the scale register are ignored with opsel 0:")
    d = run(lib, 0, 0, a, a, torch.full((1, 64), 127 | (0xABCDEF << 8)), plain)[0, 0, 0].item()
    say(f"  scale register 0xabcdef7f: D = {d}")


def q3_ff(lib):
    say("== 3. scale byte 0xFF (lane 0 of A or B holds it; its block is row / column 0, k 0..31)")
    for f in (0, 2, 4):
        one = code_of(f, 1.0)
        ones = pack(torch.full((1, 64, 32), one), f)
        zeros = torch.zeros(1, 64, 8, dtype=torch.int32)
        s_ff = torch.full((1, 64), 127)
        s_ff[0, 0] = 255
        plain = torch.full((1, 64), 127)
        for what, a, b, sa, sb in (("A scale 0xFF, all codes 1.0", ones, ones, s_ff, plain), ("B scale 0xFF, all codes 1.0", ones, ones, plain, s_ff),
                                   ("A scale 0xFF, A codes 0 (as the quantizer writes them), B 1.0", zeros, ones, s_ff, plain),
                                   ("B scale 0xFF, B codes 0, A 1.0", ones, zeros, plain, s_ff),
                                   ("A scale 0xFF, A codes 0, B codes 0", zeros, zeros, s_ff, plain)):
            D = d_to_matrix(run(lib, f, f, a, b, sa, sb))[0]
            nan = D.isnan()
            say(f"  {FORMATS[f][0]}: {what}: NaN rows {sorted(set(nan.nonzero()[:, 0].tolist()))} cols {sorted(set(nan.nonzero()[:, 1].tolist()))} "
                f"count {int(nan.sum())}; other values {sorted(set(D[~nan].tolist()))[:4]}")


def q4_accumulate(lib):
    say("== 4. accumulation (FP8 E4M3; row 0 x column 0; block kb of A carries scale 127 + e[kb]); exact sum vs D[0][0]")
    one = code_of(0, 1.0)

    def case(label, avals, exps, c0=0.0, bvals=None):
        A = torch.zeros(1, 64, 32, dtype=torch.int64)
        B = torch.zeros(1, 64, 32, dtype=torch.int64)
        sa = torch.full((1, 64), 127)
        exact = c0
        for kb in range(4):
            for j, v in enumerate(avals[kb]):
                g, slot = place(0, 32 * kb + j)
                A[0, 16 * g, slot] = code_of(0, float(v))
                B[0, 16 * g, slot] = one
                exact += v * 2.0 ** exps[kb]
            sa[0, 16 * kb] = 127 + exps[kb]
        c = torch.zeros(1, 64, 4)
        c[0, 0, 0] = c0
        d = run(lib, 0, 0, pack(A, 0), pack(B, 0), sa, torch.full((1, 64), 127), c)[0, 0, 0].item()
        rn = torch.tensor(exact, dtype=torch.float64).float().item()
        say(f"  {label}: exact {exact!r}  float32(exact) {rn!r}  D {d!r}  {'= RN(exact)' if d == rn else ('= exact' if d == exact else 'NEITHER')}")

    case("2^24 + 1 (two blocks)", [[1], [1], [], []], [24, 0, 0, 0])
    case("2^24 + 1 + 1 (three blocks)", [[1], [1], [1], []], [24, 0, 0, 0])
    case("2^24 + 1 + 1 + 1 (four blocks)", [[1], [1], [1], [1]], [24, 0, 0, 0])
    case("2^24 + 3 x 1 inside one block of ones after it", [[1], [1, 1, 1], [], []], [24, 0, 0, 0])
    case("2^25 + 32 x 1 (one block of 32 ones)", [[1], [1] * 32, [], []], [25, 0, 0, 0])
    case("2^30 + 96 x 1", [[1], [1] * 32, [1] * 32, [1] * 32], [30, 0, 0, 0])
    case("2^30 - 2^30 + 1 (cancellation across blocks)", [[1], [-1], [1], []], [30, 30, 0, 0])
    case("2^40 - 2^40 + 1", [[1], [-1], [1], []], [40, 40, 0, 0])
    case("C = 2^24, products 1 + 1", [[1], [1], [], []], [0, 0, 0, 0], c0=2.0 ** 24)
    case("C = 2^24, products 4 x 1", [[1], [1], [1], [1]], [0, 0, 0, 0], c0=2.0 ** 24)
    case("C = -2^30, products 2^30 + 1", [[1], [1], [], []], [30, 0, 0, 0], c0=-2.0 ** 30)
    case("1 + 2^-24 (small after large)", [[1], [1], [], []], [0, -24, 0, 0])
    case("1 + 2^-24 + 2^-24", [[1], [1], [1], []], [0, -24, -24, 0])
    case("1.5 * 2^24 + 1 + 1 (tie cases)", [[1.5], [1], [1], []], [24, 0, 0, 0])
    case("same block: 448 * 2^16 + 31 x 2^-9 (within one block)", [[448] + [2.0 ** -9] * 31, [], [], []], [16, 0, 0, 0])


def q4_window(lib):
    say("== 4b. how far below the largest product a term survives (A FP8 E5M2: 2^d at k = 0 and 2^-16, its smallest subnormal, at k = kk;")
    say("       B = 1.0, all scales 127, row 0 x column 0; the exact sum 2^d + 2^-16 is a float32 up to a ratio of 2^23)")
    one = code_of(0, 1.0)
    small = code_of(1, 2.0 ** -16)
    for kk, where in ((1, "same 8 bytes"), (8, "same lane, next 8 bytes"), (16, "same block, the other lane"), (32, "next block"), (64, "same lane, upper registers")):
        kept = []
        ds = list(range(-15, 16))
        A = torch.zeros(len(ds), 64, 32, dtype=torch.int64)
        B = torch.zeros(len(ds), 64, 32, dtype=torch.int64)
        for n, d in enumerate(ds):
            for k, code in ((0, code_of(1, 2.0 ** d)), (kk, small)):
                g, slot = place(1, k)
                A[n, 16 * g, slot] = code
                B[n, 16 * g, slot] = one
        s = torch.full((len(ds), 64), 127)
        out = run(lib, 1, 0, pack(A, 1), pack(B, 0), s, s)[:, 0, 0].double()
        for n, d in enumerate(ds):
            if out[n].item() == 2.0 ** d + 2.0 ** -16:
                kept.append(d + 16)
        lost = [d + 16 for n, d in enumerate(ds) if out[n].item() == 2.0 ** d]
        say(f"  small term at k = {kk:2d} ({where}): kept exactly for ratios 2^r, r in {kept}; dropped entirely for r in {lost}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "mx_mfma_scale_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_mfma_scale.py runs on the GPU: none found")
    lib = ctypes.CDLL(os.path.join(HERE, "libprobe_mfma_scale.so"))
    lib.probe_mfma_scale.argtypes = [I, I, I, I, I, P, P, P, P, P, P, P]
    lib.probe_mfma_scale.restype = I
    say("v_mfma_scale_f32_16x16x128_f8f6f4 on", torch.cuda.get_device_name(0))
    for q in (q1_random, q1_onehot, q2_scale, q3_ff, q4_accumulate, q4_window):
        q(lib)
        with open(args.out, "w") as f:          # (kept current after every section)
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
