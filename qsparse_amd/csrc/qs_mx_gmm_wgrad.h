// Weight gradient of the grouped (ragged) matrix product on MX codes (include/qsparse_hip.h, "MX grouped weight gradient"):
// dw[e] [N, K] = dy_e^T x_e, the contraction over the rows of group e -- the RAGGED axis.  Both operands carry their blocks of 32
// along that axis: gt_codes [N, T] and xt_codes [K, T] are the col pairs of the two-way quantizer on dy [T, N] and x [T, K].  The
// boundaries are those of the forward (qs_mx_gmm.h): c_-1 = 0, c_e = min(max(offs[e], c_{e-1}), T), group e the tokens [c_{e-1}, c_e),
// read on the device only.
//
// Definition (normative, the header's).  An empty group gives +0.  Otherwise, with s0 = 128 floor(lo / 128) and s1 = min(T, 128
// ceil(hi / 128)), dw[e] is bit for bit what mx_gemm_kernel (qs_mx_gemm.h) writes for the columns [s0, s1) of the two operands after
// every code outside [lo, hi) was set to byte 0 and every scale byte of a block that does not intersect [lo, hi) to 127.  The kernel
// gets there without a copy: it walks the GLOBAL steps of 128 tokens [lo / 128, ceil(hi / 128)), so each MFMA sees exactly the 128
// codes the plain product sees at step (t - s0 / 128) of the slice, and the operand model below (MxgwOperand) applies the mask where
// the bytes enter registers:
//   fetch    a 16-code piece keeps the bytes whose token lies in [lo, hi) and zeroes the others (two byte counts -> one 128-bit
//            mask per thread and step, the same for the four rows it stages); a piece wholly outside is not loaded at all
//   scales   a block [32 b, 32 b + 32) that does not intersect [lo, hi) is 127 and is not loaded.  A block that STRADDLES a boundary
//            keeps its byte for both groups: a 0xFF there is NaN in both, which is what the quantizer's byte means
// A block wholly outside the group contributes nothing whatever its bytes are: zero codes under the scale 2^0.
//
// Index decode: one work-group per (group, 128 x 128 tile of [N, K]); the host knows the grid, E tiles(N) tiles(K), the group the
// slowest index so that the work-groups of one group, which read the same columns of gt and xt, run together and those stay in L2:
//   block = (e * tiles_m + tile_m) * tiles_n + tile_n          tile_m over N (the product's M), tile_n over K (its N)
// Every work-group walks offs from the front up to ITS group (MxgwBounds): the chunked scalar walk of MxgmBlock -- eight entries per
// round trip to the scalar cache, 32-bit SALU, uniform across the work-group -- without the tile count that one accumulates.  An empty
// group skips the loop as the forward's tail pseudo-group does: its accumulators stay zero and go through the same epilogue.
// No split-K, no atomics, no workspace: every element of dw is stored exactly once, by one work-group.
#pragma once
#include "qs_mx_gmm.h"

namespace qs {

// the tokens [lo, hi) of group e < E
struct MxgwBounds {
    int32_t lo, hi;

    __device__ __forceinline__ MxgwBounds(const int32_t* __restrict__ offs, int E, int64_t T, int e) {
        const int32_t cap = (int32_t)(T < (int64_t)INT32_MAX ? T : (int64_t)INT32_MAX);
        int32_t c = 0;
        lo = hi = 0;
        for (int e0 = 0; e0 <= e; e0 += kMxgmChunk) {
            int32_t v[kMxgmChunk];
#pragma unroll
            for (int i = 0; i < kMxgmChunk; ++i) v[i] = offs[e0 + i < E ? e0 + i : E - 1];
            // all eight in scalar registers here, as in MxgmBlock: one round trip per eight entries
            asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]));
#pragma unroll
            for (int i = 0; i < kMxgmChunk; ++i) {
                int32_t ce = v[i] > c ? v[i] : c;
                ce = ce < cap ? ce : cap;
                const bool hit = e0 + i == e;
                lo = hit ? c : lo, hi = hit ? ce : hi;
                c = ce;
            }
        }
    }
};

// the low `n` bytes of a register as a mask: n <= 0 none, n >= 4 all
__device__ __forceinline__ uint32_t mxgw_low_bytes(int n) {
    return n <= 0 ? 0u : (n >= 4 ? 0xffffffffu : (1u << (8 * n)) - 1u);
}

// the operand (qs_mx_gemm.h, mx_tile_loop) of a row-major matrix `codes` [rows, T] whose contraction runs along T, seen through the
// tokens [lo, hi) of one group: `sbytes` [rows, ceil(T / 32)].  Tile rows start at row0; w is the wave's corner.  0 <= lo < hi <= T
struct MxgwOperand {
    const uint8_t* __restrict__ codes;
    const uint8_t* __restrict__ sbytes;
    int64_t rows, T, ntb, lo, hi;
    int64_t prow, srow;            // the first row this thread stages a piece of, the first row it takes a scale byte of
    int k, kb;                     // this thread's piece inside a step (codes), this lane's block inside a step

    __device__ __forceinline__ MxgwOperand(const uint8_t* codes, const uint8_t* scales, int64_t rows, int64_t T, int64_t lo, int64_t hi,
                                           int64_t row0, int w, int tid)
        : codes(codes), sbytes(scales), rows(rows), T(T), ntb((T + QS_MX_BLOCK - 1) / QS_MX_BLOCK), lo(lo), hi(hi),
          prow(row0 + (tid >> 3)), srow(row0 + w + (tid & 15)), k((tid & 7) * 16), kb((tid & 63) >> 4) {}

    __device__ __forceinline__ void advance() {}

    template <bool VEC>
    __device__ __forceinline__ void fetch(u32x4 (&reg)[4], int64_t step) const {
        const int64_t t0 = step * kMxgK + k;
        // the bytes [a, b) of the piece are tokens of the group; hi <= T, so b also stops at the end of the row
        const int64_t da = lo - t0, db = hi - t0;
        const int a = (int)(da < 0 ? 0 : (da > 16 ? 16 : da)), b = (int)(db < 0 ? 0 : (db > 16 ? 16 : db));
        const bool live = a < b;
        u32x4 m;
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = mxgw_low_bytes(b - 4 * r) & ~mxgw_low_bytes(a - 4 * r);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t row = prow + 32 * i;
            reg[i] = mx_load16<VEC>(codes, row < rows && live, row * T + t0, b) & m;
        }
    }

    __device__ __forceinline__ void scales(uint32_t (&s)[4], int64_t step) const {
        const int64_t blk = step * (kMxgK / QS_MX_BLOCK) + kb, t0 = blk * QS_MX_BLOCK;
        const bool live = t0 < hi && t0 + QS_MX_BLOCK > lo;         // (t0 < hi <= T: the block exists)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = srow + 16 * j;
            s[j] = mx_scale(sbytes, row < rows && live, row * ntb + blk);
        }
    }
};

// gt [N, T] is the product's A (tile rows n of dw), xt [K, T] its B (tile rows k): dw[e] [N, K] is the plain product's y [M, N]
template <int FG, int FX, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_gmm_wgrad_kernel(const uint8_t* __restrict__ gt_codes, const uint8_t* __restrict__ gt_scales,
                                                                   const uint8_t* __restrict__ xt_codes, const uint8_t* __restrict__ xt_scales,
                                                                   const int32_t* __restrict__ offs, void* __restrict__ dw, int ydt, int64_t T,
                                                                   int E, int64_t N, int64_t K, int tiles_m, int tiles_n, int y_vec) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxTileLds<FG, FX>];
    const int tid = threadIdx.x, wave = tid >> 6;
    const unsigned tile_n = blockIdx.x % (unsigned)tiles_n, rest = blockIdx.x / (unsigned)tiles_n;
    const unsigned tile_m = rest % (unsigned)tiles_m, e = rest / (unsigned)tiles_m;
    const int64_t m0 = (int64_t)tile_m * kMxgTile, n0 = (int64_t)tile_n * kMxgTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;          // this wave's 64 x 64 corner of the tile
    const MxgwBounds grp(offs, E, T, (int)e);
    f32x4 acc[4][4];
    mx_zero(acc);
    if (grp.hi > grp.lo) {                                          // (uniform: the barriers of the loop are taken by all or none)
        MxgwOperand A(gt_codes, gt_scales, N, T, grp.lo, grp.hi, m0, wm, tid);
        MxgwOperand B(xt_codes, xt_scales, K, T, grp.lo, grp.hi, n0, wn, tid);
        mx_tile_loop<FG, FX, VEC>(acc, A, B, grp.lo / kMxgK, ((int64_t)grp.hi + kMxgK - 1) / kMxgK, lds, tid, wm, wn);
    }
    mx_epilogue(acc, nullptr, (uint8_t*)dw + (int64_t)e * N * K * (ydt == QS_F32 ? 4 : 2), ydt, N, K, m0 + wm, n0 + wn, tid & 63, y_vec);
}

}  // namespace qs
