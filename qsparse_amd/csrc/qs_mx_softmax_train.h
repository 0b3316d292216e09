// The training side of the MX softmax quantizer (include/qsparse_hip.h, "MX two-way softmax quantizer" and "MX softmax backward
// quantizer"): p = softmax(s * scale (+ mask)) as BOTH MX pairs, and the softmax backward ds as both pairs, each from two launches;
// neither u, e, p nor ds ever exists in memory.  The definition of u, E and the row sum is qs_mx_softmax.h's and qs_mx_norm.h's
// (msx_load_u, msx_exp, mxn_add_quads, mxn_fold): nothing of it is restated here.
//
//   mx_softmax_stats_kernel     one WAVE per row (four rows per work-group, no LDS, no barrier): walks 1 and 2 of mx_softmax_quant_kernel
//     -- the maximum m, then e and Z in the header's row-sum order -- and writes m [R] and Z [R]; a row that is NaN as a whole (a NaN,
//     m = +inf, nothing admitted) writes the quiet NaN 0x7fc00000 into both, which is how the launches below know it.  The second walk
//     forms u again from memory (served from the cache).
//   mx_softmax_quant2_kernel    the tile of qs_mx_quant2.h (128 rows of T x 64 columns of S, 256 lanes) per slice, the slice folded into
//     the block index as mx_quant2_batched_kernel does, with p_j = E(u_j - m) / Z as its widen step.  Phase 1 is mx_norm_apply_kernel's
//     lane layout: a lane holds 4 consecutive elements of a row in 8 passes of 16 rows, taken in two groups of 4 passes whose loads --
//     s, the mask, the row's m and Z -- are all issued before the group's first use; a row block of 32 is 8 adjacent lanes.
//   mx_softmax_bwd_rows_kernel  one wave per row: D = sum_j p_j * dp_j in the row-sum order, p formed again from s, m and Z (no
//     maximum walk, no sum of e), written to D [R].
//   mx_softmax_bwd_quant2_kernel  the same tile with ds_j = (p_j * (dp_j - D)) * scale as its widen step, stochastic rounding included:
//     the words are those qs_mx_quant2_batched_v draws for ds [G, T, S] -- stream 0 at index (g T + t) S + j for the row pair, stream 1
//     at (g S + j) T + t for the col pair.
// What follows once a value is a float under a scale -- the block maximum, the encode step, the code stores, the whole of phase 2 --
// is qs_mx_quant2.h's shared functions.  Phase 1 keeps its OWN statement here (mst_load4, mst_tile, mst_emit) and does not call
// qs_mx_quant2.h's mxq2_load4f / mxq2_at / mxq2_emit_row: on them four VEC instantiations of the backward kernel went from 91 - 96 to
// 97 - 103 VGPRs, a wave per SIMD fewer.  No atomics; a null pair skips its phase, a null col pair also the LDS traffic and the barrier
// (kernel-uniform).  VEC = false is the same text with element accesses, each predicated on its own index: any T, S >= 1, any
// element-aligned base.  A causal row loads nothing of s or the mask at or behind its limit.
#pragma once
#include "qs_mx_softmax.h"

namespace qs {

// the first launch of both forward routes: m and Z of every row
template <int XDT, bool VEC>
__global__ __launch_bounds__(kMxq2Threads) void mx_softmax_stats_kernel(const void* __restrict__ s, const float* __restrict__ mask,
                                                                        float* __restrict__ m_out, float* __restrict__ z_out, int64_t R,
                                                                        int64_t T, int64_t S, int64_t mask_rows, float scale, int causal) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMsxRows + (threadIdx.x >> 6);
    if (r >= R) return;                                         // (wave-uniform; the kernel has no barrier)
    const int64_t t = r % T;
    const int64_t L = (causal && t + 1 < S) ? t + 1 : S;        // top-left aligned
    const int64_t sbase = r * S, mbase = (r % mask_rows) * S;
    float u[8];
    float m = __uint_as_float(0xff800000u);
    bool bad = false;
    for (int64_t c0 = 0; c0 < S; c0 += kMxnPass) {              // (wave-uniform trip count)
        msx_load_u<XDT, VEC>(s, mask, sbase, mbase, c0 + lane * 8, L, scale, u);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            bad |= u[j] != u[j];
            m = fmaxf(m, u[j]);                                 // (a NaN is skipped here and kept in `bad`)
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    const bool rownan = __any((int)bad) || mx_abs_bits(m) >= 0x7f800000u;
    float pa = 0.0f, pb = 0.0f;
    for (int64_t c0 = 0; c0 < S; c0 += kMxnPass) {
        msx_load_u<XDT, VEC>(s, mask, sbase, mbase, c0 + lane * 8, L, scale, u);
#pragma unroll
        for (int j = 0; j < 8; ++j) u[j] = msx_exp(u[j] - m);
        mxn_add_quads(u, pa, pb);
    }
    const float Z = mxn_fold(pa, pb);
    if (lane == 0) {
        m_out[r] = rownan ? __uint_as_float(0x7fc00000u) : m + 0.0f;          // (a zero maximum of either sign is handed out as +0)
        z_out[r] = rownan ? __uint_as_float(0x7fc00000u) : Z;
    }
}

constexpr int kMstGroup = 4;                                    // passes whose loads are in flight together
constexpr int kMstGroups = kMxnPasses / kMstGroup;              // 2

// the lane's 4 elements [gc, gc + 4) of the row at `base` of x [., C] as float32, those below `lim` <= C of a row that exists; the
// others are +0 and are not loaded.  VEC: C % 4 == 0 and an aligned base, one load of 16 (float32) or 8 bytes
template <int DT, bool VEC>
__device__ __forceinline__ void mst_load4(const void* __restrict__ x, int64_t base, int64_t gc, int64_t lim, bool row, float (&out)[4]) {
    using raw_t = typename Mxq2Raw<DT>::type;
    if constexpr (VEC && DT == QS_F32) {
        u32x4 a = {0u, 0u, 0u, 0u};
        if (row && gc < lim) a = ld16<true>((const u32x4*)((const raw_t*)x + base + gc));
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = __uint_as_float(a[j]);
    } else if constexpr (VEC) {
        u32x2 a = {0u, 0u};
        if (row && gc < lim) a = __builtin_nontemporal_load((const u32x2*)((const raw_t*)x + base + gc));
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = mxq2_widen<DT>((raw_t)(a[j >> 1] >> ((j & 1) * 16)));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = (row && gc + j < lim) ? mxq2_widen<DT>(((const raw_t*)x)[base + gc + j]) : 0.0f;
    }
}

// p of the lane's 4 elements from their s (`v`) and mask (`a`) values and the row's m and Z: the forward's p to the bit.  A row
// whose m is NaN is NaN as a whole
__device__ __forceinline__ void mst_p4(const float (&v)[4], const float (&a)[4], bool has_mask, float scale, int64_t gc, int64_t L,
                                       float m, float Z, float (&p)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float w = v[j] * scale;
        if (has_mask) w = w + a[j];                             // (kernel-uniform; an absent mask is not added)
        const float u = gc + j < L ? w : __uint_as_float(0xff800000u);
        p[j] = m != m ? __uint_as_float(0x7fc00000u) : msx_exp(u - m) / Z;
    }
}

// where the tile of this block lies: slice g, first row and column inside the slice
struct MstTile {
    int64_t g, r0, c0;
};
__device__ __forceinline__ MstTile mst_tile(int tiles, int tiles_c) {
    const unsigned t = blockIdx.x % (unsigned)tiles;
    return MstTile{(int64_t)(blockIdx.x / (unsigned)tiles), (int64_t)(t / (unsigned)tiles_c) * kMxq2Rows,
                   (int64_t)(t % (unsigned)tiles_c) * kMxq2Cols};
}

// one pass's 4 values `y` of row `gr` (tile row `trow`) from column `gc` on: staged for phase 2, and the row pair's scale byte and codes
template <bool VEC, bool SR>
__device__ __forceinline__ void mst_emit(float* tile, int trow, int lcol, const float (&y)[4], MxFormat fr, uint8_t* __restrict__ row_codes,
                                         uint8_t* __restrict__ row_scales, bool stage, int64_t gr, int64_t gc, int64_t T, int64_t S,
                                         int64_t nbc, int row_vec, MxSrKey key, uint64_t base) {
    if (stage)
        *(u32x4*)(tile + trow * kMxq2Cols + lcol) =
            u32x4{__float_as_uint(y[0]), __float_as_uint(y[1]), __float_as_uint(y[2]), __float_as_uint(y[3])};
    if (!row_codes) return;                                     // (kernel-uniform)
    uint32_t am = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t a = mx_abs_bits(y[j]);
        am = a > am ? a : am;
    }
    const MxScale sc = mx_scale(mxq2_block_max<kMxnLpb>(am), fr);
    uint32_t c[4];                                              // (VEC: S % 4 == 0 and gc % 4 == 0: the lane's first index is a multiple of 4)
    mx_encode_run<4, SR, VEC>(y, sc, fr, key, 0u, base + (uint64_t)(gr * S + gc), c);
    if (gr < T && gc < S) {
        if ((threadIdx.x % kMxnLpb) == 0) row_scales[gr * nbc + (gc >> 5)] = (uint8_t)sc.byte;
        mxq2_store_row<4, VEC>(row_codes + gr * S + gc, c, VEC && row_vec, gc, S);
    }
}

// `row_vec`: row_codes is 4-byte aligned, so a lane stores its 4 codes at once; `col_vec`: T % 16 == 0 and col_codes 16-byte aligned,
// so a lane stores its column block as two 16-byte runs (both VEC only; otherwise byte stores).  m and Z are [G T]
template <int XDT, bool VEC>
__global__ __launch_bounds__(kMxq2Threads) void mx_softmax_quant2_kernel(MxFormat fr, MxFormat fc, const void* __restrict__ s,
                                                                         const float* __restrict__ mask, const float* __restrict__ m,
                                                                         const float* __restrict__ Z, uint8_t* __restrict__ row_codes,
                                                                         uint8_t* __restrict__ row_scales, uint8_t* __restrict__ col_codes,
                                                                         uint8_t* __restrict__ col_scales, int64_t T, int64_t S,
                                                                         int64_t mask_rows, float scale, int causal, int tiles, int tiles_c,
                                                                         int row_vec, int col_vec) {
    __shared__ __attribute__((aligned(16))) float tile[kMxq2Rows * kMxq2Cols];
    const MstTile at = mst_tile(tiles, tiles_c);
    const int64_t nbc = (S + QS_MX_BLOCK - 1) / QS_MX_BLOCK, nbr = (T + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    uint8_t* rc = row_codes ? row_codes + at.g * T * S : nullptr;
    uint8_t* rs = row_scales + at.g * T * nbc;
    uint8_t* cc = col_codes ? col_codes + at.g * S * T : nullptr;
    uint8_t* cs = col_scales + at.g * S * nbr;

    const int tid = threadIdx.x;
    const int lrow = tid / kMxnLpr, lcol = (tid % kMxnLpr) * kMxnV;
    const int64_t gc = at.c0 + lcol;
    for (int h = 0; h < kMstGroups; ++h) {                      // (a loop: the group's text, E included, exists once)
        float v[kMstGroup][4], a[kMstGroup][4], rm[kMstGroup], rz[kMstGroup];
#pragma unroll
        for (int q = 0; q < kMstGroup; ++q) {
            const int64_t gr = at.r0 + (h * kMstGroup + q) * kMxnRpp + lrow, r = at.g * T + gr;
            const int64_t L = (causal && gr + 1 < S) ? gr + 1 : S;
            mst_load4<XDT, VEC>(s, r * S, gc, L, gr < T, v[q]);
            if (mask) mst_load4<QS_F32, VEC>(mask, (r % mask_rows) * S, gc, L, gr < T, a[q]);
            rm[q] = gr < T ? m[r] : 0.0f;
            rz[q] = gr < T ? Z[r] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < kMstGroup; ++q) {
            const int trow = (h * kMstGroup + q) * kMxnRpp + lrow;
            const int64_t gr = at.r0 + trow;
            const int64_t L = (causal && gr + 1 < S) ? gr + 1 : S;
            float p[4], y[4];
            mst_p4(v[q], a[q], mask != nullptr, scale, gc, L, rm[q], rz[q], p);
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = (gr < T && gc + j < S) ? p[j] : 0.0f;
            mst_emit<VEC, false>(tile, trow, lcol, y, fr, rc, rs, cc != nullptr, gr, gc, T, S, nbc, row_vec, MxSrKey{0u, 0u}, 0ull);
        }
    }
    if (!cc) return;                                            // (kernel-uniform)
    __syncthreads();
    mxq2_col_phase<QS_F32, VEC, false>(tile, fc, cc, cs, T, S, at.r0, at.c0, nbr, col_vec, MxSrKey{0u, 0u}, 0ull);
}

// D [r] = sum_j p_j * dp_j in the row-sum order; elements behind S are +0
template <int XDT, int DDT, bool VEC>
__global__ __launch_bounds__(kMxq2Threads) void mx_softmax_bwd_rows_kernel(const void* __restrict__ dp, const void* __restrict__ s,
                                                                           const float* __restrict__ mask, const float* __restrict__ m,
                                                                           const float* __restrict__ Z, float* __restrict__ D, int64_t R,
                                                                           int64_t T, int64_t S, int64_t mask_rows, float scale,
                                                                           int causal) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMsxRows + (threadIdx.x >> 6);
    if (r >= R) return;                                         // (wave-uniform; the kernel has no barrier)
    const int64_t t = r % T;
    const int64_t L = (causal && t + 1 < S) ? t + 1 : S;
    const int64_t sbase = r * S, mbase = (r % mask_rows) * S;
    const float rm = m[r], rz = Z[r];
    float pa = 0.0f, pb = 0.0f;
    for (int64_t c0 = 0; c0 < S; c0 += kMxnPass) {              // (wave-uniform trip count)
        float u[8], d[8], tm[8];
        bool in[8];
        msx_load_u<XDT, VEC>(s, mask, sbase, mbase, c0 + lane * 8, L, scale, u);
        mxn_load8<DDT, VEC>(dp, sbase, c0 + lane * 8, S, d, in);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float p = rm != rm ? __uint_as_float(0x7fc00000u) : msx_exp(u[j] - rm) / rz;
            tm[j] = in[j] ? p * d[j] : 0.0f;
        }
        mxn_add_quads(tm, pa, pb);
    }
    const float sum = mxn_fold(pa, pb);
    if (lane == 0) D[r] = sum;
}

// VEC here also means: T % 16 == 0 and col_codes 16-byte aligned where a col pair is asked for (qs_mx_quant2_batched_v's rule), so
// phase 2 stores whole runs and, with SR, draws one Philox call per four codes
template <int XDT, int DDT, bool VEC, bool SR>
__global__ __launch_bounds__(kMxq2Threads) void mx_softmax_bwd_quant2_kernel(MxFormat fr, MxFormat fc, const void* __restrict__ dp,
                                                                             const void* __restrict__ s, const float* __restrict__ mask,
                                                                             const float* __restrict__ m, const float* __restrict__ Z,
                                                                             const float* __restrict__ D, uint8_t* __restrict__ row_codes,
                                                                             uint8_t* __restrict__ row_scales, uint8_t* __restrict__ col_codes,
                                                                             uint8_t* __restrict__ col_scales, int64_t T, int64_t S,
                                                                             int64_t mask_rows, float scale, int causal, int tiles,
                                                                             int tiles_c, int row_vec, MxSr sr) {
    __shared__ __attribute__((aligned(16))) float tile[kMxq2Rows * kMxq2Cols];
    const MstTile at = mst_tile(tiles, tiles_c);
    const int64_t nbc = (S + QS_MX_BLOCK - 1) / QS_MX_BLOCK, nbr = (T + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    uint8_t* rc = row_codes ? row_codes + at.g * T * S : nullptr;
    uint8_t* rs = row_scales + at.g * T * nbc;
    uint8_t* cc = col_codes ? col_codes + at.g * S * T : nullptr;
    uint8_t* cs = col_scales + at.g * S * nbr;
    MxSrKey key = {0u, 0u};
    if constexpr (SR) key = mx_sr_key(sr);
    const uint64_t base = sr.base + (uint64_t)(at.g * T * S);   // the index of the slice's first code in the whole dense output

    const int tid = threadIdx.x;
    const int lrow = tid / kMxnLpr, lcol = (tid % kMxnLpr) * kMxnV;
    const int64_t gc = at.c0 + lcol;
    for (int h = 0; h < kMstGroups; ++h) {                      // (a loop: the group's text, E included, exists once)
        float v[kMstGroup][4], a[kMstGroup][4], g[kMstGroup][4], rm[kMstGroup], rz[kMstGroup], rd[kMstGroup];
#pragma unroll
        for (int q = 0; q < kMstGroup; ++q) {
            const int64_t gr = at.r0 + (h * kMstGroup + q) * kMxnRpp + lrow, r = at.g * T + gr;
            const int64_t L = (causal && gr + 1 < S) ? gr + 1 : S;
            mst_load4<XDT, VEC>(s, r * S, gc, L, gr < T, v[q]);
            if (mask) mst_load4<QS_F32, VEC>(mask, (r % mask_rows) * S, gc, L, gr < T, a[q]);
            mst_load4<DDT, VEC>(dp, r * S, gc, S, gr < T, g[q]);
            rm[q] = gr < T ? m[r] : 0.0f;
            rz[q] = gr < T ? Z[r] : 0.0f;
            rd[q] = gr < T ? D[r] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < kMstGroup; ++q) {
            const int trow = (h * kMstGroup + q) * kMxnRpp + lrow;
            const int64_t gr = at.r0 + trow;
            const int64_t L = (causal && gr + 1 < S) ? gr + 1 : S;
            float p[4], y[4];
            mst_p4(v[q], a[q], mask != nullptr, scale, gc, L, rm[q], rz[q], p);
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = (gr < T && gc + j < S) ? (p[j] * (g[q][j] - rd[q])) * scale : 0.0f;
            mst_emit<VEC, SR>(tile, trow, lcol, y, fr, rc, rs, cc != nullptr, gr, gc, T, S, nbc, row_vec, key, base);
        }
    }
    if (!cc) return;                                            // (kernel-uniform)
    __syncthreads();
    mxq2_col_phase<QS_F32, VEC, SR>(tile, fc, cc, cs, T, S, at.r0, at.c0, nbr, true, key, base);
}

}  // namespace qs
