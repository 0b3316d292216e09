// The two-way MX quantizer with the GLU derivative in front (include/qsparse_hip.h, "MX gated backward quantizer"): the gradient of
// h = act(g) * u with respect to the interleaved pre-activations v [T, 2 H],
//   dv[m, 64 q + t]      = (d * u) * act'(g)        the gate half
//   dv[m, 64 q + 32 + t] = d * act(g)               the up half          g = v[m, 64 q + t], u = v[m, 64 q + 32 + t], d = dh[m, 32 q + t]
// is computed in registers from ONE read of dh [T, H] and v [T, 2 H] and leaves as the two MX pairs of qs_mx_quant2.h -- row codes
// [T, 2 H] / scales [T, 2 H / 32] and, transposed, col codes [2 H, T] / scales [2 H, ceil(T / 32)].  dv itself is float32, is never
// rounded to a narrower type and never exists in memory.  The per-element arithmetic of the quantizer is qs_mx.h's, act is
// mx_glu_act of qs_mx_glu.h.  This file states the loads' operands and the derivative; the four-element load (mxq2_load4f), the staging
// store (mxq2_stage), the row pair of a pass (mxq2_emit_row) and the whole of phase 2 (mxq2_col_phase) are qs_mx_quant2.h's shared
// functions.
//
// A work-group of 256 lanes owns mxq2_tile's tile, 128 rows x 64 dv columns = the hidden units [32 q, 32 q + 32) of 128 tokens: the
// interleave puts the gate and the up column of a hidden unit into the same tile, 32 columns apart.
//   Phase 1, lanes along H: a lane holds 4 consecutive HIDDEN units of a row -- g, u (two loads of 4 elements of v, 32 columns apart:
//     16 bytes each for a float32 v, 8 for a two-byte one) and d (one load of 4 elements of dh) -- in 128 * 32 / (256 * 4) = 4 passes
//     whose loads are all issued before the first use.  8 lanes cover a tile row, a wave 8 rows.  The lane evaluates act(g) and act'(g)
//     once per hidden unit (they share expf / the sigmoid) and so owns 4 + 4 values of dv: 4 of the row's gate block and 4 of its up
//     block.  A row block of 32 is 8 adjacent lanes: its maximum is three __shfl_xor steps, two blocks per lane and pass.  Both runs of
//     4 go to the float32 LDS tile [128][64] as 16-byte stores: the 8 lanes of a row write 32 consecutive dwords, the 32 banks of
//     a store, so no bank is hit twice.
//   Phase 2 is mxq2_col_phase on a float32 tile (C % 64 == 0, so its column test never binds): lane (c = tid & 63, b = tid >> 6) walks the 32 rows of a column block.
// No atomics, no workspace; a null pair skips its phase, a null col pair also the LDS traffic and the barrier.  VEC = false is the same
// tiling with element loads and byte stores, each predicated on its row: any T >= 1, any element-aligned base (2 H % 64 == 0, so no
// column is ever outside).  SR = true rounds stochastically with the words qs_mx_quant2_v would draw for dv [T, 2 H]: stream 0 at
// index m * 2 H + n for the row pair, stream 1 at n * T + m for the col pair.
#pragma once
#include "qs_mx_glu.h"
#include "qs_mx_quant2.h"

namespace qs {

// act'(g) of include/qsparse_hip.h, float32 without contraction (gelu_grad_factor's one fma is part of its definition)
__device__ __forceinline__ float mx_glu_act_grad(float g, int act) {
    if (act == QS_MX_GLU_RELU) return g > 0.0f ? 1.0f : (g != g ? g : 0.0f);
    if (act == QS_MX_GLU_SILU) {
        const float s = 1.0f / (1.0f + expf(-g));
        return s * (1.0f + g * (1.0f - s));
    }
    return gelu_grad_factor(g);
}

constexpr int kMxgbUnits = 4;                                   // hidden units per lane and pass
constexpr int kMxgbLpr = QS_MX_BLOCK / kMxgbUnits;              // 8 lanes per tile row (and per row block)
constexpr int kMxgbRpp = kMxq2Threads / kMxgbLpr;               // 32 tile rows per pass
constexpr int kMxgbPasses = kMxq2Rows / kMxgbRpp;               // 4

// `row_vec`: row_codes is 4-byte aligned, so a lane stores its 4 codes at once (VEC only; otherwise byte stores)
template <int DDT, int VDT, bool VEC, bool SR>
__global__ __launch_bounds__(kMxq2Threads) void mx_glu_bwd_quant2_kernel(MxFormat fr, MxFormat fc, const void* __restrict__ dh,
                                                                         const void* __restrict__ v, int act,
                                                                         uint8_t* __restrict__ row_codes, uint8_t* __restrict__ row_scales,
                                                                         uint8_t* __restrict__ col_codes, uint8_t* __restrict__ col_scales,
                                                                         int64_t T, int64_t H, int tiles_c, int row_vec, MxSr sr) {
    __shared__ __attribute__((aligned(16))) float tile[kMxq2Rows * kMxq2Cols];

    const int tid = threadIdx.x;
    const int64_t R = T, C = 2 * H;                             // the extents of dv, named as in qs_mx_quant2.h
    const int64_t r0 = (int64_t)(blockIdx.x / tiles_c) * kMxq2Rows;
    const int64_t q = blockIdx.x % tiles_c, c0 = q * kMxq2Cols; // (C % 64 == 0: c0 + 64 <= C)
    const int64_t nbc = C / QS_MX_BLOCK, nbr = (R + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    MxSrKey key = {0u, 0u};
    if constexpr (SR) key = mx_sr_key(sr);

    // ---- phase 1: load, derivative, stage, row pair --------------------------------------------------------------------------
    const int lrow = tid / kMxgbLpr, t0 = (tid % kMxgbLpr) * kMxgbUnits;
    const int64_t gg = c0 + t0, gh = q * QS_MX_BLOCK + t0;      // the lane's first gate column of v / dv and its first hidden unit
    float g[kMxgbPasses][4], u[kMxgbPasses][4], d[kMxgbPasses][4];
#pragma unroll
    for (int p = 0; p < kMxgbPasses; ++p) {                     // (the loads' column tests never bind: C % 64 == 0)
        const int64_t gr = r0 + p * kMxgbRpp + lrow;
        mxq2_load4f<VDT, VEC>(v, gr * C + gg, gr < R, gg, C, g[p]);
        mxq2_load4f<VDT, VEC>(v, gr * C + gg + QS_MX_BLOCK, gr < R, gg + QS_MX_BLOCK, C, u[p]);
        mxq2_load4f<DDT, VEC>(dh, gr * H + gh, gr < R, gh, H, d[p]);
    }
#pragma unroll
    for (int p = 0; p < kMxgbPasses; ++p) {
        const int trow = p * kMxgbRpp + lrow;
        const int64_t gr = r0 + trow;
        float dv[2][4];                                         // [0]: the gate block's columns c0 + t0 .., [1]: the up block's, 32 on
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dv[0][j] = (d[p][j] * u[p][j]) * mx_glu_act_grad(g[p][j], act);
            dv[1][j] = d[p][j] * mx_glu_act(g[p][j], act);
        }
#pragma unroll
        for (int b = 0; b < 2; ++b) {                           // (rows past T hold +0: every input was taken as 0)
            const int64_t gc = gg + b * QS_MX_BLOCK;            // (a multiple of 4, as C and sr.base: one Philox call for the four)
            if (col_codes) mxq2_stage<4>(tile, trow, t0 + b * QS_MX_BLOCK, dv[b]);
            if (row_codes)                                      // (kernel-uniform, as col_codes; FULL: gc + 4 <= C)
                mxq2_emit_row<4, VEC, true, SR, true>(dv[b], fr, row_codes, row_scales, gr, gc, R, C, nbc, row_vec, key,
                                                      sr.base + (uint64_t)(gr * C + gc));
        }
    }
    if (!col_codes) return;                                     // (kernel-uniform)
    __syncthreads();
    mxq2_col_phase<QS_F32, VEC, SR>(tile, fc, col_codes, col_scales, R, C, r0, c0, nbr, true, key, sr.base);
}

}  // namespace qs
