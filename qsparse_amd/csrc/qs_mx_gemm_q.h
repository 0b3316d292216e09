// Matrix product on MX codes that WRITES MX codes (include/qsparse_hip.h, "MX products that write MX codes"): the tile, the fetch and
// the K loop of mx_gemm_kernel (qs_mx_gemm.h), then mx_epilogue_codes instead of the float stores -- bias, optional ReLU and the MX
// quantizer with blocks of 32 along N on the accumulators, while they are still in registers.
//
// The loop is written out a fourth time (after mx_gemm_kernel, mx_gemm_partial_kernel and mx_tile_loop) and not taken from
// mx_tile_loop with a row-major operand: for the float kernel that form measured 2-17 % slower where K is short or the tiles are
// few, and this kernel has the same loop in front of a cheaper store, so the same would show.  The statements are
// mx_gemm_kernel's, which stays untouched: its code objects are the parent's.
#pragma once
#include "qs_mx_gemm.h"

namespace qs {

template <int FA, int FB, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_gemm_q_kernel(const uint8_t* __restrict__ a_codes, const uint8_t* __restrict__ a_scales,
                                                                const uint8_t* __restrict__ b_codes, const uint8_t* __restrict__ b_scales,
                                                                const float* __restrict__ bias, int relu, MxFormat f,
                                                                uint8_t* __restrict__ out_codes, uint8_t* __restrict__ out_scales,
                                                                int64_t M, int64_t N, int64_t K, int tiles_n, int c_vec) {
    using LA = MxgLds<mxg_bits(FA)>;
    using LB = MxgLds<mxg_bits(FB)>;
    constexpr int kBuf = LA::kBytes + LB::kBytes;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kBuf];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * kMxgTile, n0 = (int64_t)(blockIdx.x % tiles_n) * kMxgTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;          // this wave's 64 x 64 corner of the tile
    const int64_t nkb = (K + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    const int64_t steps = (K + kMxgK - 1) / kMxgK;

    f32x4 acc[4][4];                                                // [i: 16 n][j: 16 m]
    mx_zero(acc);

    u32x4 ra[4], rb[4];
    uint32_t sa[4], sb[4], sa_next[4], sb_next[4];
    mxg_fetch<VEC>(ra, a_codes, m0, M, K, 0, tid);
    mxg_fetch<VEC>(rb, b_codes, n0, N, K, 0, tid);
    mxg_scales(sa, a_scales, m0 + wm, M, nkb, lane >> 4, lane);
    mxg_scales(sb, b_scales, n0 + wn, N, nkb, lane >> 4, lane);
    mxg_stage<mxg_bits(FA)>(lds, ra, tid);
    mxg_stage<mxg_bits(FB)>(lds + LA::kBytes, rb, tid);
    __syncthreads();

    for (int64_t t = 0; t < steps; ++t) {
        const bool more = t + 1 < steps;
        if (more) {
            mxg_fetch<VEC>(ra, a_codes, m0, M, K, (t + 1) * kMxgK, tid);
            mxg_fetch<VEC>(rb, b_codes, n0, N, K, (t + 1) * kMxgK, tid);
            mxg_scales(sa_next, a_scales, m0 + wm, M, nkb, (t + 1) * 4 + (lane >> 4), lane);
            mxg_scales(sb_next, b_scales, n0 + wn, N, nkb, (t + 1) * 4 + (lane >> 4), lane);
        }
        const uint8_t* cur = lds + (t & 1) * kBuf;
        i32x8 fa[4], fb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fa[j] = LA::get(cur, wm + 16 * j + (lane & 15), lane >> 4);
            fb[j] = LB::get(cur + LA::kBytes, wn + 16 * j + (lane & 15), lane >> 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[i], fa[j], acc[i][j], FB, FA, 0, (int)sb[i], 0, (int)sa[j]);
        if (more) {
            uint8_t* nxt = lds + ((t + 1) & 1) * kBuf;
            mxg_stage<mxg_bits(FA)>(nxt, ra, tid);
            mxg_stage<mxg_bits(FB)>(nxt + LA::kBytes, rb, tid);
#pragma unroll
            for (int j = 0; j < 4; ++j) sa[j] = sa_next[j], sb[j] = sb_next[j];
        }
        __syncthreads();
    }

    mx_epilogue_codes(acc, bias, relu, f, out_codes, out_scales, M, N, m0 + wm, n0 + wn, lane, c_vec);
}

}  // namespace qs
