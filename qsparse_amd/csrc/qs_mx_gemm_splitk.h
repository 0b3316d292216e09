// Deterministic split-K of the matrix product on MX codes (include/qsparse_hip.h, "MX matrix product, split along K"): two
// launches, no atomics, no synchronisation between work-groups.
//   mx_gemm_partial_kernel  the tile of mx_gemm_kernel (qs_mx_gemm.h: same fetch / stage / LDS image / 16 MFMAs per step, VEC and !VEC)
//                           on a grid of tiles x slices.  Work-group (slice s, tile) walks the K-steps [s per, min((s + 1) per, steps))
//                           from zero accumulators -- the operation sequence of mx_gemm_kernel on the operands cut to that range of
//                           K, whose float32 accumulators it therefore reproduces bit for bit -- and stores them, unconverted and
//                           without bias, to workspace[s][M][N].
//   mx_gemm_reduce_kernel   y = round_once(((p_0 + p_1) + ... + p_{S-1}) + bias): plain float32 adds in ascending s (the library is
//                           built with -ffp-contract=off and without any fast-math flag, so nothing re-associates them), four
//                           consecutive n per thread, stored by the epilogue's mx_store4.
// Every (m < M, n < N) of every slice is written by exactly one lane of the first launch, so the second reads nothing stale and the
// workspace needs no clearing.  Nothing past slices * M * N floats of the workspace is touched.
// The launch of the reduction (mx_launch_reduce) stands next to its kernel, so this header, alone among the kernel headers, includes
// the host helpers (qs_mx_host.h: cdiv, mx_y_vec; qs_host.h: kMaxGrid, launch_status) and not only qs_mx_gemm.h.
#pragma once
#include "qs_mx_host.h"

namespace qs {

template <int FA, int FB, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_gemm_partial_kernel(const uint8_t* __restrict__ a_codes, const uint8_t* __restrict__ a_scales,
                                                                      const uint8_t* __restrict__ b_codes, const uint8_t* __restrict__ b_scales,
                                                                      float* __restrict__ ws, int64_t M, int64_t N, int64_t K, int tiles_n,
                                                                      int tiles, int64_t per, int ws_vec) {
    using LA = MxgLds<mxg_bits(FA)>;
    using LB = MxgLds<mxg_bits(FB)>;
    constexpr int kBuf = LA::kBytes + LB::kBytes;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kBuf];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // slice-major: the work-groups of one slice are consecutive, as the tiles of the unsplit grid are
    const int slice = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int64_t m0 = (int64_t)(tile / tiles_n) * kMxgTile, n0 = (int64_t)(tile % tiles_n) * kMxgTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int64_t nkb = (K + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    const int64_t steps = (K + kMxgK - 1) / kMxgK;
    const int64_t t0 = slice * per, t1 = t0 + per < steps ? t0 + per : steps;        // t0 < steps: no slice is empty (host)

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    u32x4 ra[4], rb[4];
    uint32_t sa[4], sb[4], sa_next[4], sb_next[4];
    mxg_fetch<VEC>(ra, a_codes, m0, M, K, t0 * kMxgK, tid);
    mxg_fetch<VEC>(rb, b_codes, n0, N, K, t0 * kMxgK, tid);
    mxg_scales(sa, a_scales, m0 + wm, M, nkb, t0 * 4 + (lane >> 4), lane);
    mxg_scales(sb, b_scales, n0 + wn, N, nkb, t0 * 4 + (lane >> 4), lane);
    mxg_stage<mxg_bits(FA)>(lds, ra, tid);
    mxg_stage<mxg_bits(FB)>(lds + LA::kBytes, rb, tid);
    __syncthreads();

    for (int64_t t = t0; t < t1; ++t) {
        const bool more = t + 1 < t1;
        if (more) {
            mxg_fetch<VEC>(ra, a_codes, m0, M, K, (t + 1) * kMxgK, tid);
            mxg_fetch<VEC>(rb, b_codes, n0, N, K, (t + 1) * kMxgK, tid);
            mxg_scales(sa_next, a_scales, m0 + wm, M, nkb, (t + 1) * 4 + (lane >> 4), lane);
            mxg_scales(sb_next, b_scales, n0 + wn, N, nkb, (t + 1) * 4 + (lane >> 4), lane);
        }
        const uint8_t* cur = lds + ((t - t0) & 1) * kBuf;
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
            uint8_t* nxt = lds + ((t + 1 - t0) & 1) * kBuf;
            mxg_stage<mxg_bits(FA)>(nxt, ra, tid);
            mxg_stage<mxg_bits(FB)>(nxt + LA::kBytes, rb, tid);
#pragma unroll
            for (int j = 0; j < 4; ++j) sa[j] = sa_next[j], sb[j] = sb_next[j];
        }
        __syncthreads();
    }

    float* __restrict__ p = ws + (int64_t)slice * M * N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t n = n0 + wn + 16 * i + 4 * (lane >> 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t m = m0 + wm + 16 * j + (lane & 15);
            if (m >= M || n >= N) continue;
            const int64_t e = m * N + n;
            if (ws_vec) {                          // N % 4 == 0 (the workspace is 16-byte aligned): n + 3 < N, aligned store
                *(f32x4*)(p + e) = acc[i][j];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (n + r >= N) break;
                    p[e + r] = acc[i][j][r];
                }
            }
        }
    }
}

// one thread per group of four consecutive n of one row m; `groups_n` = ceil(N / 4) groups per row.  static: api_mx_gemm_splitk.hip and
// api_mx_conv_wgrad.hip both launch it, each from a copy of its own
static __global__ __launch_bounds__(kBlock) void mx_gemm_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ bias,
                                                                 void* __restrict__ y, int ydt, int64_t M, int64_t N, int slices,
                                                                 int64_t groups_n, int ws_vec, int y_vec) {
    const int64_t groups = M * groups_n, plane = M * N;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < groups; q += (int64_t)gridDim.x * kBlock) {
        const int64_t m = q / groups_n, n = (q % groups_n) * 4;
        const int64_t e = m * N + n;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};     // lanes past N: never stored
        for (int s = 0; s < slices; ++s) {
            const float* p = ws + s * plane + e;
            float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (ws_vec) {
                const f32x4 t = *(const f32x4*)p;
                w[0] = t[0], w[1] = t[1], w[2] = t[2], w[3] = t[3];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < N) w[r] = p[r];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = s == 0 ? w[r] : v[r] + w[r];      // p_0 itself, not 0 + p_0: a -0 stays -0
        }
        if (bias) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < N) v[r] = v[r] + bias[n + r];
        }
        mx_store4(y, ydt, e, v, n, N, y_vec);
    }
}

// host: the second launch of a split product, y [M, N] = round_once(sum of the `slices` planes of ws (+ bias)); ws_vec: every row of
// every slice keeps the workspace's 16-byte alignment
static inline int mx_launch_reduce(const float* ws, const float* bias, void* y, int ydt, int64_t M, int64_t N, int slices, hipStream_t stream) {
    const int64_t groups_n = cdiv(N, 4), groups = M * groups_n;
    const int64_t blocks = std::min<int64_t>(cdiv(groups, kBlock), kMaxGrid);       // the kernel strides over the rest
    hipLaunchKernelGGL(mx_gemm_reduce_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, ws, bias, y, ydt, M, N, slices, groups_n,
                       (int)(N % 4 == 0), mx_y_vec(y, ydt, N));
    return launch_status();
}

}  // namespace qs
