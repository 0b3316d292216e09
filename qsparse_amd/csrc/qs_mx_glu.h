// Gated (SwiGLU / GeGLU) matrix products on MX codes (include/qsparse_hip.h, "MX gated products"): the dense and the grouped product
// on a weight of 2 H rows whose epilogue multiplies act(gate) by up while both are still accumulators, and writes H columns -- as a
// float tensor or as the MX codes of the next product.
//
// Nothing in the K loop knows about the gate.  The weight's rows are INTERLEAVED in runs of 32 when the layer is built: rows
// [64 q, 64 q + 32) are the gate rows of the hidden units [32 q, 32 q + 32), rows [64 q + 32, 64 q + 64) their up rows.  A wave owns a
// 64-wide column corner of the tile, acc[0..3] of 16 columns each, and acc[h] and acc[2 + h] hold the same (m, r) position in the
// same lane, 32 columns apart (qs_mx_gemm.h: col = lane & 15 is m, row = 4 (lane >> 4) + r is n).  With the interleave that is
// the gate and the up value of ONE hidden unit: act(g) * u is a per-lane operation on registers, and the wave's corner is exactly
// one output block of 32 -- the quantizer's abs-max is the lane's 8 values and two __shfl_xor steps, as in mx_epilogue_codes.
//
// mx_glu_kernel has the tile, the fetch and the K loop of mx_gemm_q_kernel (qs_mx_gemm_q.h) written out, for the reason given
// there; mx_grouped_glu_kernel the decode of MxgmBlock and mx_tile_loop over MxbOperand, as mx_gmm_q_kernel (qs_mx_gmm.h).  `act`
// and the float / codes choice are wave-uniform kernel arguments: 25 x 2 instantiations per kernel, not more.
#pragma once
#include "qs_mx_gmm.h"

namespace qs {

// act(g) of include/qsparse_hip.h, float32 (the tree builds with -ffp-contract=off)
__device__ __forceinline__ float mx_glu_act(float g, int act) {
    if (act == QS_MX_GLU_RELU) return g > 0.0f ? g : (g != g ? g : 0.0f);
    if (act == QS_MX_GLU_SILU) return g / (1.0f + expf(-g));
    return (g * 0.5f) * (1.0f + erff(g * 0.70710678118654752440f));
}

// where the gated epilogue writes: y [M, H] in ydt when codes == nullptr, else codes [M, H] and scales [M, H / 32] in the format f
struct MxGluOut {
    void* __restrict__ y;
    int ydt, y_vec;                // y_vec as mx_y_vec says for H columns
    uint8_t* __restrict__ codes;
    uint8_t* __restrict__ scales;
    int c_vec;                     // as mx_c_vec says for H columns
    MxFormat f;
    void* __restrict__ v;          // PRE only, else nullptr: the pre-activations [M, 2 H] in vdt, interleaved as the product's columns
    int vdt, v_vec;                // v_vec as mx_y_vec says for 2 H columns
};

// The gated epilogue on a wave's 64 (m, from mw) x 64 (n, from nw; nw % 64 == 0) corner of the product [M, 2 H]: bias in float32,
// z = act(g) * u with g from acc[h] and u from acc[2 + h], then either one rounding to ydt and the stores of y [M, H], or the MX
// quantizer of qs_mx.h on the block of 32 hidden columns from nw / 2.  H % 32 == 0, so a corner lies wholly inside 2 H or wholly
// outside, and no block is short.  Rows m >= M and corners at or past 2 H are never written.
// PRE (the training forward, qs_mx_glu_matmul_pre_v): g and u -- accumulator plus bias, what mx_epilogue stores for the same operands --
// also leave, rounded once to o.vdt, as v [M, 2 H]: acc[i] at the columns nw + 16 i + 4 (lane >> 4) + r.  A template parameter and
// instantiations of their own (api_mx_glu_pre.hip, api_mx_gmm_glu_pre.hip), so the kernels without it compile to what they were.
template <bool PRE = false>
__device__ __forceinline__ void mx_epilogue_glu(const f32x4 (&acc)[4][4], const float* __restrict__ bias, int act, const MxGluOut& o,
                                                int64_t M, int64_t H, int64_t mw, int64_t nw, int lane) {
    const bool inside = nw < 2 * H;
    const int64_t c0 = (nw >> 1) + 4 * (lane >> 4);                 // this lane's first hidden column (h = 0, r = 0)
    float bg[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}}, bu[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
    if (bias && inside) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t n = nw + 16 * h + 4 * (lane >> 4) + r;
                bg[h][r] = bias[n], bu[h][r] = bias[n + QS_MX_BLOCK];
            }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t m = mw + 16 * j + (lane & 15);
        float z[2][4];
        [[maybe_unused]] float pre[4][4];                           // PRE: v at the columns of acc[0..3]
        uint32_t am = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float g = bias ? acc[h][j][r] + bg[h][r] : acc[h][j][r];
                const float u = bias ? acc[2 + h][j][r] + bu[h][r] : acc[2 + h][j][r];
                if constexpr (PRE) pre[h][r] = g, pre[2 + h][r] = u;
                z[h][r] = mx_glu_act(g, act) * u;
                const uint32_t a = mx_abs_bits(z[h][r]);
                am = a > am ? a : am;
            }
        if (o.codes) {                                              // (wave-uniform; every lane takes part: before any early exit)
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) {
                const uint32_t v = (uint32_t)__shfl_xor((int)am, off, 64);
                am = v > am ? v : am;
            }
        }
        if (m >= M || !inside) continue;
        if constexpr (PRE) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t n = nw + 16 * i + 4 * (lane >> 4);
                mx_store4(o.v, o.vdt, m * (2 * H) + n, pre[i], n, 2 * H, o.v_vec);
            }
        }
        if (!o.codes) {
#pragma unroll
            for (int h = 0; h < 2; ++h) mx_store4(o.y, o.ydt, m * H + c0 + 16 * h, z[h], c0 + 16 * h, H, o.y_vec);
            continue;
        }
        const MxScale s = mx_scale(am, o.f);
        if ((lane >> 4) == 0) o.scales[m * (H >> 5) + (nw >> 6)] = (uint8_t)s.byte;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint32_t c[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                uint32_t sg;
                const float q = mx_round_abs(z[h][r], s, o.f, sg);
                c[r] = mx_code(q, sg, s, o.f);
            }
            uint8_t* p = o.codes + m * H + c0 + 16 * h;
            if (o.c_vec) {
                *(uint32_t*)p = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) p[r] = (uint8_t)c[r];
            }
        }
    }
}

// N = 2 H is the row count of b; the loop's statements are mx_gemm_q_kernel's
template <int FA, int FB, bool VEC, bool PRE = false>
__global__ __launch_bounds__(kMxgThreads) void mx_glu_kernel(const uint8_t* __restrict__ a_codes, const uint8_t* __restrict__ a_scales,
                                                             const uint8_t* __restrict__ b_codes, const uint8_t* __restrict__ b_scales,
                                                             const float* __restrict__ bias, int act, MxGluOut out, int64_t M, int64_t H,
                                                             int64_t K, int tiles_n) {
    using LA = MxgLds<mxg_bits(FA)>;
    using LB = MxgLds<mxg_bits(FB)>;
    constexpr int kBuf = LA::kBytes + LB::kBytes;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kBuf];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t N = 2 * H;
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

    mx_epilogue_glu<PRE>(acc, bias, act, out, M, H, m0 + wm, n0 + wn, lane);
}

// the decode and the loop of mx_gmm_q_kernel on the weights b [E, 2 H, K]; bias_stride: 0 (one [2 H] bias) or 2 H ([E, 2 H]).  The
// tail rows keep zero accumulators and no bias: act(0) * 0 = +0 for every act -- +0, or code 0 and the scale byte 0 (and v = +0)
template <int FA, int FB, bool VEC, bool PRE = false>
__global__ __launch_bounds__(kMxgThreads) void mx_grouped_glu_kernel(const uint8_t* __restrict__ a_codes, const uint8_t* __restrict__ a_scales,
                                                                     const uint8_t* __restrict__ b_codes, const uint8_t* __restrict__ b_scales,
                                                                     const float* __restrict__ bias, int64_t bias_stride,
                                                                     const int32_t* __restrict__ offs, int act, MxGluOut out, int64_t T, int E,
                                                                     int64_t H, int64_t K, int tiles_n) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxTileLds<FA, FB>];
    const MxgmBlock blk(offs, E, T, tiles_n);
    if (blk.group < 0) return;                                      // (uniform, before any barrier)
    const int tid = threadIdx.x, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int64_t N = 2 * H;
    f32x4 acc[4][4];
    mx_zero(acc);
    const float* gbias = nullptr;
    if (blk.group < E) {
        const int64_t nkb = (K + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
        MxbOperand A(a_codes, a_scales, blk.hi, K, blk.m0, wm, tid);
        MxbOperand B(b_codes + blk.group * N * K, b_scales + blk.group * N * nkb, N, K, blk.n0, wn, tid);
        mx_tile_loop<FA, FB, VEC>(acc, A, B, 0, (K + kMxgK - 1) / kMxgK, lds, tid, wm, wn);
        gbias = bias ? bias + blk.group * bias_stride : nullptr;
    }
    mx_epilogue_glu<PRE>(acc, gbias, act, out, blk.hi, H, blk.m0 + wm, blk.n0 + wn, tid & 63);
}

}  // namespace qs

// ---- host side, shared by api_mx_glu.hip and api_mx_gmm_glu.hip (Args: qs_mx_glu_matmul_args or qs_mx_grouped_glu_matmul_args).
// Internal linkage ---------------------------------------------------------------------------------------------------------------
namespace {

// the gated products' own arguments, all QS_ERR_ARG: H, act, and the output the descriptor names (out_format == -1: y)
template <class Args>
bool mx_glu_args_ok(const Args& a) {
    if (a.H < 0 || a.H % QS_MX_BLOCK != 0 || a.H > INT64_MAX / 2) return false;
    if (a.act != QS_MX_GLU_RELU && a.act != QS_MX_GLU_SILU && a.act != QS_MX_GLU_GELU) return false;
    if (a.out_format == -1) return a.y != nullptr;
    return mx_format_ok(a.out_format) && a.out_codes && a.out_scales;
}

// after them: the float output's dtype and alignment (QS_ERR_DTYPE, QS_ERR_ALIGN), QS_OK for a codes output
template <class Args>
int mx_glu_check_y(const Args& a) {
    if (a.out_format != -1) return QS_OK;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    return (((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 ? QS_ERR_ALIGN : QS_OK;
}

// does an output of `rows` rows share a byte with the `a_bytes` of a_codes or the `b_bytes` (0: there is no weight) of b_codes
template <class Args>
bool mx_glu_overlap(const Args& a, int64_t rows, int64_t a_bytes, int64_t b_bytes) {
    const auto hits = [&](const void* out, int64_t bytes) {
        return mx_overlap(out, bytes, a.a_codes, a_bytes) || (b_bytes > 0 && mx_overlap(out, bytes, a.b_codes, b_bytes));
    };
    if (a.out_format == -1) return hits(a.y, rows * a.H * dt_size(a.ydt));
    return hits(a.out_codes, rows * a.H) || hits(a.out_scales, rows * (a.H / QS_MX_BLOCK));
}

// the pre-activation output of the _pre_v entry points, checked where y is: non-null (QS_ERR_ARG) with the other arguments, then its
// dtype and the alignment of its element
template <class Args>
int mx_glu_check_v(const Args& a) {
    if (!dt_ok(a.vdt)) return QS_ERR_DTYPE;
    return (((uintptr_t)a.v) & (dt_size(a.vdt) - 1)) != 0 ? QS_ERR_ALIGN : QS_OK;
}

// does v [rows, 2 H] share a byte with an input, or with the first output
template <class Args>
bool mx_glu_v_overlap(const Args& a, int64_t rows, int64_t a_bytes, int64_t b_bytes) {
    const int64_t bytes = rows * 2 * a.H * (int64_t)dt_size(a.vdt);
    if (mx_overlap(a.v, bytes, a.a_codes, a_bytes) || (b_bytes > 0 && mx_overlap(a.v, bytes, a.b_codes, b_bytes))) return true;
    if (a.out_format == -1) return mx_overlap(a.v, bytes, a.y, rows * a.H * (int64_t)dt_size(a.ydt));
    return mx_overlap(a.v, bytes, a.out_codes, rows * a.H) || mx_overlap(a.v, bytes, a.out_scales, rows * (a.H / QS_MX_BLOCK));
}

// `pre`: the descriptor's v is an output (the _pre_v entry points); the others never look at it
template <class Args>
qs::MxGluOut mx_glu_out(const Args& a, bool pre = false) {
    qs::MxGluOut o = {};
    if (pre) o.v = a.v, o.vdt = a.vdt, o.v_vec = mx_y_vec(a.v, a.vdt, 2 * a.H);
    if (a.out_format == -1) {
        o.y = a.y, o.ydt = a.ydt, o.y_vec = mx_y_vec(a.y, a.ydt, a.H);
    } else {
        o.codes = a.out_codes, o.scales = a.out_scales, o.c_vec = mx_c_vec(a.out_codes, a.H), o.f = mx_format(a.out_format);
    }
    return o;
}

// the product [M, 2 H] as the checks qs_mx_matmul_v and qs_mx_matmul_q_v share (qs_mx_host.h) read it
struct GluProduct {
    int32_t a_format, b_format;
    const uint8_t *a_codes, *a_scales, *b_codes, *b_scales;
    int64_t M, N, K;
};

// the checks of qs_mx_glu_matmul_v (`pre`: of qs_mx_glu_matmul_pre_v, with v an output) and the kernel it launches for these operands:
// QS_MX_GEMM_ROUTE_*, 0 for an empty product, QS_ERR_*
inline int mx_glu_route(const qs_mx_glu_matmul_args& a, bool pre) {
    if (!mx_glu_args_ok(a) || (pre && !a.v)) return QS_ERR_ARG;
    const GluProduct p = {a.a_format, a.b_format, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.M, 2 * a.H, a.K};
    if (mx_gemm_check_operands(p) != QS_OK) return QS_ERR_ARG;
    int st = mx_glu_check_y(a);
    if (st == QS_OK && pre) st = mx_glu_check_v(a);
    if (st != QS_OK) return st;
    if (a.bias && (((uintptr_t)a.bias) & 3u) != 0) return QS_ERR_ALIGN;
    if (a.M == 0 || a.H == 0) return 0;
    const int route = mx_gemm_sized_route(p);
    if (route < 0) return route;
    if (pre && mx_glu_v_overlap(a, a.M, a.M * a.K, p.N * a.K)) return QS_ERR_ARG;
    return mx_glu_overlap(a, a.M, a.M * a.K, p.N * a.K) ? QS_ERR_ARG : route;
}

template <bool PRE>
int mx_glu_launch(const qs_mx_glu_matmul_args& a, int route) {
    const int tiles_n = (int)mx_tiles(2 * a.H);
    const int64_t grid = mx_tiles(a.M) * tiles_n;
    const MxGluOut out = mx_glu_out(a, PRE);
    return mx_dispatch(a.a_format, a.b_format, route == QS_MX_GEMM_ROUTE_VEC, [&](auto FA, auto FB, auto VEC) {
        hipLaunchKernelGGL((mx_glu_kernel<decltype(FA)::value, decltype(FB)::value, decltype(VEC)::value, PRE>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.bias, (int)a.act, out,
                           a.M, a.H, a.K, tiles_n);
        return launch_status();
    });
}

// the product [T, 2 H] as the checks the grouped products share (qs_mx_gmm.h) read it
struct GluGroupedProduct {
    int32_t a_format, b_format;
    const uint8_t *a_codes, *a_scales, *b_codes, *b_scales;
    int64_t bias_batch_stride;
    const int32_t* offs;
    int64_t T, E, N, K;
};

inline GluGroupedProduct mx_gmm_glu_product(const qs_mx_grouped_glu_matmul_args& a) {
    return {a.a_format, a.b_format, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.bias_batch_stride, a.offs, a.T, a.E, 2 * a.H, a.K};
}

// the checks of qs_mx_grouped_glu_matmul_v (`pre`: of qs_mx_grouped_glu_matmul_pre_v) and the kernel it launches for these operands:
// QS_MX_GEMM_ROUTE_*, 0 for an empty product, QS_ERR_*
inline int mx_gmm_glu_route(const qs_mx_grouped_glu_matmul_args& a, bool pre) {
    if (!mx_glu_args_ok(a) || (pre && !a.v)) return QS_ERR_ARG;
    const GluGroupedProduct p = mx_gmm_glu_product(a);
    if (mx_gmm_check_operands(p) != QS_OK) return QS_ERR_ARG;
    int st = mx_glu_check_y(a);
    if (st == QS_OK && pre) st = mx_glu_check_v(a);
    if (st != QS_OK) return st;
    if ((a.bias && (((uintptr_t)a.bias) & 3u) != 0) || (((uintptr_t)a.offs) & 3u) != 0) return QS_ERR_ALIGN;
    if (a.T == 0 || a.H == 0) return 0;
    const int route = mx_gmm_sized_route(p);
    if (route < 0) return route;
    if (pre && mx_glu_v_overlap(a, a.T, a.T * a.K, a.E * p.N * a.K)) return QS_ERR_ARG;
    return mx_glu_overlap(a, a.T, a.T * a.K, a.E * p.N * a.K) ? QS_ERR_ARG : route;
}

template <bool PRE>
int mx_gmm_glu_launch(const qs_mx_grouped_glu_matmul_args& a, int route) {
    const int tiles_n = (int)mx_tiles(2 * a.H);
    const int64_t grid = mx_gmm_mt_max(mx_gmm_glu_product(a)) * tiles_n;
    const MxGluOut out = mx_glu_out(a, PRE);
    return mx_dispatch(a.a_format, a.b_format, route == QS_MX_GEMM_ROUTE_VEC, [&](auto FA, auto FB, auto VEC) {
        hipLaunchKernelGGL((mx_grouped_glu_kernel<decltype(FA)::value, decltype(FB)::value, decltype(VEC)::value, PRE>),
                           dim3((unsigned)grid), dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.a_codes, a.a_scales, a.b_codes, a.b_scales,
                           a.bias, a.bias_batch_stride, a.offs, (int)a.act, out, a.T, (int)a.E, a.H, a.K, tiles_n);
        return launch_status();
    });
}

}  // namespace
