// The backward of the RMSNorm / LayerNorm in front of the MX quantizer (include/qsparse_hip.h, "MX norm backward"): from dxhat [R, C],
// the gradient with respect to the norm's output, x and the statistics the forward kept, dx [R, C] in x's dtype and the float32 column
// sums dweight [C], dbias [C].  Three launches, each skipped when nobody reads what it writes:
//
//   mx_norm_bwd_stats_kernel   one WAVE per row, as mx_norm_stats_kernel: c1 = sum(g xhat) / Cf and, in layer mode, c2 = sum(g) / Cf
//     into the workspace.  A lane takes 8 consecutive elements of dxhat, x and weight per pass of 512; both sums go through
//     mxn_add_quads / mxn_fold of qs_mx_norm.h, so their order is the forward's by construction.  One walk over the row.
//   mx_norm_bwd_apply_kernel   the 128 x 64 tile of mx_norm_apply_kernel with its lane layout: a lane holds 4 consecutive elements of
//     a row in 8 passes of 16 rows; the loads of a tile -- dxhat, x (qs_mx_quant2.h's mxq2_load4, the one thing this kernel borrows
//     from the tile's phase 1), and per row rstd, mean, c1, c2 -- are all issued before the first use.  It writes dx (rounded once to x's dtype; with RES, dresidual's tile is one more of those loads and is added to the float32
//     value in front of that rounding) and keeps, per lane and column, the sums of dxhat xhat and of dxhat over its 8
//     rows l, l + 16, .. l + 112 in ascending order: the header's 16 strided partial sums of a row tile.  Those meet in LDS
//     ([2][16][64] float32, one 16-byte store per lane and array: the 16 lanes of a row write 64 consecutive dwords), where the
//     first two waves fold them by the pairwise tree (lane c reads column c of 16 rows: consecutive banks) and store the tile's
//     column sums into the partials [ceil(R / 128), C] of the workspace.  That fold is the kernel's only LDS use and only barrier.
//   mx_norm_bwd_fold_kernel    32 columns per work-group: the 128 strided partial sums over the row tiles of each column in LDS
//     [128][32], then the pairwise tree s = 64 .. 1 -- dweight (blockIdx.y 0) and dbias (1).
// No atomics; the order of every sum is a function of the shape alone, whatever is asked for.  VEC = false is the same text with
// element accesses, each predicated on its own index: any R, C >= 1, any element-aligned base, the same bits.
#pragma once
#include "qs_mx_norm.h"

namespace qs {

// c1 [R] and, with `mean` (kernel-uniform: layer mode), c2 [R]
template <int XDT, int GDT, bool VEC>
__global__ __launch_bounds__(kMxq2Threads) void mx_norm_bwd_stats_kernel(const void* __restrict__ dxhat, const void* __restrict__ x,
                                                                         const float* __restrict__ wt, const float* __restrict__ rstd,
                                                                         const float* __restrict__ mean, float* __restrict__ c1,
                                                                         float* __restrict__ c2, int64_t R, int64_t C) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMxnStatRows + (threadIdx.x >> 6);
    if (r >= R) return;                                         // (wave-uniform; the kernel has no barrier)
    const float rs = rstd[r], mu = mean ? mean[r] : 0.0f;
    float a0 = 0.0f, a1 = 0.0f, b0 = 0.0f, b1 = 0.0f;
    for (int64_t c0 = 0; c0 < C; c0 += kMxnPass) {              // (wave-uniform trip count)
        const int64_t c = c0 + lane * 8;
        float xv[8], gv[8], wv[8];
        bool in[8], unused[8];
        mxn_load8<XDT, VEC>(x, r * C, c, C, xv, in);
        mxn_load8<GDT, VEC>(dxhat, r * C, c, C, gv, unused);
        if (wt) mxn_load8<QS_F32, VEC>(wt, 0, c, C, wv, unused);
        float t1[8], t2[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float xh = xv[j];
            if (mean) xh = xh - mu;
            xh = xh * rs;
            float g = gv[j];
            if (wt) g = g * wv[j];
            t1[j] = in[j] ? g * xh : 0.0f;                      // (the padding is +0 whatever rstd and mean are)
            t2[j] = in[j] ? g : 0.0f;
        }
        mxn_add_quads(t1, a0, a1);
        if (mean) mxn_add_quads(t2, b0, b1);
    }
    const float cf = (float)C;
    const float s1 = mxn_fold(a0, a1) / cf;
    if (lane == 0) c1[r] = s1;
    if (mean) {
        const float s2 = mxn_fold(b0, b1) / cf;
        if (lane == 0) c2[r] = s2;
    }
}

constexpr int kMxnbParts = kMxnRpp;                             // 16 strided partial sums per column of a row tile

// `dx`, `pw`, `pb` are each nullable (kernel-uniform): dx with c1 (and c2 in layer mode), pw / pb the partials of dweight / dbias.
// RES: `dres` [R, C] of x's dtype, the residual stream's gradient, is loaded with the tile's other loads and added to the float32 dx
// in front of its one rounding (it comes with dx); a template flag, so that the instantiations without it keep their registers
template <int XDT, int GDT, bool VEC, bool RES = false>
__global__ __launch_bounds__(kMxq2Threads) void mx_norm_bwd_apply_kernel(const void* __restrict__ dxhat, const void* __restrict__ x,
                                                                         const float* __restrict__ wt, const float* __restrict__ rstd,
                                                                         const float* __restrict__ mean, const float* __restrict__ c1,
                                                                         const float* __restrict__ c2, void* __restrict__ dx,
                                                                         float* __restrict__ pw, float* __restrict__ pb, int64_t R,
                                                                         int64_t C, int tiles_c, const void* __restrict__ dres = nullptr) {
    using xraw_t = typename Mxq2Raw<XDT>::type;
    using graw_t = typename Mxq2Raw<GDT>::type;
    __shared__ __attribute__((aligned(16))) float red[2 * kMxnbParts * kMxq2Cols];

    const int tid = threadIdx.x;
    const int64_t tr = blockIdx.x / tiles_c;
    const int64_t r0 = tr * kMxq2Rows;
    const int64_t c0 = (int64_t)(blockIdx.x % tiles_c) * kMxq2Cols;
    const int lrow = tid / kMxnLpr, lcol = (tid % kMxnLpr) * kMxnV;
    const int64_t gc = c0 + lcol;

    xraw_t xr[kMxnPasses][kMxnV];
    graw_t gr_[kMxnPasses][kMxnV];
    xraw_t rr[RES ? kMxnPasses : 1][kMxnV];
    float rs[kMxnPasses], mu[kMxnPasses], k1[kMxnPasses], k2[kMxnPasses];
#pragma unroll
    for (int p = 0; p < kMxnPasses; ++p) {
        const int64_t gr = r0 + p * kMxnRpp + lrow;
        const bool row_in = gr < R;
        mxq2_load4<XDT, VEC>(x, gr * C + gc, row_in, gc, C, xr[p]);
        mxq2_load4<GDT, VEC>(dxhat, gr * C + gc, row_in, gc, C, gr_[p]);
        if constexpr (RES) mxq2_load4<XDT, VEC>(dres, gr * C + gc, row_in, gc, C, rr[p]);
        rs[p] = row_in ? rstd[gr] : 0.0f;
        mu[p] = (mean && row_in) ? mean[gr] : 0.0f;
        k1[p] = (dx && row_in) ? c1[gr] : 0.0f;
        k2[p] = (dx && mean && row_in) ? c2[gr] : 0.0f;
    }
    float w[kMxnV];
#pragma unroll
    for (int j = 0; j < kMxnV; ++j) w[j] = (wt && gc + j < C) ? wt[gc + j] : 1.0f;

    float aw[kMxnV], ab[kMxnV];
#pragma unroll
    for (int j = 0; j < kMxnV; ++j) aw[j] = ab[j] = 0.0f;
#pragma unroll
    for (int p = 0; p < kMxnPasses; ++p) {
        const int64_t gr = r0 + p * kMxnRpp + lrow;
        float d[kMxnV];
#pragma unroll
        for (int j = 0; j < kMxnV; ++j) {
            const bool in = gr < R && gc + j < C;
            const float gv = mxq2_widen<GDT>(gr_[p][j]);
            float xh = mxq2_widen<XDT>(xr[p][j]);
            if (mean) xh = xh - mu[p];                          // (kernel-uniform, as every `if` on a pointer below)
            xh = xh * rs[p];
            float g = gv;
            if (wt) g = g * w[j];
            float t = g - xh * k1[p];
            if (mean) t = t - k2[p];
            d[j] = rs[p] * t;
            if constexpr (RES) d[j] = d[j] + mxq2_widen<XDT>(rr[p][j]);
            if (pw) aw[j] = aw[j] + (in ? gv * xh : 0.0f);      // (rows and columns outside the tensor are +0)
            if (pb) ab[j] = ab[j] + (in ? gv : 0.0f);
        }
        if (dx && gr < R) {
            const int64_t off = gr * C + gc;
            if constexpr (VEC) {
                if (gc < C) {
                    if constexpr (XDT == QS_F32) {
                        *(u32x4*)((float*)dx + off) =
                            u32x4{__float_as_uint(d[0]), __float_as_uint(d[1]), __float_as_uint(d[2]), __float_as_uint(d[3])};
                    } else if constexpr (XDT == QS_BF16) {
                        *(u32x2*)((uint16_t*)dx + off) = u32x2{f32_to_bf16_bits(d[0]) | (f32_to_bf16_bits(d[1]) << 16),
                                                               f32_to_bf16_bits(d[2]) | (f32_to_bf16_bits(d[3]) << 16)};
                    } else {
                        *(u32x2*)((uint16_t*)dx + off) = u32x2{f32_to_f16_bits(d[0]) | (f32_to_f16_bits(d[1]) << 16),
                                                               f32_to_f16_bits(d[2]) | (f32_to_f16_bits(d[3]) << 16)};
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < kMxnV; ++j)
                    if (gc + j < C) store1<XDT>(dx, off + j, d[j]);
            }
        }
    }
    if (!pw && !pb) return;                                     // (kernel-uniform)

    // ---- the 16 -> 1 fold of the tile's column sums -------------------------------------------------------------------------
    *(u32x4*)(red + lrow * kMxq2Cols + lcol) =
        u32x4{__float_as_uint(aw[0]), __float_as_uint(aw[1]), __float_as_uint(aw[2]), __float_as_uint(aw[3])};
    *(u32x4*)(red + (kMxnbParts + lrow) * kMxq2Cols + lcol) =
        u32x4{__float_as_uint(ab[0]), __float_as_uint(ab[1]), __float_as_uint(ab[2]), __float_as_uint(ab[3])};
    __syncthreads();
    if (tid >= 2 * kMxq2Cols) return;
    const int which = tid / kMxq2Cols, c = tid % kMxq2Cols;     // (wave-uniform: wave 0 folds dweight's sums, wave 1 dbias')
    float* __restrict__ dst = which ? pb : pw;
    if (!dst || c0 + c >= C) return;
    float s[kMxnbParts];
#pragma unroll
    for (int l = 0; l < kMxnbParts; ++l) s[l] = red[(which * kMxnbParts + l) * kMxq2Cols + c];
#pragma unroll
    for (int h = kMxnbParts / 2; h >= 1; h >>= 1) {
#pragma unroll
        for (int l = 0; l < h; ++l) s[l] = s[l] + s[l + h];
    }
    dst[tr * C + c0 + c] = s[0];
}

constexpr int kMxnbFoldCols = 32, kMxnbFoldParts = 128;

// dweight (blockIdx.y 0) / dbias (1) [C] from the partials [T, C]; a null output's blocks return at once
__global__ __launch_bounds__(kMxq2Threads) void mx_norm_bwd_fold_kernel(const float* __restrict__ pw, const float* __restrict__ pb,
                                                                        float* __restrict__ dw, float* __restrict__ db, int64_t T,
                                                                        int64_t C) {
    __shared__ float P[kMxnbFoldParts * kMxnbFoldCols];
    const float* __restrict__ src = blockIdx.y ? pb : pw;
    float* __restrict__ dst = blockIdx.y ? db : dw;
    if (!dst) return;                                           // (uniform over the work-group, in front of every barrier)
    const int tid = threadIdx.x, lc = tid % kMxnbFoldCols;
    const int64_t c = (int64_t)blockIdx.x * kMxnbFoldCols + lc;
    for (int j = tid / kMxnbFoldCols; j < kMxnbFoldParts; j += kMxq2Threads / kMxnbFoldCols) {
        float s = 0.0f;
        if (c < C)
            for (int64_t t = j; t < T; t += kMxnbFoldParts) s = s + src[t * C + c];
        P[j * kMxnbFoldCols + lc] = s;
    }
    __syncthreads();
    for (int h = kMxnbFoldParts / 2; h >= 1; h >>= 1) {
        for (int i = tid; i < h * kMxnbFoldCols; i += kMxq2Threads) P[i] = P[i] + P[i + h * kMxnbFoldCols];
        __syncthreads();
    }
    if (tid < kMxnbFoldCols && c < C) dst[c] = P[tid];
}

}  // namespace qs
