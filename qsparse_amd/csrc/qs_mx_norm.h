// RMSNorm / LayerNorm in front of the MX quantizer (include/qsparse_hip.h, "MX normalising quantizer"): x [R, C] leaves as the row
// pair and, optionally, the transposed col pair of y = norm(x) * w (+ b); the float y never exists in memory.  Two launches:
//
//   mx_norm_stats_kernel   one WAVE per row (four rows per work-group, no LDS, no barrier): rstd [R] and, in layer mode, mean [R].
//     A lane takes 8 consecutive elements per pass of 512 (one 16-byte load for two-byte inputs, two for float32, on the VEC route),
//     forms the two quad sums (t0 + t1) + (t2 + t3) and adds them to its two partial sums; the lanes' 128 partial sums are folded by
//     six __shfl_down steps (offsets 32 .. 1) and one last addition -- exactly the order the header defines, which so is a function of
//     C alone.  Layer mode walks the row twice (mean, then the centred squares): the second walk is served from the cache.
//   mx_norm_apply_kernel   the tile of qs_mx_quant2.h (128 rows x 64 columns, 256 lanes) with the normalisation as its widen step.
//     Phase 1, lanes along C: a lane holds 4 consecutive elements of a row (16 bytes of float32, 8 of a two-byte input) in 8 passes
//     of 16 rows whose loads -- x, the row's rstd / mean -- are all issued before the first use; w and b of the lane's 4 columns are
//     loaded once.  A row block of 32 is 8 adjacent lanes: three __shfl_xor steps.  y goes to the float32 LDS tile [128][64] as one
//     16-byte store per lane and pass (the 16 lanes of a row write 64 consecutive dwords: no bank is hit twice per 32-bank phase).
//   Phase 2 is qs_mx_quant2.h's mxq2_col_phase on a float32 tile, with `col_vec` as its run-time store rule: lane (c = tid & 63, b = tid >> 6) walks the 32 rows of a column block, the
//     transposition happens in registers.  Elements outside [R, C] are +0 in the tile, as the quantizer's short last blocks.
// The apply kernel's four-element load is qs_mx_quant2.h's mxq2_load4.  Its staging store and the row pair of a pass stay its OWN text
// and do not call mxq2_stage / mxq2_emit_row: through them the compiler kept 68 - 80 VGPRs in place of 94 - 108, another occupancy
// step, and the calls of tools/bench_mx_norm.py were 1.3 - 2.3 % slower than the parent's.
// The per-element arithmetic of the quantizer is qs_mx.h's; nothing of it is restated here.  No atomics, no workspace beyond rstd /
// mean; a null col pair skips the LDS traffic, the barrier and phase 2 (kernel-uniform).  VEC = false is the same text with element
// accesses, each predicated on its own index: any R, C >= 1, any element-aligned base.  Rounding is to nearest only.
//
//   mx_add_norm_stats_kernel   the add-norm quantizer's first launch ("MX add-norm quantizer"): mx_norm_stats_kernel whose load step
//     takes a lane's 8 elements of x and of residual, adds them in float32, rounds once to residual's dtype, stores that h (one
//     16-byte store for a two-byte h, two for float32, on the VEC route) and hands out the WIDENED ROUNDED values -- the sums, their
//     order and the tail are the same text.  The second launch is mx_norm_apply_kernel on h, unchanged.
#pragma once
#include "qs_mx_quant2.h"

namespace qs {

constexpr int kMxnStatRows = kMxq2Threads / 64;                 // rows per work-group of the stats kernel: one per wave
constexpr int kMxnPass = 64 * 8;                                // elements of a row a wave takes per pass

// the 8 elements [c, c + 8) of the row at `base` as float32 and whether each exists; what does not exist is +0
template <int XDT, bool VEC>
__device__ __forceinline__ void mxn_load8(const void* __restrict__ x, int64_t base, int64_t c, int64_t C, float (&v)[8], bool (&in)[8]) {
    if constexpr (VEC) {                                        // (C % 8 == 0: the 8 are inside or outside together)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[j] = 0.0f;
            in[j] = c < C;
        }
        if (c < C) unpack8<XDT>(load8_raw<XDT, false>(x, (base + c) >> 3), v);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            in[j] = c + j < C;
            v[j] = in[j] ? load1<XDT>(x, base + c + j) : 0.0f;
        }
    }
}

// the header's row sum in two steps, shared with qs_mx_norm_bwd.h so that its order is written once: a pass adds a lane's two quad
// sums to its partial sums `pa` (2 lane) and `pb` (2 lane + 1); the fold is the pairwise tree over the wave's 128, every lane returns it
__device__ __forceinline__ void mxn_add_quads(const float (&t)[8], float& pa, float& pb) {
    pa = pa + ((t[0] + t[1]) + (t[2] + t[3]));
    pb = pb + ((t[4] + t[5]) + (t[6] + t[7]));
}

__device__ __forceinline__ float mxn_fold(float pa, float pb) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {                   // partial j += partial j + 2 off, j < 2 off (the lanes above hold
        pa = pa + __shfl_down(pa, off, 64);                     //  sums nobody reads)
        pb = pb + __shfl_down(pb, off, 64);
    }
    return __shfl(pa + pb, 0, 64);
}

// sum over the row of t_i = v_i (TERM 0), v_i * v_i (1) or (v_i - mu) * (v_i - mu) (2) in the header's order, every lane returns it;
// `load(c, v, in)` hands out the 8 elements [c, c + 8) of the row as float32 and whether each exists -- the only step in which the
// statistics kernels below differ
template <int TERM, class Load>
__device__ __forceinline__ float mxn_row_sum(int64_t C, int lane, float mu, Load load) {
    float pa = 0.0f, pb = 0.0f;                                 // the partial sums 2 lane and 2 lane + 1
    for (int64_t c0 = 0; c0 < C; c0 += kMxnPass) {              // (wave-uniform trip count)
        float v[8];
        bool in[8];
        load(c0 + lane * 8, v, in);
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if constexpr (TERM == 0) t[j] = v[j];
            if constexpr (TERM == 1) t[j] = v[j] * v[j];
            if constexpr (TERM == 2) {
                const float d = v[j] - mu;
                t[j] = in[j] ? d * d : 0.0f;
            }
        }
        mxn_add_quads(t, pa, pb);
    }
    return mxn_fold(pa, pb);
}

// rstd [r] and, with `mean` (kernel-uniform: layer mode), mean [r] of the row `first` hands out; layer mode walks the row twice
// (mean, then the centred squares), the second time through `again`
template <class First, class Again>
__device__ __forceinline__ void mxn_row_stats(float* __restrict__ rstd, float* __restrict__ mean, int64_t r, int64_t C, int lane,
                                              float eps, First first, Again again) {
    const float cf = (float)C;
    float mu = 0.0f, ms;
    if (mean) {
        mu = mxn_row_sum<0>(C, lane, 0.0f, first) / cf;
        ms = mxn_row_sum<2>(C, lane, mu, again) / cf;
    } else {
        ms = mxn_row_sum<1>(C, lane, 0.0f, first) / cf;
    }
    float rs = 1.0f / sqrtf(ms + eps);                          // (both correctly rounded: the build's default for HIP)
    if (mx_abs_bits(ms) >= 0x7f800000u) rs = __uint_as_float(0x7fc00000u);      // a row that is not finite is NaN as a whole
    if (lane == 0) {
        rstd[r] = rs;
        if (mean) mean[r] = mu;
    }
}

template <int XDT, bool VEC>
__global__ __launch_bounds__(kMxq2Threads) void mx_norm_stats_kernel(const void* __restrict__ x, float* __restrict__ rstd,
                                                                     float* __restrict__ mean, int64_t R, int64_t C, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMxnStatRows + (threadIdx.x >> 6);
    if (r >= R) return;                                         // (wave-uniform; the kernel has no barrier)
    auto load = [&](int64_t c, float (&v)[8], bool (&in)[8]) { mxn_load8<XDT, VEC>(x, r * C, c, C, v, in); };
    mxn_row_stats(rstd, mean, r, C, lane, eps, load, load);
}

// ---- the add-norm quantizer's statistics launch (include/qsparse_hip.h, "MX add-norm quantizer") ----------------------------------
// 8 float32 values as the raw registers of a group of DT, each rounded once to nearest-even
template <int DT>
__device__ __forceinline__ Raw8<DT> mxn_pack8(const float (&v)[8]) {
    Raw8<DT> r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (DT == QS_F32) {
            r.a[j] = __float_as_uint(v[j]);
            r.b[j] = __float_as_uint(v[4 + j]);
        } else if constexpr (DT == QS_BF16) {
            r.a[j] = f32_to_bf16_bits(v[2 * j]) | (f32_to_bf16_bits(v[2 * j + 1]) << 16);
        } else {
            r.a[j] = f32_to_f16_bits(v[2 * j]) | (f32_to_f16_bits(v[2 * j + 1]) << 16);
        }
    }
    return r;
}

// the 8 elements [c, c + 8) of the row at `base` of h = round(x + residual), rounded to RDT and widened again, as mxn_load8 hands out
// x's; STORE: they are also written to `h` (plain stores: the quantizing launch reads them next).  What does not exist is +0.
template <int XDT, int RDT, bool VEC, bool STORE>
__device__ __forceinline__ void mxn_add_load8(const void* __restrict__ x, const void* __restrict__ res, void* __restrict__ h,
                                              int64_t base, int64_t c, int64_t C, float (&v)[8], bool (&in)[8]) {
    float a[8], b[8];
    bool unused[8];
    mxn_load8<XDT, VEC>(x, base, c, C, a, in);
    mxn_load8<RDT, VEC>(res, base, c, C, b, unused);
    if constexpr (VEC) {                                        // (C % 8 == 0: the 8 are inside or outside together)
        float s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = a[j] + b[j];
        const Raw8<RDT> raw = mxn_pack8<RDT>(s);
        unpack8<RDT>(raw, v);
        if constexpr (STORE) {
            if (c < C) {
                const int64_t g = (base + c) >> 3;
                if constexpr (RDT == QS_F32) {
                    st16<false>((u32x4*)h + 2 * g, raw.a);
                    st16<false>((u32x4*)h + 2 * g + 1, raw.b);
                } else {
                    st16<false>((u32x4*)h + g, raw.a);
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[j] = round_through<RDT>(a[j] + b[j]);
            if constexpr (STORE) {
                if (in[j]) store1<RDT>(h, base + c + j, v[j]);  // (v is a value of RDT: the store's conversion is exact)
            }
        }
    }
}

// mx_norm_stats_kernel on h = round(x + residual), which it writes: the first walk over the row stores h, layer mode's second forms
// it again from x and residual (served from the cache) and does not read `h` back
template <int XDT, int RDT, bool VEC>
__global__ __launch_bounds__(kMxq2Threads) void mx_add_norm_stats_kernel(const void* __restrict__ x, const void* __restrict__ res,
                                                                         void* __restrict__ h, float* __restrict__ rstd,
                                                                         float* __restrict__ mean, int64_t R, int64_t C, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMxnStatRows + (threadIdx.x >> 6);
    if (r >= R) return;                                         // (wave-uniform; the kernel has no barrier)
    auto first = [&](int64_t c, float (&v)[8], bool (&in)[8]) { mxn_add_load8<XDT, RDT, VEC, true>(x, res, h, r * C, c, C, v, in); };
    auto again = [&](int64_t c, float (&v)[8], bool (&in)[8]) { mxn_add_load8<XDT, RDT, VEC, false>(x, res, h, r * C, c, C, v, in); };
    mxn_row_stats(rstd, mean, r, C, lane, eps, first, again);
}

constexpr int kMxnV = 4;                                        // elements per lane and pass of the apply kernel
constexpr int kMxnLpr = kMxq2Cols / kMxnV;                      // 16 lanes per tile row
constexpr int kMxnLpb = QS_MX_BLOCK / kMxnV;                    // 8 lanes per row block (qs_mx_softmax_train.h's own row pair)
constexpr int kMxnRpp = kMxq2Threads / kMxnLpr;                 // 16 tile rows per pass
constexpr int kMxnPasses = kMxq2Rows / kMxnRpp;                 // 8

// `row_vec`: row_codes is 4-byte aligned, so a lane stores its 4 codes at once; `col_vec`: R % 16 == 0 and col_codes 16-byte aligned,
// so a lane stores its column block as two 16-byte runs (both VEC only; otherwise byte stores)
template <int XDT, bool VEC>
__global__ __launch_bounds__(kMxq2Threads) void mx_norm_apply_kernel(MxFormat fr, MxFormat fc, const void* __restrict__ x,
                                                                     const float* __restrict__ wt, const float* __restrict__ bs,
                                                                     const float* __restrict__ rstd, const float* __restrict__ mean,
                                                                     uint8_t* __restrict__ row_codes, uint8_t* __restrict__ row_scales,
                                                                     uint8_t* __restrict__ col_codes, uint8_t* __restrict__ col_scales,
                                                                     int64_t R, int64_t C, int tiles_c, int row_vec, int col_vec) {
    using raw_t = typename Mxq2Raw<XDT>::type;
    __shared__ __attribute__((aligned(16))) float tile[kMxq2Rows * kMxq2Cols];

    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)(blockIdx.x / tiles_c) * kMxq2Rows;
    const int64_t c0 = (int64_t)(blockIdx.x % tiles_c) * kMxq2Cols;
    const int64_t nbc = (C + QS_MX_BLOCK - 1) / QS_MX_BLOCK, nbr = (R + QS_MX_BLOCK - 1) / QS_MX_BLOCK;

    // ---- phase 1: load, normalise, stage, row pair ---------------------------------------------------------------------------
    const int lrow = tid / kMxnLpr, lcol = (tid % kMxnLpr) * kMxnV;
    const int64_t gc = c0 + lcol;
    raw_t raw[kMxnPasses][kMxnV];
    float rs[kMxnPasses], mu[kMxnPasses];
#pragma unroll
    for (int p = 0; p < kMxnPasses; ++p) {
        const int64_t gr = r0 + p * kMxnRpp + lrow;
        mxq2_load4<XDT, VEC>(x, gr * C + gc, gr < R, gc, C, raw[p]);
        rs[p] = gr < R ? rstd[gr] : 0.0f;
        mu[p] = (mean && gr < R) ? mean[gr] : 0.0f;
    }
    float w[kMxnV], b[kMxnV];
#pragma unroll
    for (int j = 0; j < kMxnV; ++j) {
        w[j] = (wt && gc + j < C) ? wt[gc + j] : 1.0f;
        b[j] = (bs && gc + j < C) ? bs[gc + j] : 0.0f;
    }
#pragma unroll
    for (int p = 0; p < kMxnPasses; ++p) {
        const int64_t gr = r0 + p * kMxnRpp + lrow;
        float y[kMxnV];
        uint32_t am = 0;
#pragma unroll
        for (int j = 0; j < kMxnV; ++j) {
            float v = mxq2_widen<XDT>(raw[p][j]);
            if (mean) v = v - mu[p];                            // (kernel-uniform, as the two below)
            v = v * rs[p];
            if (wt) v = v * w[j];
            if (bs) v = v + b[j];
            y[j] = (gr < R && gc + j < C) ? v : 0.0f;
            const uint32_t a = mx_abs_bits(y[j]);
            am = a > am ? a : am;
        }
        if (col_codes)
            *(u32x4*)(tile + (p * kMxnRpp + lrow) * kMxq2Cols + lcol) =
                u32x4{__float_as_uint(y[0]), __float_as_uint(y[1]), __float_as_uint(y[2]), __float_as_uint(y[3])};
        const MxScale s = mx_scale(mxq2_block_max<kMxnLpb>(am), fr);
        uint32_t c[kMxnV];
        mx_encode_run<kMxnV, false, false>(y, s, fr, MxSrKey{0u, 0u}, 0u, 0ull, c);
        if (gr < R && gc < C) {
            if ((tid % kMxnLpb) == 0) row_scales[gr * nbc + (gc >> 5)] = (uint8_t)s.byte;
            mxq2_store_row<kMxnV, VEC>(row_codes + gr * C + gc, c, VEC && row_vec, gc, C);
        }
    }
    if (!col_codes) return;                                     // (kernel-uniform)
    __syncthreads();
    mxq2_col_phase<QS_F32, VEC, false>(tile, fc, col_codes, col_scales, R, C, r0, c0, nbr, col_vec, MxSrKey{0u, 0u}, 0ull);
}

}  // namespace qs
