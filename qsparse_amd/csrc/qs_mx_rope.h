// Rotary position embedding (include/qsparse_hip.h, "MX rotary embedding") as a dense call and as the load / widen step of the
// batched two-way MX quantizer's tile (qs_mx_quant2.h).  x holds G = G0 G1 strided slices [R, C], R the sequence length, C the head
// dimension (even, h = C / 2); cos / sin are float32 [R, h], shared by the slices.  For the element at column `col` of row t, with its
// PARTNER xp, its pair index j and `lo` (it is the pair's first element):
//   half layout         lo = col < h    partner at col + h / col - h    j = col (lo) or col - h
//   interleaved layout  lo = col even   partner at col ^ 1              j = col >> 1
//   y = lo ? (x * c) - (xp * s) : (x * c) + (xp * s)        c = cos[t, j], s = sin[t, j] (inverse: -sin[t, j])
// -- the header's y_a and y_b, each float32 operation rounded on its own (__fmul_rn / __fsub_rn / __fadd_rn: never an FMA).
//
// A lane owns V consecutive columns of one row: 16 bytes of x (V = 8 two-byte elements, 4 float32); its first column gc is a multiple
// of V, so it is even and a lane never splits an interleaved pair.
//   VEC    one 16-byte load of x.  Interleaved: the partners are the lane's own registers and its V / 2 pairs read V / 2 consecutive
//          floats of each table (16 bytes for V = 8, 8 for V = 4).  Half: h % V == 0, so the lane lies on one side of h as a whole; it
//          loads the 16 bytes at gc +- h as well -- the same row, predicated exactly like its own -- and V consecutive floats of each
//          table.  Every address is 16-byte aligned (8 for the float32 interleaved tables) by the route's conditions.
//   PLAIN  the same lane mapping with element accesses, each predicated on its own row and column: any even C, any R >= 1, any
//          element-aligned base.  (col < C implies partner < C: C is even.)
// mx_rope_quant2_kernel is mx_quant2_batched_kernel's tile (128 x 64, 256 lanes, the slice folded into the linear block index) with
// this as phase 1: the passes are taken in groups of kRopeGroup whose loads -- x, partner, tables -- are all issued before the first
// use; the rotated float32 values go to a float LDS tile [128][64] (32 KB, as mx_norm_apply_kernel stages its values), the row pair is
// encoded from registers, phase 2 is mxq2_col_phase.  A null col pair skips LDS and the barrier.  The kernel states its loads (a lane's
// V elements, its partners and the tables: rope_load, whose half layout reads every line twice and so loads it plainly), the rotation and
// kRopeGroup; the slice decode (mxq2_at, mxq2_to_slice), the staging store (mxq2_stage) and the row pair of a pass (mxq2_emit_row) are
// qs_mx_quant2.h's.
// mx_rope_kernel is the element-wise form: one lane per V columns, dense output in any of the three dtypes.
#pragma once
#include "qs_mx_quant2.h"

namespace qs {

constexpr int kRopeGroup = 2;                                   // passes whose loads are in flight together

template <int XDT>
struct RopeLane {                                               // what a lane holds of one row before the arithmetic
    static constexpr int V = XDT == QS_F32 ? 4 : 8;
    float x[V], xp[V], c[V], s[V];
    bool in[V];
};

template <int XDT>
__device__ __forceinline__ void rope_unpack(u32x4 a, float (&v)[RopeLane<XDT>::V]) {
    constexpr int V = RopeLane<XDT>::V;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if constexpr (XDT == QS_F32) v[j] = __uint_as_float(a[j]);
        else v[j] = mxq2_widen<XDT>((uint16_t)(a[j >> 1] >> ((j & 1) * 16)));
    }
}

// the loads of the lane at columns gc .. gc + V - 1 of the row that begins at `xrow`, whose table rows begin at `cosr` / `sinr`;
// `row_in`: the row exists.  Nothing is read for an element outside [0, C) or a row that does not exist.
template <int XDT, bool VEC, bool IL>
__device__ __forceinline__ void rope_load(RopeLane<XDT>& L, const void* __restrict__ xrow, const float* __restrict__ cosr,
                                          const float* __restrict__ sinr, int64_t gc, int64_t C, int64_t h, bool row_in) {
    using raw_t = typename Mxq2Raw<XDT>::type;
    constexpr int V = RopeLane<XDT>::V;
    const raw_t* xr = (const raw_t*)xrow;
    if constexpr (VEC) {                                        // (C % V == 0: the lane's V elements are inside or outside together)
        const bool in = row_in && gc < C;
        u32x4 a = {0u, 0u, 0u, 0u};
        if (in) a = ld16<IL>((const u32x4*)(xr + gc));          // (half layout: every line is read twice, so not non-temporal)
        rope_unpack<XDT>(a, L.x);
#pragma unroll
        for (int j = 0; j < V; ++j) L.in[j] = in;
        if constexpr (IL) {
            const int64_t tj = gc >> 1;
            uint32_t cw[V / 2], sw[V / 2];
            if constexpr (V == 8) {
                u32x4 cv = {0u, 0u, 0u, 0u}, sv = {0u, 0u, 0u, 0u};
                if (in) {
                    cv = *(const u32x4*)(cosr + tj);
                    sv = *(const u32x4*)(sinr + tj);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) cw[j] = cv[j], sw[j] = sv[j];
            } else {
                u32x2 cv = {0u, 0u}, sv = {0u, 0u};
                if (in) {
                    cv = *(const u32x2*)(cosr + tj);
                    sv = *(const u32x2*)(sinr + tj);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) cw[j] = cv[j], sw[j] = sv[j];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                L.xp[j] = L.x[j ^ 1];
                L.c[j] = __uint_as_float(cw[j >> 1]);
                L.s[j] = __uint_as_float(sw[j >> 1]);
            }
        } else {                                                // (h % V == 0: the lane lies on one side of h)
            const bool lo = gc < h;
            const int64_t tj = lo ? gc : gc - h;
            u32x4 b = {0u, 0u, 0u, 0u};
            if (in) b = ld16<false>((const u32x4*)(xr + (lo ? gc + h : gc - h)));
            rope_unpack<XDT>(b, L.xp);
#pragma unroll
            for (int q = 0; q < V / 4; ++q) {
                u32x4 cv = {0u, 0u, 0u, 0u}, sv = {0u, 0u, 0u, 0u};
                if (in) {
                    cv = *(const u32x4*)(cosr + tj + 4 * q);
                    sv = *(const u32x4*)(sinr + tj + 4 * q);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    L.c[4 * q + j] = __uint_as_float(cv[j]);
                    L.s[4 * q + j] = __uint_as_float(sv[j]);
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int64_t col = gc + j;
            const bool in = row_in && col < C;
            int64_t pcol, tj;
            if constexpr (IL) {
                pcol = col ^ 1;
                tj = col >> 1;
            } else {
                pcol = col < h ? col + h : col - h;
                tj = col < h ? col : col - h;
            }
            L.in[j] = in;
            L.x[j] = in ? mxq2_widen<XDT>(xr[col]) : 0.0f;
            L.xp[j] = in ? mxq2_widen<XDT>(xr[pcol]) : 0.0f;
            L.c[j] = in ? cosr[tj] : 0.0f;
            L.s[j] = in ? sinr[tj] : 0.0f;
        }
    }
}

// the rotated float32 values of the lane; +0 for an element that does not exist
template <int XDT, bool IL>
__device__ __forceinline__ void rope_rotate(const RopeLane<XDT>& L, int64_t gc, int64_t h, int inverse, float (&y)[RopeLane<XDT>::V]) {
    constexpr int V = RopeLane<XDT>::V;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const bool lo = IL ? (j & 1) == 0 : gc + j < h;        // (gc is even)
        const float s = inverse ? -L.s[j] : L.s[j];
        const float p = __fmul_rn(L.x[j], L.c[j]), q = __fmul_rn(L.xp[j], s);
        const float v = lo ? __fsub_rn(p, q) : __fadd_rn(p, q);
        y[j] = L.in[j] ? v : 0.0f;
    }
}

// The batched two-way quantizer's tile with the rotation as its load / widen step; the block index, the slice bases and phase 2 are
// mx_quant2_batched_kernel's.  `row_vec`: row_codes is aligned to the V bytes a lane stores at once (VEC only; otherwise byte stores).
template <int XDT, bool VEC, bool IL>
__global__ __launch_bounds__(kMxq2Threads) void mx_rope_quant2_kernel(MxFormat fr, MxFormat fc, const void* __restrict__ x,
                                                                      const float* __restrict__ cs, const float* __restrict__ sn,
                                                                      int64_t G1, int64_t sg0, int64_t sg1, int64_t pitch,
                                                                      uint8_t* __restrict__ row_codes, uint8_t* __restrict__ row_scales,
                                                                      uint8_t* __restrict__ col_codes, uint8_t* __restrict__ col_scales,
                                                                      int64_t R, int64_t C, int tiles, int tiles_c, int row_vec,
                                                                      int inverse) {
    using raw_t = typename Mxq2Raw<XDT>::type;
    constexpr int V = RopeLane<XDT>::V;
    constexpr int LPR = kMxq2Cols / V;                          // lanes per tile row
    constexpr int RPP = kMxq2Threads / LPR;                     // tile rows per pass
    constexpr int PASSES = kMxq2Rows / RPP;
    static_assert(PASSES % kRopeGroup == 0, "the passes are taken in whole groups");
    __shared__ __attribute__((aligned(16))) float tile[kMxq2Rows * kMxq2Cols];

    const int tid = threadIdx.x;
    const Mxq2At at = mxq2_at(tiles, tiles_c);
    const int64_t r0 = at.r0, c0 = at.c0;
    const int64_t nbc = (C + QS_MX_BLOCK - 1) / QS_MX_BLOCK, nbr = (R + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    const int64_t h = C >> 1;
    const raw_t* xs = (const raw_t*)x + (at.g / G1) * sg0 + (at.g % G1) * sg1;
    mxq2_to_slice(at.g, R, C, row_codes, row_scales, col_codes, col_scales);

    // ---- phase 1: load, rotate, stage, row pair ------------------------------------------------------------------------------
    const int lrow = tid / LPR, lcol = (tid % LPR) * V;
    const int64_t gc = c0 + lcol;
#pragma unroll
    for (int p0 = 0; p0 < PASSES; p0 += kRopeGroup) {
        RopeLane<XDT> L[kRopeGroup];
#pragma unroll
        for (int q = 0; q < kRopeGroup; ++q) {
            const int64_t gr = r0 + (p0 + q) * RPP + lrow;
            const bool row_in = gr < R;
            const int64_t tr = row_in ? gr : 0;                 // (no address is formed from a row that does not exist)
            rope_load<XDT, VEC, IL>(L[q], xs + tr * pitch, cs + tr * h, sn + tr * h, gc, C, h, row_in);
        }
#pragma unroll
        for (int q = 0; q < kRopeGroup; ++q) {
            const int trow = (p0 + q) * RPP + lrow;
            const int64_t gr = r0 + trow;
            float y[V];
            rope_rotate<XDT, IL>(L[q], gc, h, inverse, y);
            if (col_codes) mxq2_stage<V>(tile, trow, lcol, y);
            if (row_codes)                                      // (kernel-uniform, as col_codes)
                mxq2_emit_row<V, VEC, VEC, false, false>(y, fr, row_codes, row_scales, gr, gc, R, C, nbc, row_vec, MxSrKey{0u, 0u}, 0ull);
        }
    }
    if (!col_codes) return;                                     // (kernel-uniform)
    __syncthreads();
    mxq2_col_phase<QS_F32, VEC, false>(tile, fc, col_codes, col_scales, R, C, r0, c0, nbr, true, MxSrKey{0u, 0u}, 0ull);
}

// The element-wise form: lane i of the grid owns the V columns of group i % CG (CG = ceil(C / V) groups per row) of row (i / CG) % R of
// slice i / (CG R) and writes them to the dense y [G, R, C] in YDT -- on the VEC route as 16-byte stores (one for equal element
// sizes, two for a widening output, one 8-byte store for a narrowing one), else element by element.
template <int XDT, int YDT, bool VEC, bool IL>
__global__ __launch_bounds__(kBlock) void mx_rope_kernel(const void* __restrict__ x, void* __restrict__ yout, const float* __restrict__ cs,
                                                         const float* __restrict__ sn, int64_t G1, int64_t sg0, int64_t sg1,
                                                         int64_t pitch, int64_t R, int64_t C, int64_t CG, int64_t total, int inverse) {
    using raw_t = typename Mxq2Raw<XDT>::type;
    constexpr int V = RopeLane<XDT>::V;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int64_t gc = (i % CG) * V, row = i / CG, gr = row % R, g = row / R, h = C >> 1;
    const raw_t* xs = (const raw_t*)x + (g / G1) * sg0 + (g % G1) * sg1 + gr * pitch;
    RopeLane<XDT> L;
    rope_load<XDT, VEC, IL>(L, xs, cs + gr * h, sn + gr * h, gc, C, h, true);
    float y[V];
    rope_rotate<XDT, IL>(L, gc, h, inverse, y);
    const int64_t o = row * C + gc;                             // (row = g R + gr: the dense output's row)
    if constexpr (VEC) {                                        // (C % V == 0 and y 16-byte aligned: o is a multiple of V)
        if constexpr (YDT == QS_F32) {
#pragma unroll
            for (int j = 0; j < V; j += 4)
                *(u32x4*)((float*)yout + o + j) =
                    u32x4{__float_as_uint(y[j]), __float_as_uint(y[j + 1]), __float_as_uint(y[j + 2]), __float_as_uint(y[j + 3])};
        } else {
            uint32_t w[V / 2];
#pragma unroll
            for (int j = 0; j < V / 2; ++j) {
                if constexpr (YDT == QS_BF16) w[j] = f32_to_bf16_bits(y[2 * j]) | (f32_to_bf16_bits(y[2 * j + 1]) << 16);
                else w[j] = f32_to_f16_bits(y[2 * j]) | (f32_to_f16_bits(y[2 * j + 1]) << 16);
            }
            if constexpr (V == 8) *(u32x4*)((uint16_t*)yout + o) = u32x4{w[0], w[1], w[2], w[3]};
            else *(u32x2*)((uint16_t*)yout + o) = u32x2{w[0], w[1]};
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (L.in[j]) store1<YDT>(yout, o + j, y[j]);
    }
}

}  // namespace qs
