// Transposed 2-d convolution on MX codes (include/qsparse_hip.h, "MX transposed convolution"): y[B, OH, OW, Cout] from channels-last
// codes x [B, H, W, C] and w [Cout, KH, KW, C] with blocks of 32 along C -- also the input gradient of a convolution, whose
// contraction runs over (kh, kw, cout).  It is the implicit GEMM of qs_mx_conv.h with another pixel functor: the product is
// A [M = B OH OW, K'] . Wp [Cout, K']^T with K' = KH KW Cp, Cp = 32 ceil(C / 32), k' = (kh KW + kw) Cp + c and
//   A[m, k'] = x[b, (oh + ph - kh dh) / sh, (ow + pw - kw dw) / sw, c]   where both divisions are exact and the pixel is inside,
//   Wp[n, k'] = w[n, kh, kw, c]   (the weight's own indices, un-flipped)
// zero codes (scale byte 127) everywhere else.  Everything behind the activation's fetch is qs_mx_conv.h's own code: MxgLds /
// mxg_stage, mxc_advance, mxc_products, mxc_epilogue and the weight path (IMG = false) of mxc_fetch / mxc_scales -- so the sum is
// accumulated in the order of mx_gemm_kernel on the host-gathered A and Wp and the result is the same bits.
//
// The pixel functor.  A row keeps (b, nh, nw) = (b, oh + ph, ow + pw), computed once before the K loop.  At tap (kh, kw) the axis
// value is t = nh - kh dh; the tap exists on that axis iff t >= 0, t % sh == 0 and t / sh < H.  There is no hardware division in
// the loop: with m = floor((2^32 - 1) / s) from the host, q = umulhi(t, m) is floor(t / s) or one less for every 0 <= t < 2^31
// (2^32 / s - m <= 1, so t / s - t m / 2^32 <= t / 2^32 < 1 / 2), and one compare-and-step of the remainder t - q s makes both
// exact.  The host checks that oh + ph, ow + pw and (KH - 1) dh, (KW - 1) dw fit 31 bits.  A row past M keeps nh = -1: t < 0 at
// every tap.  No tap is skipped: a piece that does not exist is loaded from a clamped address and replaced by zeros with a select
// (its scale byte by 127), so a 0xFF scale byte of the weight reaches the instruction at every output pixel.
// A stride s spends sh sw - 1 of every sh sw products on zero codes: there is no sub-pixel (per-phase) decomposition here.
#pragma once
#include "qs_mx_conv.h"

namespace qs {

struct MxctShape {
    MxcShape s;                    // the image, the kernel, strides, dilations as the weight path of qs_mx_conv.h reads them; OW, OHW of y
    uint32_t mh, mw;               // floor((2^32 - 1) / sh), floor((2^32 - 1) / sw)
};

struct MxctRow {                   // one output pixel: nh = oh + ph, nw = ow + pw; a row past M: nh = -1 (no tap exists)
    int b, nh, nw;
};

__device__ __forceinline__ MxctRow mxct_row(int64_t row, int64_t rows, const MxctShape& g) {
    MxctRow r;
    const bool ok = row < rows;
    const int64_t rr = ok ? row : 0;
    const int64_t b = rr / g.s.OHW, rem = rr - b * g.s.OHW;
    const int oh = (int)(rem / g.s.OW), ow = (int)(rem - (int64_t)oh * g.s.OW);
    r.b = (int)b, r.nh = ok ? oh + g.s.ph : -1, r.nw = ow + g.s.pw;
    return r;
}

// the input coordinate t / s of axis value t, where it exists (t >= 0, s divides t, t / s < n); -1 where it does not.
// m = floor((2^32 - 1) / s): see the head of this file
__device__ __forceinline__ int mxct_coord(int t, int s, uint32_t m, int n) {
    uint32_t q = __umulhi((uint32_t)t, m), r = (uint32_t)t - q * (uint32_t)s;
    if (r >= (uint32_t)s) r -= (uint32_t)s, ++q;
    return t >= 0 && r == 0u && q < (uint32_t)n ? (int)q : -1;
}

// the pixel (in units of one pixel's C codes / nb scale bytes) row `r` reads at tap `p`; -1 where there is none
__device__ __forceinline__ int64_t mxct_pixel(const MxctRow& r, const MxcPos& p, const MxctShape& g) {
    // unsigned products: at the end of the last step kh == KH, and KH dh may pass 2^31 (the tap is refused below, by kh < KH)
    const int th = (int)((uint32_t)r.nh - (uint32_t)p.kh * (uint32_t)g.s.dh), tw = (int)((uint32_t)r.nw - (uint32_t)p.kw * (uint32_t)g.s.dw);
    const int ih = mxct_coord(th, g.s.sh, g.mh, g.s.H), iw = mxct_coord(tw, g.s.sw, g.mw, g.s.W);
    const bool in = p.kh < g.s.KH && ih >= 0 && iw >= 0;
    return in ? ((int64_t)r.b * g.s.H + ih) * g.s.W + iw : -1;
}

// the four 16-code pieces this thread stages per step: piece (tid & 7) -- at position `p` -- of the output pixels `rows`
template <bool VEC>
__device__ __forceinline__ void mxct_fetch(u32x4 (&reg)[4], const uint8_t* __restrict__ codes, const MxctRow (&rows)[4], const MxcPos& p,
                                           const MxctShape& g) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t px = mxct_pixel(rows[i], p, g);
        const bool in = px >= 0 && p.c < g.s.C;
        u32x4 v = {0u, 0u, 0u, 0u};
        if constexpr (VEC) {                       // an unconditional load from a clamped address, then a select: no branch per piece
            const u32x4 w = *(const u32x4*)(codes + (in ? px * g.s.C + p.c : 0));
            v = in ? w : v;
        } else if (in) {
            const uint8_t* q = codes + px * g.s.C + p.c;
            const int left = g.s.C - p.c < 16 ? g.s.C - p.c : 16;
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (b < left) v[b >> 2] |= (uint32_t)q[b] << (8 * (b & 3));
        }
        reg[i] = v;
    }
}

// the scale bytes of this lane's four fragments (the output pixels `rows`) at block position `p`; 127 (2^0) where there is none
__device__ __forceinline__ void mxct_scales(uint32_t (&s)[4], const uint8_t* __restrict__ scales, const MxctRow (&rows)[4], const MxcPos& p,
                                            const MxctShape& g) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t px = mxct_pixel(rows[j], p, g);
        const uint32_t b = scales[px >= 0 ? px * g.s.nb + p.c : 0];     // (clamped address + select, as the pieces)
        s[j] = px >= 0 ? b : 127u;
    }
}

// FX / FW: the formats of the activation (SrcB, rows m = output pixels) and of the weight (SrcA, rows n = output channels).
// The body is mx_conv_kernel's, with the activation's rows and fetch replaced.
template <int FX, int FW, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_conv_t_kernel(const uint8_t* __restrict__ x_codes, const uint8_t* __restrict__ x_scales,
                                                                const uint8_t* __restrict__ w_codes, const uint8_t* __restrict__ w_scales,
                                                                const float* __restrict__ bias, void* __restrict__ y, int ydt, int64_t M,
                                                                int64_t N, MxctShape g, int tiles_n, int y_vec) {
    using LX = MxgLds<mxg_bits(FX)>;
    using LW = MxgLds<mxg_bits(FW)>;
    constexpr int kBuf = LX::kBytes + LW::kBytes;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kBuf];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * kMxgTile, n0 = (int64_t)(blockIdx.x % tiles_n) * kMxgTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;          // this wave's 64 x 64 corner of the tile
    const int Cp = g.s.nb * QS_MX_BLOCK;
    const int64_t steps = ((int64_t)g.s.KH * g.s.KW * Cp + kMxgK - 1) / kMxgK;

    MxctRow xr[4], xsr[4];                                          // rows of the staged pieces, rows of the fragments' scale bytes
    MxcRow wr[4], wsr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        xr[i] = mxct_row(m0 + (tid >> 3) + 32 * i, M, g);
        wr[i] = mxc_row<false>(n0 + (tid >> 3) + 32 * i, N, g.s);
        xsr[i] = mxct_row(m0 + wm + 16 * i + (lane & 15), M, g);
        wsr[i] = mxc_row<false>(n0 + wn + 16 * i + (lane & 15), N, g.s);
    }
    MxcPos pc = {0, 0, 0}, ps = {0, 0, 0};                          // of this thread's pieces (codes), of its scale bytes (blocks)
    mxc_advance(pc, (tid & 7) * 16, Cp, g.s.KW);
    mxc_advance(ps, lane >> 4, g.s.nb, g.s.KW);

    f32x4 acc[4][4];                                                // [i: 16 n][j: 16 m]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    u32x4 rx[4], rw[4];
    uint32_t sx[4], sw[4], sx_next[4], sw_next[4];
    mxct_fetch<VEC>(rx, x_codes, xr, pc, g);
    mxc_fetch<VEC, false>(rw, w_codes, wr, pc, g.s);
    mxct_scales(sx, x_scales, xsr, ps, g);
    mxc_scales<false>(sw, w_scales, wsr, ps, g.s);
    mxg_stage<mxg_bits(FX)>(lds, rx, tid);
    mxg_stage<mxg_bits(FW)>(lds + LX::kBytes, rw, tid);
    __syncthreads();

    for (int64_t t = 0; t < steps; ++t) {
        const bool more = t + 1 < steps;
        if (more) {
            mxc_advance(pc, kMxgK, Cp, g.s.KW);
            mxc_advance(ps, kMxgK / QS_MX_BLOCK, g.s.nb, g.s.KW);
            mxct_fetch<VEC>(rx, x_codes, xr, pc, g);
            mxc_fetch<VEC, false>(rw, w_codes, wr, pc, g.s);
            mxct_scales(sx_next, x_scales, xsr, ps, g);
            mxc_scales<false>(sw_next, w_scales, wsr, ps, g.s);
        }
        mxc_products<FX, FW>(acc, lds + (t & 1) * kBuf, wm, wn, lane, sx, sw);
        if (more) {
            uint8_t* nxt = lds + ((t + 1) & 1) * kBuf;
            mxg_stage<mxg_bits(FX)>(nxt, rx, tid);
            mxg_stage<mxg_bits(FW)>(nxt + LX::kBytes, rw, tid);
#pragma unroll
            for (int j = 0; j < 4; ++j) sx[j] = sx_next[j], sw[j] = sw_next[j];
        }
        __syncthreads();
    }

    mxc_epilogue(acc, bias, y, ydt, M, N, m0 + wm, n0 + wn, lane, y_vec);
}

}  // namespace qs
