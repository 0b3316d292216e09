// Transposed 2-d convolution on MX codes (include/qsparse_hip.h, "MX transposed convolution"): y[B, OH, OW, Cout] from channels-last
// codes x [B, H, W, C] and w [Cout, KH, KW, C] with blocks of 32 along C -- also the input gradient of a convolution, whose
// contraction runs over (kh, kw, cout).  It is the implicit GEMM of qs_mx_conv.h with another image operand: the product is
// A [M = B OH OW, K'] . Wp [Cout, K']^T with K' = KH KW Cp, Cp = 32 ceil(C / 32), k' = (kh KW + kw) Cp + c and
//   A[m, k'] = x[b, (oh + ph - kh dh) / sh, (ow + pw - kw dw) / sw, c]   where both divisions are exact and the pixel is inside,
//   Wp[n, k'] = w[n, kh, kw, c]   (the weight's own indices, un-flipped)
// zero codes (scale byte 127) everywhere else.  Everything but the image's rows and pixels is shared: the walk along k', the piece
// and scale loads and the weight's operand are qs_mx_conv.h's, the loop and the epilogue qs_mx_gemm.h's -- so the sum is
// accumulated in the order of mx_gemm_kernel on the host-gathered A and Wp and the result is the same bits.
//
// The image operand.  A row keeps (b, nh, nw) = (b, oh + ph, ow + pw), computed once before the K loop.  At tap (kh, kw) the axis
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

// the operand (qs_mx_gemm.h, mx_tile_loop) of the image x: MxcOperand<true> with the rows and the pixel above
struct MxctOperand {
    const uint8_t* __restrict__ codes;
    const uint8_t* __restrict__ sbytes;
    const MxctShape& g;
    MxcWalk& walk;
    MxctRow pr[4], sr[4];          // rows of the staged pieces, rows of the fragments' scale bytes: computed once, before the K loop

    __device__ __forceinline__ MxctOperand(const uint8_t* codes, const uint8_t* scales, int64_t rows, const MxctShape& g, MxcWalk& walk,
                                           int64_t row0, int w, int tid)
        : codes(codes), sbytes(scales), g(g), walk(walk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pr[i] = mxct_row(row0 + (tid >> 3) + 32 * i, rows, g);
            sr[i] = mxct_row(row0 + w + 16 * i + (tid & 15), rows, g);
        }
    }

    __device__ __forceinline__ void advance() { walk.advance(); }

    template <bool VEC>
    __device__ __forceinline__ void fetch(u32x4 (&reg)[4], int64_t) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) reg[i] = mxc_piece<VEC>(codes, mxct_pixel(pr[i], walk.pc, g), walk.pc, g.s);
    }

    __device__ __forceinline__ void scales(uint32_t (&s)[4], int64_t) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = mxc_scale(sbytes, mxct_pixel(sr[j], walk.ps, g), walk.ps, g.s);
    }
};

// FX / FW: the formats of the activation (SrcB, rows m = output pixels) and of the weight (SrcA, rows n = output channels)
template <int FX, int FW, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_conv_t_kernel(const uint8_t* __restrict__ x_codes, const uint8_t* __restrict__ x_scales,
                                                                const uint8_t* __restrict__ w_codes, const uint8_t* __restrict__ w_scales,
                                                                const float* __restrict__ bias, void* __restrict__ y, int ydt, int64_t M,
                                                                int64_t N, MxctShape g, int tiles_n, int y_vec) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxTileLds<FX, FW>];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * kMxgTile, n0 = (int64_t)(blockIdx.x % tiles_n) * kMxgTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;          // this wave's 64 x 64 corner of the tile
    MxcWalk walk(g.s, tid);
    MxctOperand X(x_codes, x_scales, M, g, walk, m0, wm, tid);
    MxcOperand<false> Wt(w_codes, w_scales, N, g.s, walk, n0, wn, tid);
    f32x4 acc[4][4];
    mx_zero(acc);
    mx_tile_loop<FX, FW, VEC>(acc, X, Wt, 0, ((int64_t)g.s.KH * g.s.KW * walk.Cp + kMxgK - 1) / kMxgK, lds, tid, wm, wn);
    mx_epilogue(acc, bias, y, ydt, M, N, m0 + wm, n0 + wn, tid & 63, y_vec);
}

}  // namespace qs
