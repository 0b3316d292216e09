// 2-d convolution on MX codes (include/qsparse_hip.h, "MX convolution"): y[B, OH, OW, Cout] from channels-last codes x [B, H, W, C]
// and w [Cout, KH, KW, C] with blocks of 32 along C, by IMPLICIT GEMM on the tile of qs_mx_gemm.h -- no im2col matrix exists in
// memory.  The product is A [M = B OH OW, K'] . Wp [Cout, K']^T with K' = KH KW Cp, Cp = 32 ceil(C / 32) and
//   k' = (kh KW + kw) Cp + c,   A[m, k'] = x[b, oh sh - ph + kh dh, ow sw - pw + kw dw, c],   Wp[n, k'] = w[n, kh, kw, c]
// zero codes (scale byte 127) where c >= C or the tap lies outside the image.  Everything behind the fetch is the GEMM's own code:
// the kernel hands two operands (MxcOperand) to mx_tile_loop and its accumulators to mx_epilogue (qs_mx_gemm.h) -- so the sum is
// accumulated in the order of mx_gemm_kernel on the host-built A and Wp and the result is the same bits.
//
// The fetch.  Piece q = thread + 256 i of a step is piece (thread & 7) of tile row (thread >> 3) + 32 i: the four pieces a thread
// stages per operand share ONE k' and differ in the row.  So a thread keeps
//   per row (4 for the codes, 4 for the scale bytes of its MFMA fragments; computed once, before the K loop): the image b and the
//       corner (ih0, iw0) = (oh sh - ph, ow sw - pw) of the row's window
//   per operand kind one position (c, kh, kw) of its k', advanced by 128 codes (4 blocks) per step with carries into kw and kh --
//       no division inside the loop
// and a piece's address is ((b H + ih0 + kh dh) W + iw0 + kw dw) C + c, in 64 bits.  A piece that does not exist (row past M, tap
// outside the image, c >= C, k' >= K') is loaded from a clamped address and replaced by zeros with a select (mx_load16);
// a scale byte that does not exist is 127.  Because C % 16 == 0 on the VEC route and Cp % 32 == 0, a piece never straddles a tap
// or the end of C there; the PLAIN route loads bytes, each predicated on its own c.  No tap is ever skipped: a 0xFF scale byte
// reaches the instruction whatever the codes are.
// The weight is the same operand without an image (IMG = false): row n, tap, c -> (n KH KW + tap) C + c.
#pragma once
#include "qs_mx_gemm.h"

namespace qs {

struct MxcShape {
    int H, W, C, nb;               // the image; nb = ceil(C / 32) scale bytes per pixel
    int KH, KW, sh, sw, ph, pw, dh, dw;
    int OW;
    int64_t OHW;                   // OH * OW
};

struct MxcRow {                    // one tile row: an output pixel (IMG) or an output channel
    int b, ih0, iw0;               // a row past the operand: ih0 = INT32_MIN (IMG; no tap of it is inside the image), b = -1 (weight)
};

struct MxcPos {                    // where a k' lies: c (codes or blocks) inside the padded channel run of tap (kh, kw)
    int c, kh, kw;
};

// `by` further along k'; `period` = Cp (codes) or nb (blocks).  by <= 4 periods, so at most four carries
__device__ __forceinline__ void mxc_advance(MxcPos& p, int by, int period, int KW) {
    p.c += by;
    while (p.c >= period) {
        p.c -= period;
        if (++p.kw == KW) p.kw = 0, ++p.kh;
    }
}

template <bool IMG>
__device__ __forceinline__ MxcRow mxc_row(int64_t row, int64_t rows, const MxcShape& g) {
    MxcRow r;
    const bool ok = row < rows;
    const int64_t rr = ok ? row : 0;
    if constexpr (IMG) {
        const int64_t b = rr / g.OHW, rem = rr - b * g.OHW;
        const int oh = (int)(rem / g.OW), ow = (int)(rem - (int64_t)oh * g.OW);
        r.b = (int)b, r.ih0 = ok ? oh * g.sh - g.ph : INT32_MIN, r.iw0 = ow * g.sw - g.pw;
    } else {
        r.b = ok ? (int)rr : -1, r.ih0 = 0, r.iw0 = 0;
    }
    return r;
}

// the pixel (in units of one pixel's C codes / nb scale bytes) row `r` reads at tap `p`; -1 where there is none
template <bool IMG>
__device__ __forceinline__ int64_t mxc_pixel(const MxcRow& r, const MxcPos& p, const MxcShape& g) {
    if constexpr (IMG) {
        // unsigned: a tap above / left of the image wraps to a huge value and fails the one comparison; so does every tap of a row
        // past M (2^31 + kh dh with kh dh < 2^31 for kh < KH: the host checks the dilated kernel against the padded image)
        const unsigned ih = (unsigned)r.ih0 + (unsigned)p.kh * (unsigned)g.dh, iw = (unsigned)r.iw0 + (unsigned)p.kw * (unsigned)g.dw;
        const bool in = p.kh < g.KH && ih < (unsigned)g.H && iw < (unsigned)g.W;
        return in ? ((int64_t)r.b * g.H + (int64_t)ih) * g.W + (int64_t)iw : -1;
    } else {
        return r.b >= 0 && p.kh < g.KH ? ((int64_t)r.b * g.KH + p.kh) * g.KW + p.kw : -1;
    }
}

// where this thread stands along k': the position of its pieces (codes) and of its lane's scale bytes (blocks).  One walk serves
// both operands of a product -- they read the same k' -- and the activation's operand advances it: 128 codes (4 blocks) per step.
// The walk is over any k' = (outer * wrap + middle) * period + inner: the weight gradient (qs_mx_conv_wgrad.h) walks (oh, ow, b)
struct MxcWalk {
    MxcPos pc, ps;
    int Cp, nb, KW;

    // a period of `nb` blocks, the middle coordinate wrapping at `wrap`; `start` = where the first code of the first step lies (its c:
    // a multiple of the block)
    __device__ __forceinline__ MxcWalk(int nb, int wrap, const MxcPos& start, int tid)
        : pc(start), ps{start.c / QS_MX_BLOCK, start.kh, start.kw}, Cp(nb * QS_MX_BLOCK), nb(nb), KW(wrap) {
        mxc_advance(pc, (tid & 7) * 16, Cp, KW);
        mxc_advance(ps, (tid & 63) >> 4, nb, KW);
    }
    __device__ __forceinline__ MxcWalk(const MxcShape& g, int tid) : MxcWalk(g.nb, g.KW, MxcPos{0, 0, 0}, tid) {}
    __device__ __forceinline__ void advance() {
        mxc_advance(pc, kMxgK, Cp, KW);
        mxc_advance(ps, kMxgK / QS_MX_BLOCK, nb, KW);
    }
};

// the 16 codes / the scale byte of pixel `px` (-1: none) at position `p`
template <bool VEC>
__device__ __forceinline__ u32x4 mxc_piece(const uint8_t* __restrict__ codes, int64_t px, const MxcPos& p, const MxcShape& g) {
    return mx_load16<VEC>(codes, px >= 0 && p.c < g.C, px * g.C + p.c, g.C - p.c < 16 ? g.C - p.c : 16);
}
__device__ __forceinline__ uint32_t mxc_scale(const uint8_t* __restrict__ scales, int64_t px, const MxcPos& p, const MxcShape& g) {
    return mx_scale(scales, px >= 0, px * g.nb + p.c);
}

// the operand (qs_mx_gemm.h, mx_tile_loop) of a convolution: the image x (IMG; tile rows = output pixels from row0) or the weight
// (tile rows = output channels).  It follows `walk` from step 0 and ignores the step it is asked for
template <bool IMG>
struct MxcOperand {
    const uint8_t* __restrict__ codes;
    const uint8_t* __restrict__ sbytes;
    const MxcShape& g;
    MxcWalk& walk;
    MxcRow pr[4], sr[4];           // rows of the staged pieces, rows of the fragments' scale bytes: computed once, before the K loop

    __device__ __forceinline__ MxcOperand(const uint8_t* codes, const uint8_t* scales, int64_t rows, const MxcShape& g, MxcWalk& walk,
                                          int64_t row0, int w, int tid)
        : codes(codes), sbytes(scales), g(g), walk(walk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pr[i] = mxc_row<IMG>(row0 + (tid >> 3) + 32 * i, rows, g);
            sr[i] = mxc_row<IMG>(row0 + w + 16 * i + (tid & 15), rows, g);
        }
    }

    __device__ __forceinline__ void advance() {
        if constexpr (IMG) walk.advance();
    }

    template <bool VEC>
    __device__ __forceinline__ void fetch(u32x4 (&reg)[4], int64_t) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) reg[i] = mxc_piece<VEC>(codes, mxc_pixel<IMG>(pr[i], walk.pc, g), walk.pc, g);
    }

    __device__ __forceinline__ void scales(uint32_t (&s)[4], int64_t) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = mxc_scale(sbytes, mxc_pixel<IMG>(sr[j], walk.ps, g), walk.ps, g);
    }
};

// the kernel's view of a convolution's arguments (Args: qs_mx_conv2d_args or its transposed sibling) with the output OH x OW
template <class Args>
inline MxcShape mxc_shape(const Args& a, int64_t OH, int64_t OW) {
    MxcShape g;
    g.H = (int)a.H, g.W = (int)a.W, g.C = (int)a.C, g.nb = (int)((a.C + QS_MX_BLOCK - 1) / QS_MX_BLOCK);
    g.KH = a.KH, g.KW = a.KW, g.sh = a.stride_h, g.sw = a.stride_w, g.ph = a.pad_h, g.pw = a.pad_w, g.dh = a.dil_h, g.dw = a.dil_w;
    g.OW = (int)OW, g.OHW = OH * OW;
    return g;
}

// FX / FW: the formats of the activation (SrcB, rows m = output pixels) and of the weight (SrcA, rows n = output channels)
template <int FX, int FW, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_conv_kernel(const uint8_t* __restrict__ x_codes, const uint8_t* __restrict__ x_scales,
                                                              const uint8_t* __restrict__ w_codes, const uint8_t* __restrict__ w_scales,
                                                              const float* __restrict__ bias, void* __restrict__ y, int ydt, int64_t M,
                                                              int64_t N, MxcShape g, int tiles_n, int y_vec) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxTileLds<FX, FW>];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * kMxgTile, n0 = (int64_t)(blockIdx.x % tiles_n) * kMxgTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;          // this wave's 64 x 64 corner of the tile
    MxcWalk walk(g, tid);
    MxcOperand<true> X(x_codes, x_scales, M, g, walk, m0, wm, tid);
    MxcOperand<false> Wt(w_codes, w_scales, N, g, walk, n0, wn, tid);
    f32x4 acc[4][4];
    mx_zero(acc);
    mx_tile_loop<FX, FW, VEC>(acc, X, Wt, 0, ((int64_t)g.KH * g.KW * walk.Cp + kMxgK - 1) / kMxgK, lds, tid, wm, wn);
    mx_epilogue(acc, bias, y, ydt, M, N, m0 + wm, n0 + wn, tid & 63, y_vec);
}

}  // namespace qs
