// 2-d convolution on MX codes (include/qsparse_hip.h, "MX convolution"): y[B, OH, OW, Cout] from channels-last codes x [B, H, W, C]
// and w [Cout, KH, KW, C] with blocks of 32 along C, by IMPLICIT GEMM on the tile of qs_mx_gemm.h -- no im2col matrix exists in
// memory.  The product is A [M = B OH OW, K'] . Wp [Cout, K']^T with K' = KH KW Cp, Cp = 32 ceil(C / 32) and
//   k' = (kh KW + kw) Cp + c,   A[m, k'] = x[b, oh sh - ph + kh dh, ow sw - pw + kw dw, c],   Wp[n, k'] = w[n, kh, kw, c]
// zero codes (scale byte 127) where c >= C or the tap lies outside the image.  Everything behind the fetch is the GEMM's own code:
// MxgLds / mxg_stage (LDS image), and its step (16 MFMAs per step of 128 along k') and epilogue -- so the sum is accumulated in
// the order of mx_gemm_kernel on the host-built A and Wp and the result is the same bits.
//
// The fetch.  Piece q = thread + 256 i of a step is piece (thread & 7) of tile row (thread >> 3) + 32 i: the four pieces a thread
// stages per operand share ONE k' and differ in the row.  So a thread keeps
//   per row (4 for the codes, 4 for the scale bytes of its MFMA fragments; computed once, before the K loop): the image b and the
//       corner (ih0, iw0) = (oh sh - ph, ow sw - pw) of the row's window
//   per operand kind one position (c, kh, kw) of its k', advanced by 128 codes (4 blocks) per step with carries into kw and kh --
//       no division inside the loop
// and a piece's address is ((b H + ih0 + kh dh) W + iw0 + kw dw) C + c, in 64 bits.  A piece that does not exist (row past M, tap
// outside the image, c >= C, k' >= K') is loaded from a clamped address and replaced by zeros with a select, as mxg_fetch does;
// a scale byte that does not exist is 127.  Because C % 16 == 0 on the VEC route and Cp % 32 == 0, a piece never straddles a tap
// or the end of C there; the PLAIN route loads bytes, each predicated on its own c.  No tap is ever skipped: a 0xFF scale byte
// reaches the instruction whatever the codes are.
// The weight goes through the same functor as an operand without an image (IMG = false): row n, tap, c -> (n KH KW + tap) C + c.
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

// the four 16-code pieces this thread stages per step: piece (tid & 7) -- at position `p` -- of the rows `rows`
template <bool VEC, bool IMG>
__device__ __forceinline__ void mxc_fetch(u32x4 (&reg)[4], const uint8_t* __restrict__ codes, const MxcRow (&rows)[4], const MxcPos& p,
                                          const MxcShape& g) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t px = mxc_pixel<IMG>(rows[i], p, g);
        const bool in = px >= 0 && p.c < g.C;
        u32x4 v = {0u, 0u, 0u, 0u};
        if constexpr (VEC) {                       // an unconditional load from a clamped address, then a select: no branch per piece
            const u32x4 w = *(const u32x4*)(codes + (in ? px * g.C + p.c : 0));
            v = in ? w : v;
        } else if (in) {
            const uint8_t* q = codes + px * g.C + p.c;
            const int left = g.C - p.c < 16 ? g.C - p.c : 16;
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (b < left) v[b >> 2] |= (uint32_t)q[b] << (8 * (b & 3));
        }
        reg[i] = v;
    }
}

// the scale bytes of this lane's four fragments (the rows `rows`) at block position `p`; 127 (2^0) where there is none
template <bool IMG>
__device__ __forceinline__ void mxc_scales(uint32_t (&s)[4], const uint8_t* __restrict__ scales, const MxcRow (&rows)[4], const MxcPos& p,
                                           const MxcShape& g) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t px = mxc_pixel<IMG>(rows[j], p, g);
        const uint32_t b = scales[px >= 0 ? px * g.nb + p.c : 0];       // (clamped address + select, as the pieces)
        s[j] = px >= 0 ? b : 127u;
    }
}

// mxc_products / mxc_epilogue are the step and the epilogue of mx_gemm_kernel, statement for statement.  They are stated here and
// not shared with that kernel on purpose: moving them out of mx_gemm_kernel into helpers, force-inlined, changed its register
// allocation (180 -> 182 VGPRs on E4M3 x E4M3, other pairs likewise), and the GEMM's device code is not to change with this unit.
// one step's products of a wave: its four fragments of either operand from the staged tile `cur`, 16 MFMAs into 16 accumulators
template <int FA, int FB>
__device__ __forceinline__ void mxc_products(f32x4 (&acc)[4][4], const uint8_t* cur, int wm, int wn, int lane, const uint32_t (&sa)[4],
                                             const uint32_t (&sb)[4]) {
    using LA = MxgLds<mxg_bits(FA)>;
    using LB = MxgLds<mxg_bits(FB)>;
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
}

// bias in float32, one rounding to ydt, the stores of a wave's 64 (m, from mw) x 64 (n, from nw) corner of y [M, N]
__device__ __forceinline__ void mxc_epilogue(const f32x4 (&acc)[4][4], const float* __restrict__ bias, void* __restrict__ y, int ydt,
                                             int64_t M, int64_t N, int64_t mw, int64_t nw, int lane, int y_vec) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t n = nw + 16 * i + 4 * (lane >> 4);
        float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (bias) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < N) bv[r] = bias[n + r];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t m = mw + 16 * j + (lane & 15);
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = bias ? acc[i][j][r] + bv[r] : acc[i][j][r];
            if (m >= M || n >= N) continue;
            const int64_t e = m * N + n;
            if (y_vec) {                           // N % 4 == 0 and y 16-byte (float32) / 8-byte aligned: n + 3 < N, aligned store
                if (ydt == QS_F32) {
                    *(u32x4*)((float*)y + e) = u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
                } else if (ydt == QS_BF16) {
                    *(u32x2*)((uint16_t*)y + e) = u32x2{f32_to_bf16_bits(v[0]) | (f32_to_bf16_bits(v[1]) << 16),
                                                        f32_to_bf16_bits(v[2]) | (f32_to_bf16_bits(v[3]) << 16)};
                } else {
                    *(u32x2*)((uint16_t*)y + e) = u32x2{f32_to_f16_bits(v[0]) | (f32_to_f16_bits(v[1]) << 16),
                                                        f32_to_f16_bits(v[2]) | (f32_to_f16_bits(v[3]) << 16)};
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (n + r >= N) break;
                    if (ydt == QS_F32) ((float*)y)[e + r] = v[r];
                    else if (ydt == QS_BF16) ((uint16_t*)y)[e + r] = (uint16_t)f32_to_bf16_bits(v[r]);
                    else ((uint16_t*)y)[e + r] = (uint16_t)f32_to_f16_bits(v[r]);
                }
            }
        }
    }
}

// FX / FW: the formats of the activation (SrcB, rows m = output pixels) and of the weight (SrcA, rows n = output channels)
template <int FX, int FW, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_conv_kernel(const uint8_t* __restrict__ x_codes, const uint8_t* __restrict__ x_scales,
                                                              const uint8_t* __restrict__ w_codes, const uint8_t* __restrict__ w_scales,
                                                              const float* __restrict__ bias, void* __restrict__ y, int ydt, int64_t M,
                                                              int64_t N, MxcShape g, int tiles_n, int y_vec) {
    using LX = MxgLds<mxg_bits(FX)>;
    using LW = MxgLds<mxg_bits(FW)>;
    constexpr int kBuf = LX::kBytes + LW::kBytes;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kBuf];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * kMxgTile, n0 = (int64_t)(blockIdx.x % tiles_n) * kMxgTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;          // this wave's 64 x 64 corner of the tile
    const int Cp = g.nb * QS_MX_BLOCK;
    const int64_t steps = ((int64_t)g.KH * g.KW * Cp + kMxgK - 1) / kMxgK;

    MxcRow xr[4], wr[4], xsr[4], wsr[4];                            // rows of the staged pieces, rows of the fragments' scale bytes
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        xr[i] = mxc_row<true>(m0 + (tid >> 3) + 32 * i, M, g);
        wr[i] = mxc_row<false>(n0 + (tid >> 3) + 32 * i, N, g);
        xsr[i] = mxc_row<true>(m0 + wm + 16 * i + (lane & 15), M, g);
        wsr[i] = mxc_row<false>(n0 + wn + 16 * i + (lane & 15), N, g);
    }
    MxcPos pc = {0, 0, 0}, ps = {0, 0, 0};                          // of this thread's pieces (codes), of its scale bytes (blocks)
    mxc_advance(pc, (tid & 7) * 16, Cp, g.KW);
    mxc_advance(ps, lane >> 4, g.nb, g.KW);

    f32x4 acc[4][4];                                                // [i: 16 n][j: 16 m]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    u32x4 rx[4], rw[4];
    uint32_t sx[4], sw[4], sx_next[4], sw_next[4];
    mxc_fetch<VEC, true>(rx, x_codes, xr, pc, g);
    mxc_fetch<VEC, false>(rw, w_codes, wr, pc, g);
    mxc_scales<true>(sx, x_scales, xsr, ps, g);
    mxc_scales<false>(sw, w_scales, wsr, ps, g);
    mxg_stage<mxg_bits(FX)>(lds, rx, tid);
    mxg_stage<mxg_bits(FW)>(lds + LX::kBytes, rw, tid);
    __syncthreads();

    for (int64_t t = 0; t < steps; ++t) {
        const bool more = t + 1 < steps;
        if (more) {
            mxc_advance(pc, kMxgK, Cp, g.KW);
            mxc_advance(ps, kMxgK / QS_MX_BLOCK, g.nb, g.KW);
            mxc_fetch<VEC, true>(rx, x_codes, xr, pc, g);
            mxc_fetch<VEC, false>(rw, w_codes, wr, pc, g);
            mxc_scales<true>(sx_next, x_scales, xsr, ps, g);
            mxc_scales<false>(sw_next, w_scales, wsr, ps, g);
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
