// Weight gradient of the 2-d convolution on MX codes (include/qsparse_hip.h, "MX convolution, weight gradient"):
//   dW[n, kh, kw, c] = sum over (oh, ow, b) of dy[oh, ow, n, b] * x[oh sh - ph + kh dh, ow sw - pw + kw dw, c, b]
// from BATCH-BLOCKED operands: dyt [OH, OW, Cout, B] and xt [H, W, C, B] with MX blocks of 32 along the batch B, the innermost axis.
// A block of 32 images at one pixel and channel is the same 32 numbers under every tap (kh, kw), so each tensor is quantized once
// (the column pair of the two-way quantizer on [B, H W C]) and serves all taps; blocks along the output pixels could not.
//
// It is the implicit GEMM of qs_mx_conv.h with two other operands: the product is G [M = Cout, K'] . X' [N = KH KW C, K']^T with
//   Bp = 32 ceil(B / 32),  k' = (oh OW + ow) Bp + b,  K' = OH OW Bp
//   G[n, k']  = dyt[oh, ow, n, b]                                        slot A of mx_tile_loop (tile rows m = output channels)
//   X'[r, k'] = xt[oh sh - ph + kh dh, ow sw - pw + kw dw, c, b]         slot B (tile rows r = (kh KW + kw) C + c)
// zero codes where b >= B or the tap lies outside the image; the scale byte of a block that does not exist at all (a tap outside
// the image) is 127.  y [Cout, KH KW C] row-major IS dW [Cout, KH, KW, C].  The loop and the epilogue are qs_mx_gemm.h's, so the sum
// is accumulated in the order of mx_gemm_kernel on the host-gathered G and X' and the result is the same bits.
//
// The walk.  Both operands read the same k', so they share one MxcWalk (qs_mx_conv.h) with period Bp and OW in place of KW: the
// position (c, kw, kh) of that struct is (b, ow, oh) here, advanced by 128 codes (4 blocks) per step with carries -- no division
// inside the loop.  A slice of a split product starts at step t0: the position of code 128 t0 is found once, with divisions,
// before the loop (mxw_walk).  Per tile row the x operand keeps (c, kh dh - ph, kw dw - pw), decomposed once before the loop; its
// pixel at the walk's (oh, ow) is (oh sh + kh dh - ph, ow sw + kw dw - pw).  A piece that does not exist (row past the operand,
// tap outside the image, b >= B, k' >= K') is loaded from a clamped address and replaced by zeros with a select (mx_load16), a
// scale byte by 127 (mx_scale).  B % 16 == 0 on the VEC route and Bp % 32 == 0, so a piece never straddles the end of B there; the
// PLAIN route loads bytes, each predicated on its own b.  No tap and no pixel is skipped: a 0xFF scale byte reaches the instruction
// whatever the codes are.
//
// Split along K' (qs_mx_gemm_splitk.h's slicing): the grid is tiles x slices, slice-major; work-group (s, tile) walks the steps
// [s per, min((s + 1) per, steps)) from zero accumulators.  With one slice it rounds once into dW (mx_epilogue); with more it stores
// its raw float32 accumulators to workspace[s][Cout][KH KW C] and mx_gemm_reduce_kernel adds the slices in ascending order -- one
// kernel with a uniform branch at the end, not two.
#pragma once
#include "qs_mx_conv.h"

namespace qs {

struct MxwShape {
    int H, W, C, B, nb;            // the image x [H, W, C, B]; nb = ceil(B / 32) scale bytes per (pixel, channel)
    int OH, OW, Cout;              // dy [OH, OW, Cout, B]
    int KH, KW, sh, sw, ph, pw, dh, dw;
};

// where the thread stands at step t0: MxcWalk over (b, ow, oh) -- its (c, kw, kh) -- with period Bp, ow wrapping at OW, from the
// position of code 128 t0.  The divisions are of work-group-uniform values, once
__device__ __forceinline__ MxcWalk mxw_walk(const MxwShape& g, int tid, int64_t t0) {
    const int64_t Bp = (int64_t)g.nb * QS_MX_BLOCK, k0 = t0 * kMxgK, pix = k0 / Bp, oh = pix / g.OW;
    return MxcWalk(g.nb, g.OW, MxcPos{(int)(k0 - pix * Bp), (int)oh, (int)(pix - oh * g.OW)}, tid);
}

// the operand dy: tile rows are output channels n from row0; the address of (oh, ow, n, b) is ((oh OW + ow) Cout + n) B + b.
// It advances the walk
struct MxwDyOperand {
    const uint8_t* __restrict__ codes;
    const uint8_t* __restrict__ sbytes;
    const MxwShape& g;
    MxcWalk& walk;
    int64_t prow, srow;            // the first of this thread's four piece rows (+ 32 i) and of its four scale rows (+ 16 j)

    __device__ __forceinline__ MxwDyOperand(const uint8_t* codes, const uint8_t* scales, const MxwShape& g, MxcWalk& walk, int64_t row0,
                                            int w, int tid)
        : codes(codes), sbytes(scales), g(g), walk(walk), prow(row0 + (tid >> 3)), srow(row0 + w + (tid & 15)) {}

    __device__ __forceinline__ void advance() { walk.advance(); }

    template <bool VEC>
    __device__ __forceinline__ void fetch(u32x4 (&reg)[4], int64_t) const {
        const MxcPos& p = walk.pc;                 // (b, oh, ow)
        const bool live = p.kh < g.OH && p.c < g.B;
        const int64_t px = (int64_t)p.kh * g.OW + p.kw;
        const int left = g.B - p.c < 16 ? g.B - p.c : 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t n = prow + 32 * i;
            reg[i] = mx_load16<VEC>(codes, live && n < g.Cout, (px * g.Cout + n) * g.B + p.c, left);
        }
    }

    __device__ __forceinline__ void scales(uint32_t (&s)[4], int64_t) const {
        const MxcPos& p = walk.ps;                 // (block of b, oh, ow)
        const bool live = p.kh < g.OH;
        const int64_t px = (int64_t)p.kh * g.OW + p.kw;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t n = srow + 16 * j;
            s[j] = mx_scale(sbytes, live && n < g.Cout, (px * g.Cout + n) * g.nb + p.c);
        }
    }
};

struct MxwRow {                    // one tile row r = (kh KW + kw) C + c of the x operand: c and the tap's offset (kh dh - ph, kw dw - pw)
    int c, fh, fw;                 // a row past KH KW C: fh = INT32_MIN (no pixel of it is inside the image)
};

__device__ __forceinline__ MxwRow mxw_row(int64_t row, int64_t rows, const MxwShape& g) {
    const bool ok = row < rows;
    const int64_t rr = ok ? row : 0, tap = rr / g.C;
    const int kh = (int)(tap / g.KW), kw = (int)(tap - (int64_t)kh * g.KW);
    MxwRow r;
    r.c = (int)(rr - tap * g.C), r.fh = ok ? kh * g.dh - g.ph : INT32_MIN, r.fw = kw * g.dw - g.pw;
    return r;
}

// the (pixel, channel) of x, in units of B codes / nb scale bytes, row `r` reads at the walk's (oh, ow); -1 where there is none
__device__ __forceinline__ int64_t mxw_pixel(const MxwRow& r, const MxcPos& p, const MxwShape& g) {
    // unsigned: a tap above / left of the image wraps to a huge value and fails the one comparison; so does every tap of a row past
    // the operand (2^31 + oh sh with oh sh < 2^31 for oh < OH: the host checks the padded image against 31 bits)
    const unsigned ih = (unsigned)p.kh * (unsigned)g.sh + (unsigned)r.fh, iw = (unsigned)p.kw * (unsigned)g.sw + (unsigned)r.fw;
    const bool in = p.kh < g.OH && ih < (unsigned)g.H && iw < (unsigned)g.W;
    return in ? ((int64_t)ih * g.W + (int64_t)iw) * g.C + r.c : -1;
}

// the operand x: tile rows are r = (kh KW + kw) C + c from row0; the address of (ih, iw, c, b) is ((ih W + iw) C + c) B + b.
// It follows the walk dy's operand advances
struct MxwXOperand {
    const uint8_t* __restrict__ codes;
    const uint8_t* __restrict__ sbytes;
    const MxwShape& g;
    const MxcWalk& walk;
    MxwRow pr[4], sr[4];           // rows of the staged pieces, rows of the fragments' scale bytes: computed once, before the K loop

    __device__ __forceinline__ MxwXOperand(const uint8_t* codes, const uint8_t* scales, int64_t rows, const MxwShape& g, const MxcWalk& walk,
                                           int64_t row0, int w, int tid)
        : codes(codes), sbytes(scales), g(g), walk(walk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pr[i] = mxw_row(row0 + (tid >> 3) + 32 * i, rows, g);
            sr[i] = mxw_row(row0 + w + 16 * i + (tid & 15), rows, g);
        }
    }

    __device__ __forceinline__ void advance() {}

    template <bool VEC>
    __device__ __forceinline__ void fetch(u32x4 (&reg)[4], int64_t) const {
        const MxcPos& p = walk.pc;
        const int left = g.B - p.c < 16 ? g.B - p.c : 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t px = mxw_pixel(pr[i], p, g);
            reg[i] = mx_load16<VEC>(codes, px >= 0 && p.c < g.B, px * g.B + p.c, left);
        }
    }

    __device__ __forceinline__ void scales(uint32_t (&s)[4], int64_t) const {
        const MxcPos& p = walk.ps;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t px = mxw_pixel(sr[j], p, g);
            s[j] = mx_scale(sbytes, px >= 0, px * g.nb + p.c);
        }
    }
};

// a wave's 64 (m, from mw) x 64 (n, from nw) corner of one slice's raw accumulators to p [M, N]: the stores of mx_gemm_partial_kernel
__device__ __forceinline__ void mxw_store_partial(const f32x4 (&acc)[4][4], float* __restrict__ p, int64_t M, int64_t N, int64_t mw,
                                                  int64_t nw, int lane, int ws_vec) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t n = nw + 16 * i + 4 * (lane >> 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t m = mw + 16 * j + (lane & 15);
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

// FG / FX: the formats of dy (SrcB of the instruction, rows m = output channels) and of x (SrcA, rows n = (kh, kw, c)).
// M = Cout, N = KH KW C; grid = tiles x slices, slice-major; slice s walks [s per, min((s + 1) per, steps)), never empty (host)
template <int FG, int FX, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_conv_wgrad_kernel(const uint8_t* __restrict__ dy_codes, const uint8_t* __restrict__ dy_scales,
                                                                    const uint8_t* __restrict__ x_codes, const uint8_t* __restrict__ x_scales,
                                                                    float* __restrict__ ws, void* __restrict__ dw, int ydt, int64_t M,
                                                                    int64_t N, MxwShape g, int tiles_n, int tiles, int64_t per, int64_t steps,
                                                                    int slices, int y_vec, int ws_vec) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxTileLds<FG, FX>];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int slice = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int64_t m0 = (int64_t)(tile / tiles_n) * kMxgTile, n0 = (int64_t)(tile % tiles_n) * kMxgTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;          // this wave's 64 x 64 corner of the tile
    const int64_t t0 = slice * per, t1 = t0 + per < steps ? t0 + per : steps;
    MxcWalk walk = mxw_walk(g, tid, t0);
    MxwDyOperand G(dy_codes, dy_scales, g, walk, m0, wm, tid);
    MxwXOperand X(x_codes, x_scales, N, g, walk, n0, wn, tid);
    f32x4 acc[4][4];
    mx_zero(acc);
    mx_tile_loop<FG, FX, VEC>(acc, G, X, t0, t1, lds, tid, wm, wn);
    if (slices > 1) mxw_store_partial(acc, ws + (int64_t)slice * M * N, M, N, m0 + wm, n0 + wn, tid & 63, ws_vec);
    else mx_epilogue(acc, nullptr, dw, ydt, M, N, m0 + wm, n0 + wn, tid & 63, y_vec);
}

}  // namespace qs
