// 2-d convolution on MX codes that WRITES MX codes (include/qsparse_hip.h, "MX products that write MX codes"): the body of
// mx_conv_kernel (qs_mx_conv.h) -- the same two operands handed to mx_tile_loop, hence the same sums -- with mx_epilogue_codes
// (qs_mx_gemm.h) in place of mx_epilogue: codes [B, OH, OW, Cout] and scale bytes [B, OH, OW, ceil(Cout / 32)] with blocks of 32
// along the output channels, which are the next convolution's input channels.
#pragma once
#include "qs_mx_conv.h"

namespace qs {

template <int FX, int FW, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_conv_q_kernel(const uint8_t* __restrict__ x_codes, const uint8_t* __restrict__ x_scales,
                                                                const uint8_t* __restrict__ w_codes, const uint8_t* __restrict__ w_scales,
                                                                const float* __restrict__ bias, int relu, MxFormat f,
                                                                uint8_t* __restrict__ out_codes, uint8_t* __restrict__ out_scales,
                                                                int64_t M, int64_t N, MxcShape g, int tiles_n, int c_vec) {
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
    mx_epilogue_codes(acc, bias, relu, f, out_codes, out_scales, M, N, m0 + wm, n0 + wn, tid & 63, c_vec);
}

}  // namespace qs
