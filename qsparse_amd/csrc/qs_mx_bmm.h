// Batched matrix product on MX codes (include/qsparse_hip.h, "MX batched matrix product"): y[g] = A[g] [M, K] . B[g] [N, K]^T for G
// dense slices, neither operand a weight -- the Q . K^T and P . V of attention, the per-expert linear layers.  Slice g of the result
// is bit for bit what mx_gemm_kernel (qs_mx_gemm.h) writes for slice g of the operands: the same 128 x 128 tile, the same walk along
// K in steps of 128, the same 16 MFMAs per step in the same order, the same epilogue.
//
// It is mx_tile_loop over a row-major operand (MxbOperand) whose bases are the slice's, which is what the shared loop is for; the
// plain product keeps its written-out loop because this form measured 3-17 % slower there at short K (qs_mx_gemm.h), a cost the
// batched product accepts rather than state the loop a fifth time.
//
// Index decode: one work-group per tile per slice, the slice folded into the linear block index (gridDim.y stops at 65535):
//   block = g * tiles + tile,  tile = tile_m * tiles_n + tile_n,  tiles = tiles_m * tiles_n
// Rows past M / N and codes past K are zero codes with the scale byte 127; the addresses of such pieces are clamped to the SLICE's
// base, so nothing outside slice g of the operands is read by the work-groups of slice g, and nothing outside slice g of y written.
#pragma once
#include "qs_mx_host.h"

namespace qs {

// the operand (qs_mx_gemm.h, mx_tile_loop) of a row-major matrix: `codes` [rows, K] and `sbytes` [rows, nkb] are one slice's.  Tile
// rows start at row0; w is the wave's corner (the rows of its fragments' scale bytes)
struct MxbOperand {
    const uint8_t* __restrict__ codes;
    const uint8_t* __restrict__ sbytes;
    int64_t rows, K, nkb;
    int64_t prow, srow;            // the first row this thread stages a piece of, the first row it takes a scale byte of
    int k, kb;                     // this thread's piece inside a step (codes), this lane's block inside a step

    __device__ __forceinline__ MxbOperand(const uint8_t* codes, const uint8_t* scales, int64_t rows, int64_t K, int64_t row0, int w, int tid)
        : codes(codes), sbytes(scales), rows(rows), K(K), nkb((K + QS_MX_BLOCK - 1) / QS_MX_BLOCK), prow(row0 + (tid >> 3)),
          srow(row0 + w + (tid & 15)), k((tid & 7) * 16), kb((tid & 63) >> 4) {}

    __device__ __forceinline__ void advance() {}

    template <bool VEC>
    __device__ __forceinline__ void fetch(u32x4 (&reg)[4], int64_t step) const {
        const int64_t k0 = step * kMxgK + k;
        const int left = (int)(K - k0 < 16 ? K - k0 : 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t row = prow + 32 * i;
            reg[i] = mx_load16<VEC>(codes, row < rows && k0 < K, row * K + k0, left);
        }
    }

    __device__ __forceinline__ void scales(uint32_t (&s)[4], int64_t step) const {
        const int64_t b = step * (kMxgK / QS_MX_BLOCK) + kb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = srow + 16 * j;
            s[j] = mx_scale(sbytes, row < rows && b < nkb, row * nkb + b);
        }
    }
};

// what both batched kernels decode from the block index: the slice and the tile's corner
struct MxbBlock {
    int64_t g, m0, n0;
    __device__ __forceinline__ MxbBlock(int tiles, int tiles_n) {
        const unsigned tile = blockIdx.x % (unsigned)tiles;
        g = blockIdx.x / (unsigned)tiles;
        m0 = (int64_t)(tile / (unsigned)tiles_n) * kMxgTile, n0 = (int64_t)(tile % (unsigned)tiles_n) * kMxgTile;
    }
};

// bias_stride: 0 (one [N] bias for every slice) or N ([G, N]); y_vec as mx_y_vec says, which every slice keeps when N % 4 == 0
template <int FA, int FB, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_bmm_kernel(const uint8_t* __restrict__ a_codes, const uint8_t* __restrict__ a_scales,
                                                             const uint8_t* __restrict__ b_codes, const uint8_t* __restrict__ b_scales,
                                                             const float* __restrict__ bias, int64_t bias_stride, void* __restrict__ y,
                                                             int ydt, int64_t M, int64_t N, int64_t K, int tiles, int tiles_n, int y_vec) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxTileLds<FA, FB>];
    const int tid = threadIdx.x, wave = tid >> 6;
    const MxbBlock blk(tiles, tiles_n);
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;          // this wave's 64 x 64 corner of the tile
    const int64_t nkb = (K + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    MxbOperand A(a_codes + blk.g * M * K, a_scales + blk.g * M * nkb, M, K, blk.m0, wm, tid);
    MxbOperand B(b_codes + blk.g * N * K, b_scales + blk.g * N * nkb, N, K, blk.n0, wn, tid);
    f32x4 acc[4][4];
    mx_zero(acc);
    mx_tile_loop<FA, FB, VEC>(acc, A, B, 0, (K + kMxgK - 1) / kMxgK, lds, tid, wm, wn);
    mx_epilogue(acc, bias ? bias + blk.g * bias_stride : nullptr, (uint8_t*)y + blk.g * M * N * (ydt == QS_F32 ? 4 : 2), ydt, M, N,
                blk.m0 + wm, blk.n0 + wn, tid & 63, y_vec);
}

// the same loop in front of mx_epilogue_codes: out_codes [G, M, N] and out_scales [G, M, ceil(N / 32)] instead of y
template <int FA, int FB, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_bmm_q_kernel(const uint8_t* __restrict__ a_codes, const uint8_t* __restrict__ a_scales,
                                                               const uint8_t* __restrict__ b_codes, const uint8_t* __restrict__ b_scales,
                                                               const float* __restrict__ bias, int64_t bias_stride, int relu, MxFormat f,
                                                               uint8_t* __restrict__ out_codes, uint8_t* __restrict__ out_scales, int64_t M,
                                                               int64_t N, int64_t K, int tiles, int tiles_n, int c_vec) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxTileLds<FA, FB>];
    const int tid = threadIdx.x, wave = tid >> 6;
    const MxbBlock blk(tiles, tiles_n);
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int64_t nkb = (K + QS_MX_BLOCK - 1) / QS_MX_BLOCK, nnb = (N + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    MxbOperand A(a_codes + blk.g * M * K, a_scales + blk.g * M * nkb, M, K, blk.m0, wm, tid);
    MxbOperand B(b_codes + blk.g * N * K, b_scales + blk.g * N * nkb, N, K, blk.n0, wn, tid);
    f32x4 acc[4][4];
    mx_zero(acc);
    mx_tile_loop<FA, FB, VEC>(acc, A, B, 0, (K + kMxgK - 1) / kMxgK, lds, tid, wm, wn);
    mx_epilogue_codes(acc, bias ? bias + blk.g * bias_stride : nullptr, relu, f, out_codes + blk.g * M * N, out_scales + blk.g * M * nnb, M,
                      N, blk.m0 + wm, blk.n0 + wn, tid & 63, c_vec);
}

}  // namespace qs

// ---- host side, shared by api_mx_bmm.hip and api_mx_bmm_q.hip (Args: qs_mx_bmm_args or qs_mx_bmm_q_args).  Internal linkage ----------
namespace {

// the operands and extents, all QS_ERR_ARG: mx_gemm_check_operands and what the slices add
template <class Args>
int mx_bmm_check_operands(const Args& a) {
    if (mx_gemm_check_operands(a) != QS_OK || a.G < 0) return QS_ERR_ARG;
    return a.bias_batch_stride == 0 || a.bias_batch_stride == a.N ? QS_OK : QS_ERR_ARG;
}

// A slice of this many tiles or more fills the GPU by itself (two co-resident work-groups on each of 256 CUs): qs_mx_bmm_v and
// qs_mx_bmm_q_v then launch the slices one by one through qs_mx_matmul_v / qs_mx_matmul_q_v -- G launches from one call, the bits of the
// batched kernel by definition -- as the 1 x 1 convolution is forwarded (QS_MX_CONV_ROUTE_GEMM).  Measured on 8 slices of 1024 tiles
// the batched kernel took 1.15 - 1.88 x the time of those launches, for a reason that is not found; below the threshold
// one launch is what pays (3072 slices of 4 tiles: 1 / 130 or less of the launches' time).
constexpr int64_t kMxbForwardTiles = 512;

template <class Args>
bool mx_bmm_forwards(const Args& a) {
    return mx_tiles(a.M) * mx_tiles(a.N) >= kMxbForwardTiles;
}

// after them, for a product that is not empty: QS_MX_GEMM_ROUTE_VEC or _PLAIN, or QS_ERR_ARG.  K % 16 == 0 makes M K and N K
// multiples of 16, so aligned bases align every slice
template <class Args>
int mx_bmm_sized_route(const Args& a) {
    const int route = mx_gemm_sized_route(a);      // K == 0, M N / M K / N K beyond INT64_MAX, the tiles of one slice
    if (route < 0) return route;
    if (a.G > INT64_MAX / (a.M * a.K) || a.G > INT64_MAX / (a.N * a.K) || a.G > INT64_MAX / (a.M * a.N)) return QS_ERR_ARG;
    if (a.G > kMaxGrid / (mx_tiles(a.M) * mx_tiles(a.N))) return QS_ERR_ARG;
    return route;
}

}  // namespace
