// Grouped (ragged) matrix product on MX codes (include/qsparse_hip.h, "MX grouped matrix product"): the rows of A [T, K] are E
// consecutive groups whose END rows lie in DEVICE memory (`offs` [E] int32, cumulative), group e multiplied by its own weight
// B[e] [N, K] -- the expert layers of a mixture-of-experts block after routing.  The rows of group e are bit for bit what
// mx_gemm_kernel (qs_mx_gemm.h) writes for them with the weight B[e]: the same 128 x 128 tile, the same walk along K in steps of
// 128, the same 16 MFMAs per step in the same order, the same epilogue -- it is mx_tile_loop over MxbOperand (qs_mx_bmm.h), which
// takes an absolute first row and an absolute row bound, in front of mx_epilogue / mx_epilogue_codes, which take them too.
//
// Boundaries (normative, the header's): c_-1 = 0, c_e = min(max(offs[e], c_{e-1}), T); group e is the rows [c_{e-1}, c_e).  With the
// running maximum and the clamp the groups partition [0, c_{E-1}) for ANY content of offs, so every row is stored exactly once and no
// address outside the operands is formed.  The rows [c_{E-1}, T) belong to no group: the pseudo-group E, which has no weight and no
// K loop -- its accumulators stay zero and go through the same epilogue without a bias (+0; code 0 and scale byte 0).
//
// Index decode.  M-tiles are group-relative: tile t of group e starts at row c_{e-1} + 128 t and is bounded by c_e, so no tile holds
// rows of two groups.  The host cannot know how many there are; the grid is the bound mt_max = floor((T + 127 (E + 1)) / 128) times
// tiles_n (each of the E + 1 ranges wastes less than one tile), tiles_n the fastest index so that the tiles of one group are adjacent
// and its weight stays in L2:
//   block = mt * tiles_n + tile_n
// Every work-group walks offs once from the front, accumulating c_e and the tile count, until the group that holds its mt is found
// (MxgmBlock).  The walk is uniform across the work-group: the addresses depend on kernel arguments alone, so the loads are scalar
// loads, eight entries per round trip (indices past E - 1 re-read entry E - 1, which the running maximum turns into empty groups
// that own no tile), and the arithmetic is 32-bit SALU -- offs is int32, so the boundaries are clamped to min(T, INT32_MAX) and only
// the tail needs T itself.  A work-group whose mt is not below the real total returns before any barrier.  No workspace, no second
// launch.
#pragma once
#include "qs_mx_bmm.h"

namespace qs {

constexpr int kMxgmChunk = 8;      // entries of offs per round of the decode

// what both grouped kernels decode from the block index and offs: the group (E: the tail), its rows [lo, hi), the tile's corner
struct MxgmBlock {
    int group;                     // -1: this work-group owns no tile
    int64_t hi, m0, n0;

    __device__ __forceinline__ MxgmBlock(const int32_t* __restrict__ offs, int E, int64_t T, int tiles_n) {
        uint32_t rem = blockIdx.x / (unsigned)tiles_n;              // M-tiles still in front of this one
        n0 = (int64_t)(blockIdx.x % (unsigned)tiles_n) * kMxgTile;
        const int32_t cap = (int32_t)(T < (int64_t)INT32_MAX ? T : (int64_t)INT32_MAX);
        int32_t c = 0, lo = 0, end = 0;
        group = -1;
        for (int e0 = 0; e0 < E && group < 0; e0 += kMxgmChunk) {
            int32_t v[kMxgmChunk];
#pragma unroll
            for (int i = 0; i < kMxgmChunk; ++i) v[i] = offs[e0 + i < E ? e0 + i : E - 1];
            // all eight in scalar registers here: without this the compiler sinks each load behind the test of the entry before
            // it, one round trip to the scalar cache per group instead of one per eight
            asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]));
#pragma unroll
            for (int i = 0; i < kMxgmChunk; ++i) {
                int32_t ce = v[i] > c ? v[i] : c;
                ce = ce < cap ? ce : cap;
                const uint32_t nt = ((uint32_t)(ce - c) + (kMxgTile - 1)) / kMxgTile;
                const bool hit = group < 0 && rem < nt;
                lo = hit ? c : lo, end = hit ? ce : end, group = hit ? e0 + i : group;
                rem -= group < 0 ? nt : 0u;
                c = ce;
            }
        }
        hi = end;
        if (group < 0 && (int64_t)rem < (T - c + (kMxgTile - 1)) / kMxgTile) group = E, lo = c, hi = T;       // the tail
        m0 = (int64_t)lo + (int64_t)rem * kMxgTile;
    }
};

// bias_stride: 0 (one [N] bias for every group) or N ([E, N]); y_vec as mx_y_vec says, which every row keeps when N % 4 == 0
template <int FA, int FB, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_gmm_kernel(const uint8_t* __restrict__ a_codes, const uint8_t* __restrict__ a_scales,
                                                             const uint8_t* __restrict__ b_codes, const uint8_t* __restrict__ b_scales,
                                                             const float* __restrict__ bias, int64_t bias_stride,
                                                             const int32_t* __restrict__ offs, void* __restrict__ y, int ydt, int64_t T,
                                                             int E, int64_t N, int64_t K, int tiles_n, int y_vec) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxTileLds<FA, FB>];
    const MxgmBlock blk(offs, E, T, tiles_n);
    if (blk.group < 0) return;                                      // (uniform, before any barrier)
    const int tid = threadIdx.x, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;          // this wave's 64 x 64 corner of the tile
    f32x4 acc[4][4];
    mx_zero(acc);
    const float* gbias = nullptr;
    if (blk.group < E) {
        const int64_t nkb = (K + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
        MxbOperand A(a_codes, a_scales, blk.hi, K, blk.m0, wm, tid);
        MxbOperand B(b_codes + blk.group * N * K, b_scales + blk.group * N * nkb, N, K, blk.n0, wn, tid);
        mx_tile_loop<FA, FB, VEC>(acc, A, B, 0, (K + kMxgK - 1) / kMxgK, lds, tid, wm, wn);
        gbias = bias ? bias + blk.group * bias_stride : nullptr;
    }
    mx_epilogue(acc, gbias, y, ydt, blk.hi, N, blk.m0 + wm, blk.n0 + wn, tid & 63, y_vec);
}

// the same decode and loop in front of mx_epilogue_codes: out_codes [T, N] and out_scales [T, ceil(N / 32)] instead of y
template <int FA, int FB, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_gmm_q_kernel(const uint8_t* __restrict__ a_codes, const uint8_t* __restrict__ a_scales,
                                                               const uint8_t* __restrict__ b_codes, const uint8_t* __restrict__ b_scales,
                                                               const float* __restrict__ bias, int64_t bias_stride,
                                                               const int32_t* __restrict__ offs, int relu, MxFormat f,
                                                               uint8_t* __restrict__ out_codes, uint8_t* __restrict__ out_scales, int64_t T,
                                                               int E, int64_t N, int64_t K, int tiles_n, int c_vec) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxTileLds<FA, FB>];
    const MxgmBlock blk(offs, E, T, tiles_n);
    if (blk.group < 0) return;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    f32x4 acc[4][4];
    mx_zero(acc);
    const float* gbias = nullptr;
    if (blk.group < E) {
        const int64_t nkb = (K + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
        MxbOperand A(a_codes, a_scales, blk.hi, K, blk.m0, wm, tid);
        MxbOperand B(b_codes + blk.group * N * K, b_scales + blk.group * N * nkb, N, K, blk.n0, wn, tid);
        mx_tile_loop<FA, FB, VEC>(acc, A, B, 0, (K + kMxgK - 1) / kMxgK, lds, tid, wm, wn);
        gbias = bias ? bias + blk.group * bias_stride : nullptr;
    }
    mx_epilogue_codes(acc, gbias, relu, f, out_codes, out_scales, blk.hi, N, blk.m0 + wm, blk.n0 + wn, tid & 63, c_vec);
}

}  // namespace qs

// ---- host side, shared by api_mx_gmm.hip and api_mx_gmm_q.hip (Args: qs_mx_grouped_matmul_args or qs_mx_grouped_matmul_q_args).
// Internal linkage.  offs is never read here ---------------------------------------------------------------------------------------
namespace {

// the operands and extents, all QS_ERR_ARG.  Without groups (E == 0) there is no weight and no offs: they may be NULL
template <class Args>
int mx_gmm_check_operands(const Args& a) {
    if (!a.a_codes || !a.a_scales) return QS_ERR_ARG;
    if (!mx_format_ok(a.a_format) || !mx_format_ok(a.b_format)) return QS_ERR_ARG;
    if (a.T < 0 || a.N < 0 || a.K < 0 || a.E < 0 || a.E > QS_MX_GROUPED_MAX_GROUPS) return QS_ERR_ARG;
    if (a.E > 0 && (!a.b_codes || !a.b_scales || !a.offs)) return QS_ERR_ARG;
    return a.bias_batch_stride == 0 || a.bias_batch_stride == a.N ? QS_OK : QS_ERR_ARG;
}

// the grid's bound on the M-tiles: each of the E groups and the tail wastes less than one tile
template <class Args>
int64_t mx_gmm_mt_max(const Args& a) {
    return (a.T + (kMxgTile - 1) * (a.E + 1)) / kMxgTile;
}

// after them, for a product that is not empty (T, N > 0): QS_MX_GEMM_ROUTE_VEC or _PLAIN, or QS_ERR_ARG.  K % 16 == 0 makes every row
// and every N K a multiple of 16, so aligned bases align every group's rows and every weight
template <class Args>
int mx_gmm_sized_route(const Args& a) {
    if (a.K == 0 || a.T > INT64_MAX / a.K || a.N > INT64_MAX / a.K || a.T > INT64_MAX / a.N) return QS_ERR_ARG;
    if (a.E > INT64_MAX / (a.N * a.K)) return QS_ERR_ARG;
    if (a.T > INT64_MAX - (kMxgTile - 1) * (a.E + 1) || mx_gmm_mt_max(a) > kMaxGrid / mx_tiles(a.N)) return QS_ERR_ARG;
    return (a.K % 16 == 0 && aligned16(a.a_codes) && aligned16(a.b_codes)) ? QS_MX_GEMM_ROUTE_VEC : QS_MX_GEMM_ROUTE_PLAIN;
}

}  // namespace
