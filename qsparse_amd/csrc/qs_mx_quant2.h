// Two-way, codes-only MX quantizer (include/qsparse_hip.h, "MX two-way quantizer"): x [R, C] is read ONCE and leaves as
//   row pair  codes [R, C] / scales [R, ceil(C / 32)], blocks along C, format `fr`
//   col pair  codes [C, R] / scales [C, ceil(R / 32)], blocks along R, format `fc`, stored transposed
// -- the operands the three matrix products of a linear layer's training step need.  The per-element arithmetic is
// qs_mx.h's (mx_scale / mx_round_abs / mx_code); nothing of it is restated here.
//
// A work-group of 256 lanes owns a tile of 128 rows x 64 columns (both multiples of 32: every block of either direction lies
// inside one tile).
//   Phase 1, lanes along C: a lane holds V = 8 (two-byte inputs) or 4 (float32) consecutive elements of a row -- one 16-byte load
//     on the VEC route -- in 128 * 64 / (256 * V) passes whose loads are all issued before the first use.  The raw elements go to
//     the LDS tile [128][64] unchanged (one 16-byte store per lane and pass: 8 contiguous lanes cover 32 consecutive dwords, no
//     bank is hit twice); a row block is 32 / V adjacent lanes, its maximum two or three __shfl_xor steps, as mx_inner_vec_kernel.
//   Phase 2, lanes along C again, a lane WALKS along R: lane (c = tid & 63, b = tid >> 6) reads the 32 elements tile[32 b + j][c],
//     j = 0..31 -- a whole column block, so its maximum needs no exchange.  Each read instruction of a 32-lane half addresses 32
//     consecutive columns of one tile row: 32 consecutive dwords (float32) or 16 (two-byte: two lanes per dword), conflict-free with
//     the UNPADDED row pitch, because the transposition happens in registers, not in the addressing.  The lane packs its 32 codes
//     into two 16-byte stores at col_codes[c][r0 + 32 b ..]: the four waves of the group write 128 contiguous bytes per output row.
// No atomics, no workspace; a null pair skips its phase (wave-uniform), a null col pair also the LDS traffic and the barrier.
// VEC = false is the same tiling with element accesses, each predicated on its own index: any R, C >= 1, any element-aligned base.
// mx_quant2_batched_kernel (at the end) is the same tile for G strided slices of x and dense batched outputs, one launch.
// SR = true rounds stochastically (qs_mx.h): the row pair draws its words at stream 0 and index gr * C + gc of row_codes, the col pair
// at stream 1 and index oc * R + orow of col_codes.  On the VEC route both indices are multiples of 4 at a lane's first code, so a
// Philox call serves four codes: V / 4 calls per lane and pass in phase 1, eight per lane in phase 2.  PLAIN spends a call per code.
#pragma once
#include <type_traits>

#include "qs_mx.h"

namespace qs {

constexpr int kMxq2Rows = 128, kMxq2Cols = 64, kMxq2Threads = 256;

template <int XDT>
struct Mxq2Raw {
    using type = uint16_t;
};
template <>
struct Mxq2Raw<QS_F32> {
    using type = uint32_t;
};

template <int XDT>
__device__ __forceinline__ float mxq2_widen(typename Mxq2Raw<XDT>::type raw) {
    if constexpr (XDT == QS_F32) return __uint_as_float(raw);
    if constexpr (XDT == QS_BF16) return bf16_bits_to_f32(raw);
    return f16_bits_to_f32(raw);
}

__device__ __forceinline__ uint32_t mxq2_pack4(const uint32_t* c) { return c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24); }

// ---- what every kernel on this tile shares (this file, qs_mx_glu_bwd.h, qs_mx_norm.h, qs_mx_softmax_train.h, qs_mx_rope.h; the loads
// also qs_mx_norm_bwd.h): all that happens once a value is a float, and phase 1's own steps further down (3z) ----
// the maximum of `am` over the LPB adjacent lanes of a row block
template <int LPB>
__device__ __forceinline__ uint32_t mxq2_block_max(uint32_t am) {
#pragma unroll
    for (int off = 1; off < LPB; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)am, off, 64);
        am = o > am ? o : am;
    }
    return am;
}

// N values under one scale to N codes.  SR draws the words of `stream` at index .. index + N - 1 (sr.base included): QUAD -- index
// and N are multiples of 4 -- with one Philox call per four codes, otherwise with one per code.  SR = false draws nothing.
template <int N, bool SR, bool QUAD>
__device__ __forceinline__ void mx_encode_run(const float (&v)[N], MxScale s, MxFormat f, MxSrKey key,
                                              uint32_t stream, uint64_t index, uint32_t (&c)[N]) {
    if constexpr (SR && QUAD) {
#pragma unroll
        for (int q = 0; q < N; q += 4) {
            uint32_t w[4];
            mx_sr_words4(key, stream, index + q, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t sg;
                const float r = mx_round_abs_sr(v[q + j], s, f, w[j], sg);
                c[q + j] = mx_code(r, sg, s, f);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            uint32_t sg;
            float r;
            if constexpr (SR) r = mx_round_abs_sr(v[j], s, f, mx_sr_word(key, stream, index + j), sg);
            else r = mx_round_abs(v[j], s, f, sg);
            c[j] = mx_code(r, sg, s, f);
        }
    }
}

// phase 1's code store at out = row_codes + gr * C + gc: one store of V = 4 or 8 bytes when `vec` (out is aligned to V), else byte
// stores.  FULL: the lane's V columns are inside together (the VEC route; the GLU tile); otherwise each is predicated on gc + j < C.
template <int V, bool FULL>
__device__ __forceinline__ void mxq2_store_row(uint8_t* out, const uint32_t (&c)[V], bool vec, int64_t gc, int64_t C) {
    if (vec) {
        if constexpr (V == 8) *(u32x2*)out = u32x2{mxq2_pack4(c), mxq2_pack4(c + 4)};
        else *(uint32_t*)out = mxq2_pack4(c);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (FULL || gc + j < C) out[j] = (uint8_t)c[j];
    }
}

// ---- phase 1 of the kernels on this tile: the kernels state their loads' operands and the arithmetic between load and
// emit; the load of a lane's four elements, the staging store, the row-pair emit and the slice decode stand here once.  (The softmax
// kernels and the norm kernel's emit keep a text of their own: measured slower, or another occupancy step, on these.) ----
// the lane's four consecutive elements at p + e (in elements of DT), column gc of a row, as raw bits: those below `lim` of a row that
// exists (`row`); the others are 0 and are not loaded.  VEC: gc % 4 == 0 and the four are in memory together -- one non-temporal load
// of 16 (float32) or 8 bytes under `gc < lim`; otherwise four element loads, each under `gc + j < lim`
template <int DT, bool VEC>
__device__ __forceinline__ void mxq2_load4(const void* __restrict__ p, int64_t e, bool row, int64_t gc, int64_t lim,
                                           typename Mxq2Raw<DT>::type (&raw)[4]) {
    using raw_t = typename Mxq2Raw<DT>::type;
    if constexpr (VEC && DT == QS_F32) {
        u32x4 a = {0u, 0u, 0u, 0u};
        if (row && gc < lim) a = ld16<true>((const u32x4*)((const raw_t*)p + e));
#pragma unroll
        for (int j = 0; j < 4; ++j) raw[j] = a[j];
    } else if constexpr (VEC) {
        u32x2 a = {0u, 0u};
        if (row && gc < lim) a = __builtin_nontemporal_load((const u32x2*)((const raw_t*)p + e));
#pragma unroll
        for (int j = 0; j < 4; ++j) raw[j] = (raw_t)(a[j >> 1] >> ((j & 1) * 16));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) raw[j] = (row && gc + j < lim) ? ((const raw_t*)p)[e + j] : (raw_t)0;
    }
}

// the same four, widened at once
template <int DT, bool VEC>
__device__ __forceinline__ void mxq2_load4f(const void* __restrict__ p, int64_t e, bool row, int64_t gc, int64_t lim, float (&out)[4]) {
    typename Mxq2Raw<DT>::type raw[4];
    mxq2_load4<DT, VEC>(p, e, row, gc, lim, raw);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = mxq2_widen<DT>(raw[j]);
}

// a lane's V floats into the float tile [128][64] at tile row `trow`, column `lcol`: 16-byte stores
template <int V>
__device__ __forceinline__ void mxq2_stage(float* tile, int trow, int lcol, const float (&y)[V]) {
#pragma unroll
    for (int j = 0; j < V; j += 4)
        *(u32x4*)(tile + trow * kMxq2Cols + lcol + j) =
            u32x4{__float_as_uint(y[j]), __float_as_uint(y[j + 1]), __float_as_uint(y[j + 2]), __float_as_uint(y[j + 3])};
}

// The row pair of one pass: the lane's V values `y` of row gr from column gc on -- a row block is the 32 / V adjacent lanes -- to the
// block's scale byte (stored by its first lane) and the lane's V codes.  `index`: the absolute index of the lane's first code in
// stream 0 (sr.base included; unused without SR).  FULL, `row_vec`: mxq2_store_row's; QUAD: mx_encode_run's.  Every lane of the block
// must call it (the maximum is a shuffle); what lies outside [R, C] is not stored.
template <int V, bool VEC, bool FULL, bool SR, bool QUAD>
__device__ __forceinline__ void mxq2_emit_row(const float (&y)[V], MxFormat fr, uint8_t* __restrict__ row_codes,
                                              uint8_t* __restrict__ row_scales, int64_t gr, int64_t gc, int64_t R, int64_t C, int64_t nbc,
                                              int row_vec, MxSrKey key, uint64_t index) {
    constexpr int LPB = QS_MX_BLOCK / V;                  // lanes per row block
    uint32_t am = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const uint32_t a = mx_abs_bits(y[j]);
        am = a > am ? a : am;
    }
    const MxScale s = mx_scale(mxq2_block_max<LPB>(am), fr);
    uint32_t c[V];
    mx_encode_run<V, SR, QUAD>(y, s, fr, key, 0u, index, c);
    if (gr < R && gc < C) {
        if ((threadIdx.x % LPB) == 0) row_scales[gr * nbc + (gc >> 5)] = (uint8_t)s.byte;
        mxq2_store_row<V, FULL>(row_codes + gr * C + gc, c, VEC && row_vec, gc, C);
    }
}

// Where the tile of this block lies, for the kernels that fold G slices into the linear block index as mx_bmm_kernel does (gridDim.y
// stops at 65535):  block = g * tiles + tile,  tile = tile_r * tiles_c + tile_c,  tiles = tiles_r * tiles_c per slice
struct Mxq2At {
    int64_t g, r0, c0;                                    // slice, first row and column inside the slice
};
__device__ __forceinline__ Mxq2At mxq2_at(int tiles, int tiles_c) {
    const unsigned t = blockIdx.x % (unsigned)tiles;
    return Mxq2At{(int64_t)(blockIdx.x / (unsigned)tiles), (int64_t)(t / (unsigned)tiles_c) * kMxq2Rows,
                  (int64_t)(t % (unsigned)tiles_c) * kMxq2Cols};
}

// the four output pointers moved to slice g of the dense outputs [G, R, C] / [G, C, R]; a null pair stays null
__device__ __forceinline__ void mxq2_to_slice(int64_t g, int64_t R, int64_t C, uint8_t* __restrict__& row_codes,
                                              uint8_t* __restrict__& row_scales, uint8_t* __restrict__& col_codes,
                                              uint8_t* __restrict__& col_scales) {
    const int64_t nbc = (C + QS_MX_BLOCK - 1) / QS_MX_BLOCK, nbr = (R + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    if (row_codes) row_codes += g * R * C;
    row_scales += g * R * nbc;
    if (col_codes) col_codes += g * C * R;
    col_scales += g * C * nbr;
}

// Phase 2, after the barrier: lane (cc = tid & 63, cb = tid >> 6) walks the column block tile[32 cb .. 32 cb + 31][cc] and writes its
// 32 codes and its scale byte into the transposed col pair.  The tile holds raw elements of type XDT, or floats (widened by nothing).
// `col_vec`: R % 16 == 0 and col_codes is 16-byte aligned, so each half of the block is inside or outside as a whole and leaves as one
// 16-byte store; a constant `true` where the VEC route guarantees it.  SR && VEC: orow % 32 == 0 and R % 4 == 0, so eight Philox
// calls serve the lane's 32 codes.  `base` is sr.base.
template <int XDT, bool VEC, bool SR, typename T>
__device__ __forceinline__ void mxq2_col_phase(const T* tile, MxFormat fc, uint8_t* __restrict__ col_codes,
                                               uint8_t* __restrict__ col_scales, int64_t R, int64_t C, int64_t r0, int64_t c0, int64_t nbr,
                                               bool col_vec, MxSrKey key, uint64_t base) {
    const int tid = threadIdx.x;
    const int cc = tid & (kMxq2Cols - 1), cb = tid / kMxq2Cols;
    const int64_t oc = c0 + cc, orow = r0 + cb * QS_MX_BLOCK;
    float w[QS_MX_BLOCK];
    uint32_t am = 0;
#pragma unroll
    for (int j = 0; j < QS_MX_BLOCK; ++j) {
        if constexpr (std::is_same<T, float>::value) w[j] = tile[(cb * QS_MX_BLOCK + j) * kMxq2Cols + cc];
        else w[j] = mxq2_widen<XDT>(tile[(cb * QS_MX_BLOCK + j) * kMxq2Cols + cc]);
        const uint32_t a = mx_abs_bits(w[j]);
        am = a > am ? a : am;
    }
    if (oc >= C || orow >= R) return;
    const MxScale s = mx_scale(am, fc);
    col_scales[oc * nbr + (orow >> 5)] = (uint8_t)s.byte;
    uint32_t c[QS_MX_BLOCK];
    mx_encode_run<QS_MX_BLOCK, SR, VEC>(w, s, fc, key, 1u, base + (uint64_t)(oc * R + orow), c);
    uint8_t* out = col_codes + oc * R + orow;
    if (VEC && col_vec) {
        *(u32x4*)out = u32x4{mxq2_pack4(c), mxq2_pack4(c + 4), mxq2_pack4(c + 8), mxq2_pack4(c + 12)};
        if (orow + 16 < R) *(u32x4*)(out + 16) = u32x4{mxq2_pack4(c + 16), mxq2_pack4(c + 20), mxq2_pack4(c + 24), mxq2_pack4(c + 28)};
    } else {
#pragma unroll
        for (int j = 0; j < QS_MX_BLOCK; ++j)
            if (orow + j < R) out[j] = (uint8_t)c[j];
    }
}

// The tile's two phases as a function of the bases and the row pitch of x: the tile at (r0, c0) of x [R, C] whose row r begins at
// x + r * pitch.  mx_quant2_batched_kernel calls it with ONE SLICE's x, outputs, R and C and the slice's row stride, mx_quant2_kernel
// with the whole tensor and pitch = C.  Only the loads (16 bytes per lane, the raw LDS tile) are the tile's own; the row pair is
// mxq2_emit_row, phase 2 mxq2_col_phase.
// `row_vec`: row_codes is aligned to the V bytes a lane stores at once (VEC only; otherwise byte stores).  `sr.base` is the index of
// the pairs' first code: index_base, plus g R C for slice g.
template <int XDT, bool VEC, bool SR>
__device__ __forceinline__ void mxq2_tile(MxFormat fr, MxFormat fc, const void* __restrict__ x, int64_t pitch,
                                          uint8_t* __restrict__ row_codes, uint8_t* __restrict__ row_scales,
                                          uint8_t* __restrict__ col_codes, uint8_t* __restrict__ col_scales, int64_t R, int64_t C,
                                          int64_t r0, int64_t c0, int row_vec, MxSr sr) {
    using raw_t = typename Mxq2Raw<XDT>::type;
    constexpr int V = XDT == QS_F32 ? 4 : 8;              // elements per lane and pass: 16 bytes
    constexpr int LPR = kMxq2Cols / V;                    // lanes per tile row
    constexpr int RPP = kMxq2Threads / LPR;               // tile rows per pass
    constexpr int PASSES = kMxq2Rows / RPP;
    __shared__ __attribute__((aligned(16))) raw_t tile[kMxq2Rows * kMxq2Cols];

    const int tid = threadIdx.x;
    const int64_t nbc = (C + QS_MX_BLOCK - 1) / QS_MX_BLOCK, nbr = (R + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    MxSrKey key = {0u, 0u};
    if constexpr (SR) key = mx_sr_key(sr);

    // ---- phase 1: load, stage, row pair --------------------------------------------------------------------------------------
    const int lrow = tid / LPR, lcol = (tid % LPR) * V;
    const int64_t gc = c0 + lcol;
    raw_t raw[PASSES][V];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int64_t gr = r0 + p * RPP + lrow;
        if constexpr (VEC) {                              // (C % V == 0: the lane's V elements are inside or outside together)
            u32x4 a = {0u, 0u, 0u, 0u};
            if (gr < R && gc < C) a = ld16<true>((const u32x4*)((const raw_t*)x + gr * pitch + gc));
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if constexpr (XDT == QS_F32) raw[p][j] = a[j];
                else raw[p][j] = (raw_t)(a[j >> 1] >> ((j & 1) * 16));
            }
            if (col_codes) *(u32x4*)(tile + (p * RPP + lrow) * kMxq2Cols + lcol) = a;
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                raw[p][j] = (gr < R && gc + j < C) ? ((const raw_t*)x)[gr * pitch + gc + j] : (raw_t)0;
                if (col_codes) tile[(p * RPP + lrow) * kMxq2Cols + lcol + j] = raw[p][j];
            }
        }
    }
    if (row_codes) {
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int64_t gr = r0 + p * RPP + lrow;
            float v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = mxq2_widen<XDT>(raw[p][j]);
            // (VEC: C % V == 0, gc % V == 0: the lane's first index is a multiple of 4)
            mxq2_emit_row<V, VEC, VEC, SR, VEC>(v, fr, row_codes, row_scales, gr, gc, R, C, nbc, row_vec, key,
                                                sr.base + (uint64_t)(gr * C + gc));
        }
    }
    if (!col_codes) return;                               // (kernel-uniform)
    __syncthreads();
    mxq2_col_phase<XDT, VEC, SR>(tile, fc, col_codes, col_scales, R, C, r0, c0, nbr, true, key, sr.base);
}

// The 2-d kernel is the tile at pitch = C: there is ONE text of the two phases.  The phase-2 text and the encode step are shared with
// mx_glu_bwd_quant2_kernel and mx_norm_apply_kernel as mxq2_col_phase and mx_encode_run; those kernels keep their phase-1 loads.
// Measured (profiles/mx_quant2_share.json): no instantiation is the former text's instruction for instruction -- the
// scheduler orders the same work differently -- so each was timed against the parent in alternating fresh processes; every case of
// the four benchmarks stayed inside the parent's own band or 1 %.  DESIGN 3l's 1.5 - 2.8 % miss of this merge did not reproduce
// (-1.0 .. +0.4 % here, the 2-d kernel's twelve instantiations 0 - 56 instructions shorter than their former text).
// `row_vec`: row_codes is aligned to the V bytes a lane stores at once (VEC only; otherwise byte stores)
template <int XDT, bool VEC, bool SR>
__global__ __launch_bounds__(kMxq2Threads) void mx_quant2_kernel(MxFormat fr, MxFormat fc, const void* __restrict__ x,
                                                                 uint8_t* __restrict__ row_codes, uint8_t* __restrict__ row_scales,
                                                                 uint8_t* __restrict__ col_codes, uint8_t* __restrict__ col_scales,
                                                                 int64_t R, int64_t C, int tiles_c, int row_vec, MxSr sr) {
    mxq2_tile<XDT, VEC, SR>(fr, fc, x, C, row_codes, row_scales, col_codes, col_scales, R, C, (int64_t)(blockIdx.x / tiles_c) * kMxq2Rows,
                            (int64_t)(blockIdx.x % tiles_c) * kMxq2Cols, row_vec, sr);
}

// The batched, strided form (include/qsparse_hip.h, "MX batched two-way quantizer"): G = G0 G1 slices [R, C] of x, slice g = g0 G1 +
// g1 at x + g0 sg0 + g1 sg1 with the row pitch `pitch` (all in elements), dense outputs [G, R, C] / [G, C, R].  One work-group per tile
// per slice, the slice folded into the linear block index (mxq2_at).  A tile lies inside one slice and mxq2_tile predicates on that slice's R and C: no block spans two slices, nothing of slice g + 1
// is read for the short last block of slice g.  The random word of a code is indexed in the whole dense output: base + g R C.
template <int XDT, bool VEC, bool SR>
__global__ __launch_bounds__(kMxq2Threads) void mx_quant2_batched_kernel(MxFormat fr, MxFormat fc, const void* __restrict__ x,
                                                                         int64_t G1, int64_t sg0, int64_t sg1, int64_t pitch,
                                                                         uint8_t* __restrict__ row_codes, uint8_t* __restrict__ row_scales,
                                                                         uint8_t* __restrict__ col_codes, uint8_t* __restrict__ col_scales,
                                                                         int64_t R, int64_t C, int tiles, int tiles_c, int row_vec, MxSr sr) {
    using raw_t = typename Mxq2Raw<XDT>::type;
    const Mxq2At at = mxq2_at(tiles, tiles_c);
    mxq2_to_slice(at.g, R, C, row_codes, row_scales, col_codes, col_scales);
    sr.base += (uint64_t)(at.g * R * C);
    mxq2_tile<XDT, VEC, SR>(fr, fc, (const raw_t*)x + (at.g / G1) * sg0 + (at.g % G1) * sg1, pitch, row_codes, row_scales, col_codes,
                            col_scales, R, C, at.r0, at.c0, row_vec, sr);
}

}  // namespace qs
