// Appending T tokens per sequence to the MX KV cache that mx_flash_decode reads (include/qsparse_hip.h, "MX KV cache append"): k_codes
// [B, Hkv, S, d] with blocks along d, vt_codes [B, Hkv, dv, S] with blocks along S, the write position L_b = clamp(kv_len[b], 0, S) read
// on the device.  ONE launch; the work-group (256 lanes) takes one of three kinds of item by its block index:
//
//   row items   [0, n_row)   sequence b = block / row_groups, `rpg` rows of it: its K rows (hk, t), then its Q rows (hq, t).  A row is
//               `lpr` = ceil(d / 32) * 32 / V adjacent lanes, a lane owns V columns (16 bytes of input: qs_mx_rope.h's RopeLane).  Load
//               (rope_load: the half layout's partner is a second load), rotate in registers by table row min(L_b + t, P - 1)
//               (rope_rotate: never an FMA), block maximum over the 32 / V lanes of a block and encode (mxq2_emit_row) straight to row
//               L_b + t of the cache (K; a row at or past S is not stored) or to the dense q_codes / q_scales (Q).  No LDS, no barrier.
//   edge items  [n_row, n_row + B Hkv)   one per (b, hk): the FIRST and the LAST 32-column block of vt that the append touches.  The
//               first block reads v_tail (the open block's float32 history), the last writes it; for T > 32 - L_b % 32 these are
//               different blocks over the same columns of v_tail, so ONE work-group owns both: tail read -> barrier -> first block ->
//               barrier -> last block -> tail write.
//   mid items   the whole blocks between the two, (b, hk, m): block L_b / 32 + 1 + m, all of it from v_new; an item at or behind the
//               last block ends at once (their count is sized on T, the length is the device's).
//
// A block of vt, all dv channels at once.  Gather into the float LDS tile [32 positions][dv], pitch 129:
//     positions <  L_b   from v_tail [.., dv, 32], lanes along the 32 columns (128 contiguous bytes per channel), transposed by the store
//     positions >= L_b   from v_new [.., T, dv], lanes along dv: V elements (16 bytes) per lane on the VEC route; +0 at or past L'
// The odd pitch keeps the transposing store (lanes 129 floats apart) and the column reads off each other's banks.  After the barrier lane
// 2 c + half reads the 16 values of channel c at positions 16 half .., takes the block maximum with its neighbour (one __shfl_xor),
// encodes (mx_encode_run) and stores 16 code bytes -- one 16-byte store on the VEC route (S % 16 == 0: a half block is inside S or
// outside as a whole), else bytes each predicated on its column -- and half 0 the scale byte.  The pair of lanes writes 32 contiguous
// bytes.  A block that stays open (L' % 32 != 0) then copies its new columns from the tile to v_tail, lanes along the columns again.
// No atomics, no counters, no workspace; nothing is read by the host.
#pragma once
#include "qs_mx_rope.h"

namespace qs {

constexpr int kKvaThreads = 256;
constexpr int kKvaPitch = 4 * QS_MX_BLOCK + 1;                  // floats per tile row: dv <= 128 columns + 1
constexpr int kKvaMaxD = 128;
enum { kKvaPlainRows = 0, kKvaHalf = 1, kKvaInterleaved = 2 };  // KvaArgs::mode

struct KvaArgs {
    const void* __restrict__ k_new;                             // [B, Hkv, T, d]
    const void* __restrict__ v_new;                             // [B, Hkv, T, dv]
    const void* __restrict__ q_new;                             // [B, Hq, T, d] (Hq == 0: none)
    const float* __restrict__ cs;                               // [P, d / 2] (mode != kKvaPlainRows)
    const float* __restrict__ sn;
    const int32_t* __restrict__ kv_len;                         // [B]
    uint8_t* __restrict__ k_codes;
    uint8_t* __restrict__ k_scales;
    uint8_t* __restrict__ vt_codes;
    uint8_t* __restrict__ vt_scales;
    uint8_t* __restrict__ q_codes;
    uint8_t* __restrict__ q_scales;
    float* __restrict__ v_tail;                                 // [B, Hkv, dv, 32]
    int B, Hkv, Hq, T, S, d, dv, P;
    int mode;
    int lpr, rpg, row_groups;                                   // lanes per row, rows per work-group, work-groups per sequence
    int mid;                                                    // mid items per (b, hk)
    unsigned n_row, n_edge;
};

// L_b: one vector load (the address is the lane's own), then wave-uniform
__device__ __forceinline__ int kva_len(const KvaArgs& a, int b) {
    const int raw = a.kv_len[b + (int)__builtin_amdgcn_mbcnt_lo(0u, 0u)];      // (+ 0, in a vector register)
    return __builtin_amdgcn_readfirstlane(raw < 0 ? 0 : (raw > a.S ? a.S : raw));
}

// ---- row items ---------------------------------------------------------------------------------------------------------------------
template <int XDT, bool VEC>
__device__ __forceinline__ void kva_row_item(const KvaArgs& a, const MxFormat& fq) {
    using raw_t = typename Mxq2Raw<XDT>::type;
    constexpr int V = RopeLane<XDT>::V;
    const int b = (int)(blockIdx.x / (unsigned)a.row_groups), grp = (int)(blockIdx.x % (unsigned)a.row_groups);
    const int L = kva_len(a, b);
    const int r = (int)threadIdx.x / a.lpr;
    const int64_t gc = (int64_t)((int)threadIdx.x % a.lpr) * V;
    const int64_t nk = (int64_t)a.Hkv * a.T, nq = (int64_t)a.Hq * a.T;
    const int64_t rr = (int64_t)grp * a.rpg + r;               // the row of sequence b: K rows (hk, t), then Q rows (hq, t)
    const bool row_in = r < a.rpg && rr < nk + nq;
    const bool isq = row_in && rr >= nk;
    const int64_t hr = !row_in ? 0 : (isq ? rr - nk : rr);      // head * T + t (no address is formed from a row that does not exist)
    const int t = (int)(hr % a.T);
    const int64_t C = a.d, h = C >> 1;
    const raw_t* xrow = (isq ? (const raw_t*)a.q_new + (int64_t)b * nq * C : (const raw_t*)a.k_new + (int64_t)b * nk * C) + hr * C;

    float y[V];
    if (a.mode == kKvaPlainRows) {                              // (kernel-uniform)
        if constexpr (VEC) {                                    // (C % V == 0: the lane's V elements are inside or outside together)
            u32x4 w = {0u, 0u, 0u, 0u};
            if (row_in && gc < C) w = ld16<true>((const u32x4*)(xrow + gc));
            rope_unpack<XDT>(w, y);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) y[j] = (row_in && gc + j < C) ? mxq2_widen<XDT>(xrow[gc + j]) : 0.0f;
        }
    } else {
        const int pos = L + t;
        const int64_t tr = pos < a.P ? pos : a.P - 1;           // the table row: min(L_b + t, P - 1)
        RopeLane<XDT> ln;
        if (a.mode == kKvaInterleaved) {
            rope_load<XDT, VEC, true>(ln, xrow, a.cs + tr * h, a.sn + tr * h, gc, C, h, row_in);
            rope_rotate<XDT, true>(ln, gc, h, 0, y);
        } else {
            rope_load<XDT, VEC, false>(ln, xrow, a.cs + tr * h, a.sn + tr * h, gc, C, h, row_in);
            rope_rotate<XDT, false>(ln, gc, h, 0, y);
        }
    }
    // where the row goes: row L_b + t of (b, hk) in the cache [B Hkv S, d] -- nowhere at or past S -- or row (b, hq, t) of q's dense pair
    const int64_t nbc = (C + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    const int64_t Rk = (int64_t)a.B * a.Hkv * a.S, Rq = (int64_t)a.B * nq;
    const int64_t R = isq ? Rq : Rk;
    int64_t gr = R;
    if (isq) gr = (int64_t)b * nq + hr;
    else if (row_in && L + t < a.S) gr = ((int64_t)b * a.Hkv + hr / a.T) * a.S + L + t;
    mxq2_emit_row<V, VEC, VEC, false, false>(y, fq, isq ? a.q_codes : a.k_codes, isq ? a.q_scales : a.k_scales, gr, gc, R, C, nbc, 1,
                                             MxSrKey{0u, 0u}, 0ull);
}

// ---- a block of vt -----------------------------------------------------------------------------------------------------------------
// the tile of the block at column c0 of (b, hk) = bh: positions below L from v_tail, [L, Lp) from v_new, +0 behind
template <int XDT, bool VEC>
__device__ __forceinline__ void kva_fill(float* tile, const KvaArgs& a, int64_t bh, int c0, int L, int Lp) {
    using raw_t = typename Mxq2Raw<XDT>::type;
    constexpr int V = RopeLane<XDT>::V;
    constexpr int CGP = kKvaMaxD / V, RPP = kKvaThreads / CGP;  // lanes per token row, token rows per pass
    const int tid = (int)threadIdx.x;
    const int nt = L - c0 < 0 ? 0 : (L - c0 > QS_MX_BLOCK ? QS_MX_BLOCK : L - c0);       // columns that come from the tail
    {
        const int col = tid & 31;
        if (col < nt) {
            const float* tl = a.v_tail + bh * a.dv * QS_MX_BLOCK + col;
            for (int ch = tid >> 5; ch < a.dv; ch += kKvaThreads / 32) tile[col * kKvaPitch + ch] = tl[(int64_t)ch * QS_MX_BLOCK];
        }
    }
    const int lc = (tid % CGP) * V, pr = tid / CGP;
    const raw_t* vn = (const raw_t*)a.v_new + bh * a.T * a.dv;
    float v[QS_MX_BLOCK / RPP][V];
#pragma unroll
    for (int i = 0; i < QS_MX_BLOCK / RPP; ++i) {               // every load is issued before the first store
        const int p = pr + i * RPP, pos = c0 + p;
        const bool in = p >= nt && pos < Lp && lc < a.dv;
        const raw_t* row = vn + (int64_t)(in ? pos - L : 0) * a.dv;
        if constexpr (VEC) {                                    // (dv % V == 0: the lane's V channels are inside or outside together)
            u32x4 w = {0u, 0u, 0u, 0u};
            if (in) w = ld16<true>((const u32x4*)(row + lc));
            rope_unpack<XDT>(w, v[i]);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) v[i][j] = (in && lc + j < a.dv) ? mxq2_widen<XDT>(row[lc + j]) : 0.0f;
        }
    }
#pragma unroll
    for (int i = 0; i < QS_MX_BLOCK / RPP; ++i) {
        const int p = pr + i * RPP;
        if (p >= nt) {
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (lc + j < a.dv) tile[p * kKvaPitch + lc + j] = v[i][j];
        }
    }
}

// the tile to the codes and scale bytes of the block at column c0
template <bool VEC>
__device__ __forceinline__ void kva_encode(const float* tile, const KvaArgs& a, const MxFormat& fv, int64_t bh, int c0) {
    const int ch = (int)threadIdx.x >> 1, half = (int)threadIdx.x & 1;
    const bool in = ch < a.dv;
    float v[16];
    uint32_t am = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        v[j] = in ? tile[(half * 16 + j) * kKvaPitch + ch] : 0.0f;
        const uint32_t x = mx_abs_bits(v[j]);
        am = x > am ? x : am;
    }
    const MxScale s = mx_scale(mxq2_block_max<2>(am), fv);
    uint32_t c[16];
    mx_encode_run<16, false, false>(v, s, fv, MxSrKey{0u, 0u}, 0u, 0ull, c);
    if (!in) return;
    const int64_t line = bh * a.dv + ch;
    const int col = c0 + half * 16;
    if (half == 0) a.vt_scales[line * ((a.S + QS_MX_BLOCK - 1) / QS_MX_BLOCK) + (c0 >> 5)] = (uint8_t)s.byte;
    uint8_t* out = a.vt_codes + line * a.S + col;
    if constexpr (VEC) {                                        // (S % 16 == 0, vt_codes 16-byte aligned)
        if (col < a.S) *(u32x4*)out = u32x4{mxq2_pack4(c), mxq2_pack4(c + 4), mxq2_pack4(c + 8), mxq2_pack4(c + 12)};
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (col + j < a.S) out[j] = (uint8_t)c[j];
    }
}

// the tile's columns [from, to) to v_tail
__device__ __forceinline__ void kva_tail_store(const float* tile, const KvaArgs& a, int64_t bh, int from, int to) {
    const int col = (int)threadIdx.x & 31;
    if (col < from || col >= to) return;
    float* tl = a.v_tail + bh * a.dv * QS_MX_BLOCK + col;
    for (int ch = (int)threadIdx.x >> 5; ch < a.dv; ch += kKvaThreads / 32) tl[(int64_t)ch * QS_MX_BLOCK] = tile[col * kKvaPitch + ch];
}

template <int XDT, bool VEC>
__global__ __launch_bounds__(kKvaThreads) void mx_kv_append_kernel(MxFormat fq, MxFormat fv, KvaArgs a) {
    __shared__ float tile[QS_MX_BLOCK * kKvaPitch];
    if (blockIdx.x < a.n_row) {                                 // (work-group-uniform, as every branch below)
        kva_row_item<XDT, VEC>(a, fq);
        return;
    }
    const unsigned item = blockIdx.x - a.n_row;
    const bool edge = item < a.n_edge;
    const int64_t bh = edge ? item : (item - a.n_edge) / (unsigned)a.mid;
    const int L = kva_len(a, (int)(bh / a.Hkv));
    const int Lp = L + (a.T < a.S - L ? a.T : a.S - L);         // L': the length after the append
    if (Lp == L) return;                                        // a full cache: nothing is stored
    const int first = L >> 5, last = (Lp - 1) >> 5;
    if (!edge) {
        const int blk = first + 1 + (int)((item - a.n_edge) % (unsigned)a.mid);
        if (blk >= last) return;
        kva_fill<XDT, VEC>(tile, a, bh, blk * QS_MX_BLOCK, L, Lp);
        __syncthreads();
        kva_encode<VEC>(tile, a, fv, bh, blk * QS_MX_BLOCK);
        return;
    }
    kva_fill<XDT, VEC>(tile, a, bh, first * QS_MX_BLOCK, L, Lp);       // (reads the tail)
    __syncthreads();
    kva_encode<VEC>(tile, a, fv, bh, first * QS_MX_BLOCK);
    if (last != first) {
        __syncthreads();                                        // (the tile is free; every read of the tail lies two barriers back)
        kva_fill<XDT, VEC>(tile, a, bh, last * QS_MX_BLOCK, L, Lp);
        __syncthreads();
        kva_encode<VEC>(tile, a, fv, bh, last * QS_MX_BLOCK);
    }
    if (Lp & 31) {                                              // the last block stays open: its new columns go to the tail
        const int c0 = last * QS_MX_BLOCK;
        kva_tail_store(tile, a, bh, L > c0 ? L - c0 : 0, Lp - c0);
    }
}

}  // namespace qs
