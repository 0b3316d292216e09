// mx_kv_append_kernel (qs_mx_kv_append.h) into a PAGED cache (include/qsparse_hip.h, "MX KV cache append, paged"): k_pool [P, Hkv, page,
// d], vt_pool [P, Hkv, dv, page], position j of sequence b in pool page block_table[b, j / page] at row / column j % page; page = 2^lg >=
// 32, so a block of 32 columns never crosses a page.  The three kinds of item, the tile, the barriers and the tail rule are that
// kernel's: kva_len, kva_fill and kva_tail_store are called as they are.  The row item, the block's encode-and-store and the item
// dispatch are stated again with the table lookup in them -- passing "where the rows and blocks lie" into the contiguous kernel's
// functions changed its register allocation, so that kernel stays as it is.
//   row item   looks up the page of ITS row, per lane, after L_b is known and only for a position < S
//   V item     looks up the page of its block (work-group-uniform: one vector load, readfirstlane)
// An entry outside [0, P) ends that store -- the row, or the block's codes and scale bytes -- and nothing else: the tile is still filled
// and v_tail still advanced, as if the token had been stored.  Table reads are vector loads; nothing is written through the scalar path.
#pragma once
#include "qs_mx_kv_append.h"

namespace qs {

struct KvaPagedArgs : KvaArgs {                                 // k_codes .. vt_scales: the pool's; S = NP page; P: the rope tables' rows
    const int32_t* __restrict__ table;                          // [B, NP]
    int pool, NP, lg;                                           // pool pages, pages per sequence, log2(page)
};

// where the cache's rows and blocks lie
struct KvaPaged {
    const KvaPagedArgs& a;
    __device__ __forceinline__ int64_t k_rows() const { return ((int64_t)a.pool * a.Hkv) << a.lg; }
    // the row of k_pool [P Hkv page, d] that holds position pos < S of (b, hk); k_rows(): nowhere (a dead entry)
    __device__ __forceinline__ int64_t k_row(int b, int64_t hk, int pos) const {
        const int e = a.table[(int64_t)b * a.NP + (pos >> a.lg)];
        if (e < 0 || e >= a.pool) return k_rows();
        return (((int64_t)e * a.Hkv + hk) << a.lg) + (pos & ((1 << a.lg) - 1));
    }
    // the block at column c0 < S of (b, hk) = bh: channel 0's line of vt_pool [P Hkv dv, page], the bytes per line, the block's column in
    // its page; false: a dead entry
    __device__ __forceinline__ bool vt_block(int64_t bh, int c0, int64_t& line0, int& pitch, int& col) const {
        const int64_t b = bh / a.Hkv, hk = bh % a.Hkv;
        const int raw = a.table[b * a.NP + (c0 >> a.lg) + (int)__builtin_amdgcn_mbcnt_lo(0u, 0u)];      // (+ 0, in a vector register)
        const int e = __builtin_amdgcn_readfirstlane(raw);
        line0 = ((int64_t)(e < 0 || e >= a.pool ? 0 : e) * a.Hkv + hk) * a.dv, pitch = 1 << a.lg, col = c0 & (pitch - 1);
        return e >= 0 && e < a.pool;
    }
};

// ---- row items: kva_row_item with the row's page looked up ------------------------------------------------------------------------------
template <int XDT, bool VEC>
__device__ __forceinline__ void kvp_row_item(const KvaPagedArgs& a, const MxFormat& fq, const KvaPaged& w) {
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
    const int64_t Rk = w.k_rows(), Rq = (int64_t)a.B * nq;
    const int64_t R = isq ? Rq : Rk;
    int64_t gr = R;
    if (isq) gr = (int64_t)b * nq + hr;
    else if (row_in && L + t < a.S) gr = w.k_row(b, hr / a.T, L + t);
    mxq2_emit_row<V, VEC, VEC, false, false>(y, fq, isq ? a.q_codes : a.k_codes, isq ? a.q_scales : a.k_scales, gr, gc, R, C, nbc, 1,
                                             MxSrKey{0u, 0u}, 0ull);
}

// ---- a block of vt: kva_encode into the block's page ------------------------------------------------------------------------------------
template <bool VEC>
__device__ __forceinline__ void kvp_encode(const float* tile, const KvaPagedArgs& a, const MxFormat& fv, int64_t bh, int c0, const KvaPaged& w) {
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
    int64_t line0;
    int pitch, cb;
    if (!w.vt_block(bh, c0, line0, pitch, cb) || !in) return;
    const int64_t line = line0 + ch;
    const int col = cb + half * 16;
    if (half == 0) a.vt_scales[line * ((pitch + QS_MX_BLOCK - 1) / QS_MX_BLOCK) + (cb >> 5)] = (uint8_t)s.byte;
    uint8_t* out = a.vt_codes + line * pitch + col;
    if constexpr (VEC) {                                        // (S % 16 == 0, vt_codes 16-byte aligned)
        if (col < pitch) *(u32x4*)out = u32x4{mxq2_pack4(c), mxq2_pack4(c + 4), mxq2_pack4(c + 8), mxq2_pack4(c + 12)};
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (col + j < pitch) out[j] = (uint8_t)c[j];
    }
}

// ---- the work-group's item: mx_kv_append_kernel's dispatch ------------------------------------------------------------------------------
template <int XDT, bool VEC>
__global__ __launch_bounds__(kKvaThreads) void mx_kv_append_paged_kernel(MxFormat fq, MxFormat fv, KvaPagedArgs a) {
    __shared__ float tile[QS_MX_BLOCK * kKvaPitch];
    const KvaPaged w{a};
    if (blockIdx.x < a.n_row) {                                 // (work-group-uniform, as every branch below)
        kvp_row_item<XDT, VEC>(a, fq, w);
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
        kvp_encode<VEC>(tile, a, fv, bh, blk * QS_MX_BLOCK, w);
        return;
    }
    kva_fill<XDT, VEC>(tile, a, bh, first * QS_MX_BLOCK, L, Lp);       // (reads the tail)
    __syncthreads();
    kvp_encode<VEC>(tile, a, fv, bh, first * QS_MX_BLOCK, w);
    if (last != first) {
        __syncthreads();                                        // (the tile is free; every read of the tail lies two barriers back)
        kva_fill<XDT, VEC>(tile, a, bh, last * QS_MX_BLOCK, L, Lp);
        __syncthreads();
        kvp_encode<VEC>(tile, a, fv, bh, last * QS_MX_BLOCK, w);
    }
    if (Lp & 31) {                                              // the last block stays open: its new columns go to the tail
        const int c0 = last * QS_MX_BLOCK;
        kva_tail_store(tile, a, bh, L > c0 ? L - c0 : 0, Lp - c0);
    }
}

}  // namespace qs
