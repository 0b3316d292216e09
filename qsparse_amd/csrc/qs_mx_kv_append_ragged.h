// mx_kv_append_paged_kernel (qs_mx_kv_append_paged.h) for a RAGGED batch (include/qsparse_hip.h, "MX KV cache append, ragged"): the new
// tokens are flat and token-major -- k_new [Ttot, Hkv, d], v_new [Ttot, Hkv, dv], q_new [Ttot, Hq, d], as a QKV projection writes them --
// and cu_seqlens [B + 1], read on the device, says which sequence owns which.  Per sequence the rule is the paged append's with T_b in the
// place of T; ONE launch for any mix of lengths.  The three kinds of item, the tile, the barriers and the tail rule are kept:
//
//   row items   run over the FLAT rows: the Ttot Hkv rows of k_new, then the Ttot Hq rows of q_new, `rpg` per work-group.  Flat row f is
//               token f / H, head f % H, and IS row f of the input and (Q) of the token-major q_codes: no transpose on either side.  Each
//               row finds its sequence by a binary search for its token in cu_seqlens (log2(B + 1) loads per lane, the lanes of a row
//               agree), checks cu[b] <= token < cu[b + 1] on the clamped entries -- a token behind cu[B], or any token under a malformed
//               cu_seqlens that fails the check, is stored nowhere -- then reads L_b and goes on as kvp_row_item: rotate by table row
//               min(L_b + t, P - 1), encode, look up the page of position L_b + t < S.
//   edge items  one per (b, hk), as before: the first and the last block of vt that the append touches and the tail; T_b == 0 ends the
//               item before v_tail is read.
//   mid items   floor(Ttot / 32) per kv head, whatever cu_seqlens holds: sequence b can have at most max(0, floor((T_b - 2) / 32))
//               whole blocks between its edge blocks, and these counts sum to no more than that.  An item finds its (b, m) through
//               qs_mx_ragged_map.h's prefix search, as the attention kernel finds its tile; one at or behind the sequence's last block
//               ends at once (the count is sized on T_b, the length is the device's).
//
// Tile fills read v_new token-major: position p of the block is token lo_b + p - L_b, its dv channels lie (Hkv dv) elements from the next
// token's.  kva_len, kvp_encode, kva_tail_store and KvaPaged are called as they are; the row item and the fill are stated again with
// the flat addressing in them (the existing kernels stay byte for byte).  cu_seqlens, kv_len and the table are read with vector loads;
// nothing is written through the scalar path.
#pragma once
#include "qs_mx_kv_append_paged.h"
#include "qs_mx_ragged_map.h"

namespace qs {

struct KvgArgs : KvaPagedArgs {                                 // k_new .. q_new flat; T, row_groups, mid are not read; n_row: work-groups
    const int32_t* __restrict__ cu;                             // [B + 1]
    int Ttot;
};

// ---- row items -------------------------------------------------------------------------------------------------------------------------
template <int XDT, bool VEC>
__device__ __forceinline__ void kvg_row_item(const KvgArgs& a, const MxFormat& fq, const KvaPaged& w) {
    using raw_t = typename Mxq2Raw<XDT>::type;
    constexpr int V = RopeLane<XDT>::V;
    const int r = (int)threadIdx.x / a.lpr;
    const int64_t gc = (int64_t)((int)threadIdx.x % a.lpr) * V;
    const int64_t nk = (int64_t)a.Hkv * a.Ttot, nq = (int64_t)a.Hq * a.Ttot;
    const int64_t rr = (int64_t)blockIdx.x * a.rpg + r;        // the flat row: K rows (token, hk), then Q rows (token, hq)
    const bool row_in = r < a.rpg && rr < nk + nq;
    const bool isq = row_in && rr >= nk;
    const int64_t fr = !row_in ? 0 : (isq ? rr - nk : rr);      // token * H + head (no address is formed from a row that does not exist)
    const int H = isq ? a.Hq : a.Hkv;
    const int token = (int)(fr / H), head = (int)(fr % H);

    // the sequence: the first entry j in [1, B] with cu[j] > token owns it as b = j - 1; none: the token lies behind cu[B]
    int b = 0, t = 0;
    bool live = false;
    if (row_in) {
        int l = 1, h = a.B + 1;
        while (l < h) {
            const int mid = (l + h) >> 1;
            if (mxrg_clamp(a.cu[mid], a.Ttot) > token) h = mid;
            else l = mid + 1;
        }
        if (l <= a.B) {
            const int s0 = mxrg_clamp(a.cu[l - 1], a.Ttot), s1 = mxrg_clamp(a.cu[l], a.Ttot);
            live = s0 <= token && token < s1;                   // (holds for a non-decreasing cu_seqlens; a guard otherwise)
            b = l - 1, t = live ? token - s0 : 0;
        }
    }
    int L = 0;
    if (live) {
        const int raw = a.kv_len[b];
        L = raw < 0 ? 0 : (raw > a.S ? a.S : raw);
    }
    const int pos = L + t;
    const int64_t C = a.d, h = C >> 1;
    const raw_t* xrow = (isq ? (const raw_t*)a.q_new : (const raw_t*)a.k_new) + fr * C;

    float y[V];
    if (a.mode == kKvaPlainRows) {                              // (kernel-uniform)
        if constexpr (VEC) {                                    // (C % V == 0: the lane's V elements are inside or outside together)
            u32x4 x = {0u, 0u, 0u, 0u};
            if (live && gc < C) x = ld16<true>((const u32x4*)(xrow + gc));
            rope_unpack<XDT>(x, y);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) y[j] = (live && gc + j < C) ? mxq2_widen<XDT>(xrow[gc + j]) : 0.0f;
        }
    } else {
        const int64_t tr = pos < a.P ? pos : a.P - 1;           // the table row: min(L_b + t, P - 1)
        RopeLane<XDT> ln;
        if (a.mode == kKvaInterleaved) {
            rope_load<XDT, VEC, true>(ln, xrow, a.cs + tr * h, a.sn + tr * h, gc, C, h, live);
            rope_rotate<XDT, true>(ln, gc, h, 0, y);
        } else {
            rope_load<XDT, VEC, false>(ln, xrow, a.cs + tr * h, a.sn + tr * h, gc, C, h, live);
            rope_rotate<XDT, false>(ln, gc, h, 0, y);
        }
    }
    // where the row goes: row (L_b + t) % page of its page -- nowhere at or past S -- or row (token, hq) of q's dense pair
    const int64_t nbc = (C + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    const int64_t R = isq ? nq : w.k_rows();
    int64_t gr = R;
    if (live && isq) gr = fr;
    else if (live && pos < a.S) gr = w.k_row(b, head, pos);
    mxq2_emit_row<V, VEC, VEC, false, false>(y, fq, isq ? a.q_codes : a.k_codes, isq ? a.q_scales : a.k_scales, gr, gc, R, C, nbc, 1,
                                             MxSrKey{0u, 0u}, 0ull);
}

// ---- a block of vt: kva_fill from the token-major v_new --------------------------------------------------------------------------------
// the tile of the block at column c0 of (b, hk) = bh, whose tokens start at flat token `lo`: positions below L from v_tail, [L, Lp) from
// v_new, +0 behind
template <int XDT, bool VEC>
__device__ __forceinline__ void kvg_fill(float* tile, const KvgArgs& a, int64_t bh, int lo, int c0, int L, int Lp) {
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
    const int64_t pitch = (int64_t)a.Hkv * a.dv;               // elements between two tokens of one head
    const raw_t* vn = (const raw_t*)a.v_new + ((int64_t)lo * a.Hkv + bh % a.Hkv) * a.dv;
    float v[QS_MX_BLOCK / RPP][V];
#pragma unroll
    for (int i = 0; i < QS_MX_BLOCK / RPP; ++i) {               // every load is issued before the first store
        const int p = pr + i * RPP, pos = c0 + p;
        const bool in = p >= nt && pos < Lp && lc < a.dv;
        const raw_t* row = vn + (int64_t)(in ? pos - L : 0) * pitch;
        if constexpr (VEC) {                                    // (dv % V == 0: the lane's V channels are inside or outside together)
            u32x4 x = {0u, 0u, 0u, 0u};
            if (in) x = ld16<true>((const u32x4*)(row + lc));
            rope_unpack<XDT>(x, v[i]);
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

// ---- the work-group's item -------------------------------------------------------------------------------------------------------------
template <int XDT, bool VEC>
__global__ __launch_bounds__(kKvaThreads) void mx_kv_append_ragged_kernel(MxFormat fq, MxFormat fv, KvgArgs a) {
    __shared__ float tile[QS_MX_BLOCK * kKvaPitch];
    __shared__ int slot[5];
    const KvaPaged w{a};
    if (blockIdx.x < a.n_row) {                                 // (work-group-uniform, as every branch below)
        kvg_row_item<XDT, VEC>(a, fq, w);
        return;
    }
    const unsigned item = blockIdx.x - a.n_row;
    if (item >= a.n_edge) {                                     // a whole block between a sequence's edge blocks
        const unsigned idx = item - a.n_edge;
        MxRaggedItem it;
        if (!mxrg_item(slot, a.cu, a.B, a.Ttot, idx / (unsigned)a.Hkv, [](int T) { return T >= 2 ? (T + 2 * QS_MX_BLOCK - 2) / QS_MX_BLOCK - 2 : 0; },
                       it))
            return;
        const int64_t bh = (int64_t)it.b * a.Hkv + idx % (unsigned)a.Hkv;
        const int L = kva_len(a, it.b);
        const int Lp = L + (it.T < a.S - L ? it.T : a.S - L);
        if (Lp == L) return;
        const int blk = (L >> 5) + 1 + it.idx;
        if (blk >= (Lp - 1) >> 5) return;
        kvg_fill<XDT, VEC>(tile, a, bh, it.lo, blk * QS_MX_BLOCK, L, Lp);
        __syncthreads();
        kvp_encode<VEC>(tile, a, fv, bh, blk * QS_MX_BLOCK, w);
        return;
    }
    const int64_t bh = item;
    int lo, T;
    mxrg_seq(a.cu, (int)(bh / a.Hkv), a.Ttot, lo, T);
    if (T == 0) return;                                         // an idle slot: v_tail is neither read nor written
    const int L = kva_len(a, (int)(bh / a.Hkv));
    const int Lp = L + (T < a.S - L ? T : a.S - L);             // L': the length after the append
    if (Lp == L) return;                                        // a full cache: nothing is stored
    const int first = L >> 5, last = (Lp - 1) >> 5;
    kvg_fill<XDT, VEC>(tile, a, bh, lo, first * QS_MX_BLOCK, L, Lp);      // (reads the tail)
    __syncthreads();
    kvp_encode<VEC>(tile, a, fv, bh, first * QS_MX_BLOCK, w);
    if (last != first) {
        __syncthreads();                                        // (the tile is free; every read of the tail lies two barriers back)
        kvg_fill<XDT, VEC>(tile, a, bh, lo, last * QS_MX_BLOCK, L, Lp);
        __syncthreads();
        kvp_encode<VEC>(tile, a, fv, bh, last * QS_MX_BLOCK, w);
    }
    if (Lp & 31) {                                              // the last block stays open: its new columns go to the tail
        const int c0 = last * QS_MX_BLOCK;
        kva_tail_store(tile, a, bh, L > c0 ? L - c0 : 0, Lp - c0);
    }
}

}  // namespace qs
