// Grouped-query attention on MX codes for a CHUNK OF NEW TOKENS against the cache they were appended to (include/qsparse_hip.h, "MX flash
// attention, prefill on the cache"): any T, any r = Hq / Hkv, the valid length read on the device, the cache contiguous or paged.  The
// numerics are the decode section's at one split -- the streamed chunk recurrence (qs_mx_flash_stream.h, phases 1 to 3) on the cache
// sliced to L_b keys, row limits aligned bottom-right -- so every byte is _decode_def(..., splits=1)'s.
//
// Work split.  One work-group of 4 waves per (sequence b, kv head hk, tile of 64 packed rows); wave w owns 16 rows, lane 16 g + i holds
// row i of the wave in every accumulator (qs_mx_flash.h's lane map).  The R = r T rows of a group are packed TOKEN-MAJOR, rho = t r +
// h % r: a tile spans about 64 / r consecutive tokens of all r heads, so its rows share one K / vt chunk in LDS and its causal limits lie
// as close together as they can.  Rows are independent in the definition, so the packing decides which rows share a tile and nothing
// else; r need not divide 64 (one division by r per lane, for the Q load and the store).  This is neither the decode kernel on a wider
// grid (there a chunk is consumed by ONE wave, from registers, with no barrier) nor the streamed kernel (one slice per work-group, a
// top-left limit, a mask stream, no lengths).
//
// Data movement.  K and vt are read from memory ONCE per tile of 64 rows, for the whole group of r heads: one LDS tile per operand
// (16 KB each), their scale bytes (512 B each) and the per-wave bounce of p's codes (9 KB) = 43 KB, three work-groups per CU.  The next
// chunk is double-buffered in REGISTERS as in the streamed kernel: K chunk c + 1 is issued at the top of iteration c and staged behind
// barrier A, vt chunk c + 1 is issued there and staged at the top of iteration c + 1, behind barrier B; 4 + 1 registers in flight.
//
// Lengths.  L = clamp(kv_len[b], 0, S): one load per work-group, then uniform.  Keys >= L stage as zero codes under the byte 127 and
// get u = -inf by select; vt codes at columns >= L are cleared when staged (byte masks only in the chunk that holds L), a vt scale
// block wholly past L is 127, a block of e wholly past L is zero codes under 127.  Row limit lim = clamp(L - T + t + 1, 0, L) with
// `causal`, else L; a row whose limit lies at or before the chunk's first key keeps its state by select.  The loop runs to the chunk
// that holds min(L, the tile's largest lim) - 1 -- the limit of the tile's LAST row, limits ascend with rho -- and nothing behind it is
// fetched.  A work-group with nothing to walk writes NaN rows (Z == 0).
//
// Paged (template parameter: the contiguous kernel carries no table register).  A chunk of 128 keys spans npc = max(1, 128 / page)
// pages.  In the staging map piece i of K is the keys 32 i .. 32 i + 31 of the chunk: its page is uniform over the work-group; a vt
// piece's page depends on the thread's column group tid & 7 alone, a scale byte's on tid >> 1 (K) or tid & 1 (vt).  The (at most four)
// entries of chunk c + 2 are loaded behind the vt fetch of chunk c + 1, land while phase 3 of chunk c runs and are checked at the top of
// iteration c + 1, so no table load sits in front of a fetch.  Entry n is loaded only where n page < min(L, 128 c_end): what the
// definition calls dead is never turned into an address; a live entry outside [0, P) becomes -1 and its loads are predicated off
// (zero codes under 127).
//
// Block order.  blockIdx.x = (tiles - 1 - tile) heads + (b Hkv + hk): the tiles latest in T, which walk the most chunks under `causal`,
// are dispatched first.
//
// Shared code.  mxf_load16, mxf_frag, MxgLds / mxg_stage, msx_exp, the quantizer calls, the bounce layout, mxd_clip and kMxsChunk come
// from the headers included here.  qs_mx_flash_stream.h cannot be included into a second unit (its kernel is not `inline`: the link
// sees it twice) nor beside qs_mx_flash_decode.h (both define kMxsChunk), and the existing headers stay as they are, so its LDS sizes,
// mxs_stage, mxs_scores and mxs_pv are stated here a second time as mxr_*, word for word.
#pragma once
#include "qs_mx_flash_decode.h"

namespace qs {

constexpr int kMxrScales = kMxsChunk * 4;                        // the scale bytes of a tile: 128 rows x 4 blocks
constexpr int kMxrLds = 2 * kMxfTile + 2 * kMxrScales + 4 * kMxfBounce;

__device__ __forceinline__ void mxr_stage(uint8_t* tile, const u32x4 (&reg)[4], int tid, int bits) {      // (kernel-uniform)
    if (bits == 8) mxg_stage<8>(tile, reg, tid);
    else if (bits == 6) mxg_stage<6>(tile, reg, tid);
    else mxg_stage<4>(tile, reg, tid);
}

// phase 1 for the format FQ of q and k: the wave's 16 rows against the 128 keys of the tile, sk[4 r + b] the scale byte of block b of
// its row r
template <int FQ>
__device__ __forceinline__ void mxr_scores(f32x4 (&s)[8], const uint8_t* tile, const i32x8& fq, int sq, const uint8_t* sk, int i, int g) {
    using L = MxgLds<mxg_bits(FQ)>;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        s[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(L::get(tile, 16 * j + i, g), fq, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, FQ, FQ, 0,
                                                                (int)sk[4 * (16 * j + i) + g], 0, sq);
}

// phase 3 for the formats FP of p and FV of vt: o[j] = the wave's 16 rows against the rows 16 j .. of the vt tile over this chunk;
// `row`: the lane's row's 128 codes in the bounce, sp its scale byte of block g, sv[4 r + b] that of block b of the tile's row r
template <int FP, int FV>
__device__ __forceinline__ void mxr_pv(f32x4 (&o)[8], const uint8_t* tile, const uint8_t* row, int sp, const uint8_t* sv, int dv, int i, int g) {
    constexpr int PB = mxg_bits(FP);
    using LV = MxgLds<mxg_bits(FV)>;
    const int plo = PB == 8 ? 16 * g : 32 * g, phi = PB == 8 ? 64 + 16 * g : 32 * g + 16;
    const i32x8 fpv = mxf_frag<PB>(*(const u32x4*)(row + plo), *(const u32x4*)(row + phi));
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (16 * j < dv)                                        // (kernel-uniform)
            o[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(LV::get(tile, 16 * j + i, g), fpv, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, FV, FP,
                                                                    0, (int)sv[4 * (16 * j + i) + g], 0, sp);
}

template <int FP, class... A>
__device__ __forceinline__ void mxr_pv_v(int v_format, A&&... args) {
    switch (v_format) {
#define X(F) case F: mxr_pv<FP, F>(args...); break;
        QS_MXF_FORMATS(X)
#undef X
        default: mxr_pv<FP, QS_MX_FP4_E2M1>(args...); break;
    }
}

template <class... A>
__device__ __forceinline__ void mxr_pv_p(int p_format, int v_format, A&&... args) {
    switch (p_format) {
#define X(F) case F: mxr_pv_v<F>(v_format, args...); break;
        QS_MXF_FORMATS(X)
#undef X
        default: mxr_pv_v<QS_MX_FP4_E2M1>(v_format, args...); break;
    }
}

struct MxrArgs {
    const uint8_t* __restrict__ q;
    const uint8_t* __restrict__ qs;
    const uint8_t* __restrict__ k;                              // the cache [B, Hkv, S, d] or the pool [P, Hkv, page, d]
    const uint8_t* __restrict__ ks;
    const uint8_t* __restrict__ vt;                             // [B, Hkv, dv, S] or [P, Hkv, dv, page]
    const uint8_t* __restrict__ vts;
    const int32_t* __restrict__ kv_len;                         // [B]; nullable without a table
    const int32_t* __restrict__ table;                          // [B, NP] or null
    void* __restrict__ y;
    int T, S, d, dv, Hkv, r, R, tiles, heads;                   // S = NP page with a table; tiles of 64 packed rows; heads = B Hkv
    int P, NP, lg;                                              // pool pages, pages per sequence, log2(page)
    float scale;
    int qk_format, p_format, v_format, ydt, causal, vec, y_vec;
};

__device__ __forceinline__ int mxr_sel4(const int (&v)[4], int q) { return q == 0 ? v[0] : (q == 1 ? v[1] : (q == 2 ? v[2] : v[3])); }

// where a work-group's K and vt come from: mxs_fetch / mxs_fetch_scales with the length L and, PAGED, through the table
template <bool PAGED>
struct MxrSource {
    const uint8_t* __restrict__ k;
    const uint8_t* __restrict__ ks;
    const uint8_t* __restrict__ vt;
    const uint8_t* __restrict__ vts;
    const int32_t* __restrict__ tab;                            // row b of the table
    int L, S, d, dv, nkb, nsb, Hkv, hk, P, lg, last, vec;       // keys < last = min(L, 128 c_end) are needed
    int pg[4], nxt[4];                                          // the pool pages of the chunk being fetched (-1: dead), the raw entries of the next

    __device__ __forceinline__ MxrSource(const MxrArgs& a, int b, int hk_, int L_, int c_end)
        : L(L_), S(a.S), d(a.d), dv(a.dv), nkb((a.d + QS_MX_BLOCK - 1) / QS_MX_BLOCK), nsb((a.S + QS_MX_BLOCK - 1) / QS_MX_BLOCK), Hkv(a.Hkv),
          hk(hk_), P(a.P), lg(a.lg), vec(a.vec) {
        const int64_t e = (int64_t)c_end * kMxsChunk;
        last = e < L ? (int)e : L;
        if constexpr (PAGED) {
            k = a.k, ks = a.ks, vt = a.vt, vts = a.vts, tab = a.table + (int64_t)b * a.NP;
        } else {
            const int64_t bh = (int64_t)b * a.Hkv + hk_;
            k = a.k + bh * S * d, ks = a.ks + bh * S * nkb, vt = a.vt + bh * dv * S, vts = a.vts + bh * dv * nsb, tab = nullptr;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) pg[q] = nxt[q] = -1;
    }

    // issue the loads of chunk c's entries; one that is dead, behind the chunk's pages or not needed stays -1 and forms no address
    __device__ __forceinline__ void table_load(int c) {
        if constexpr (PAGED) {
            const int npc = lg >= 7 ? 1 : kMxsChunk >> lg;
            const int64_t n0 = ((int64_t)c * kMxsChunk) >> lg;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int e = -1;
                if (q < npc && ((n0 + q) << lg) < last) e = tab[n0 + q];        // (uniform over the work-group)
                nxt[q] = e;
            }
        }
    }
    // the loaded entries become the chunk's pages: one outside [0, P) is -1 from here on
    __device__ __forceinline__ void table_take() {
        if constexpr (PAGED) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = __builtin_amdgcn_readfirstlane(nxt[q]);
                pg[q] = e >= 0 && e < P ? e : -1;
            }
        }
    }

    // K: the thread's piece tid & 7 along d of the chunk's rows (tid >> 3) + 32 i, and its two scale bytes of row tid >> 1
    __device__ __forceinline__ void fetch_k(u32x4 (&reg)[4], uint32_t& rs, int64_t key0, int tid) {
        const int kk = (tid & 7) * 16, left = d - kk < 16 ? d - kk : 16, pm = (1 << lg) - 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t key = key0 + (tid >> 3) + 32 * i;
            bool in = key < L && kk < d;
            int64_t row = key;
            if constexpr (PAGED) {
                const int p = pg[lg >= 7 ? 0 : (32 * i) >> lg];     // (uniform over the work-group)
                in = in && p >= 0;
                row = (((int64_t)(p < 0 ? 0 : p) * Hkv + hk) << lg) + ((int)key & pm);     // of k_pool [P Hkv page, d]
            }
            reg[i] = mxf_load16(k, in, row * d + kk, left, vec);
        }
        const int ro = tid >> 1, b0 = 2 * (tid & 1);
        const int64_t key = key0 + ro;
        bool in = key < L;
        int64_t row = key;
        if constexpr (PAGED) {
            const int p = mxr_sel4(pg, lg >= 7 ? 0 : ro >> lg);
            in = in && p >= 0;
            row = (((int64_t)(p < 0 ? 0 : p) * Hkv + hk) << lg) + ((int)key & pm);
        }
        rs = mx_scale(ks, in && b0 < nkb, row * nkb + b0) | (mx_scale(ks, in && b0 + 1 < nkb, row * nkb + b0 + 1) << 8);
    }

    // vt: the thread's 16 columns key0 + 16 (tid & 7) .. of the rows (tid >> 3) + 32 i, columns >= L cleared, and its two scale bytes
    // (blocks 2 (tid & 1) + {0, 1} of the chunk) of row tid >> 1, 127 for a block wholly past L
    __device__ __forceinline__ void fetch_vt(u32x4 (&reg)[4], uint32_t& rs, int64_t key0, int tid) {
        const int co = (tid & 7) * 16, pm = (1 << lg) - 1;
        const int64_t col = key0 + co;
        const int nv = (int)(L - col < 16 ? L - col : 16);      // (<= 0: nothing of the piece is valid)
        const bool cut = key0 + kMxsChunk > L;                  // (uniform: the chunk that holds L)
        int p = 0;
        if constexpr (PAGED) p = mxr_sel4(pg, lg >= 7 ? 0 : co >> lg);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = (tid >> 3) + 32 * i;
            if (32 * i < dv) {                                  // (kernel-uniform)
                bool in = n < dv && nv > 0;
                int64_t off = (int64_t)n * S + col;
                if constexpr (PAGED) {
                    in = in && p >= 0;
                    off = ((((int64_t)(p < 0 ? 0 : p) * Hkv + hk) * dv + n) << lg) + ((int)col & pm);     // of vt_pool [P Hkv dv, page]
                }
                u32x4 v = mxf_load16(vt, in, off, nv, vec);
                if (cut) v = mxd_clip(v, nv);
                reg[i] = v;
            } else {
                reg[i] = u32x4{0u, 0u, 0u, 0u};
            }
        }
        const int n = tid >> 1;
        uint32_t out = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int bo = 2 * (tid & 1) + e;                   // the block inside the chunk
            const int64_t cs = key0 + QS_MX_BLOCK * bo;
            bool in = n < dv && cs < L;
            int64_t off = (int64_t)n * nsb + cs / QS_MX_BLOCK;
            if constexpr (PAGED) {
                const int ps = mxr_sel4(pg, lg >= 7 ? 0 : (QS_MX_BLOCK * bo) >> lg);
                in = in && ps >= 0;
                off = ((((int64_t)(ps < 0 ? 0 : ps) * Hkv + hk) * dv + n) << (lg - 5)) + (((int)cs & pm) >> 5);
            }
            out |= mx_scale(vts, in, off) << (8 * e);
        }
        rs = out;
    }
};

template <bool PAGED>
__global__ __launch_bounds__(kMxgThreads, 2) void mx_flash_prefill_kernel(MxFormat fp, MxrArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxrLds];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int bh = (int)(blockIdx.x % (unsigned)a.heads);       // b Hkv + hk
    const int tile = a.tiles - 1 - (int)(blockIdx.x / (unsigned)a.heads);      // the heaviest tiles first
    const int b = bh / a.Hkv, hk = bh % a.Hkv;
    const int T = a.T, S = a.S, d = a.d, dv = a.dv;
    const int nkb = (d + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    uint8_t* ktile = lds;
    uint8_t* vtile = lds + kMxfTile;
    uint8_t* sk = lds + 2 * kMxfTile;
    uint8_t* sv = sk + kMxrScales;
    uint8_t* row = sv + kMxrScales + wave * kMxfBounce + i * kMxfBounceRow;         // this lane's row in the wave's bounce
    const int qb = mxg_bits(a.qk_format), vb = mxg_bits(a.v_format);

    // this lane's packed row, token-major: token rho / r, query head hk r + rho % r
    const int rho = kMxfRows * tile + 16 * wave + i;
    const bool rin = rho < a.R;
    const int tok = rin ? rho / a.r : 0;
    const int64_t qrow = ((int64_t)bh * a.r + (rin ? rho % a.r : 0)) * T + tok;     // row of q [B Hq T, d] and of y

    // L: one vector load (the address is the lane's own), then uniform
    int L = S;
    if (a.kv_len) {
        const int raw = a.kv_len[b + (int)__builtin_amdgcn_mbcnt_lo(0u, 0u)];     // (+ 0, in a vector register)
        L = __builtin_amdgcn_readfirstlane(raw < 0 ? 0 : (raw > S ? S : raw));
    }
    int Lim = !rin ? 0 : L;                                     // the row admits the keys j < Lim
    if (a.causal && rin) Lim = L - T + tok + 1 < 0 ? 0 : L - T + tok + 1;
    // limits ascend with rho: the tile's largest is its last row's
    const int rlast = kMxfRows * tile + kMxfRows - 1 < a.R ? kMxfRows * tile + kMxfRows - 1 : a.R - 1;
    int top = L;
    if (a.causal) top = L - T + rlast / a.r + 1 < 0 ? 0 : L - T + rlast / a.r + 1;
    const int c_end = (top + kMxsChunk - 1) / kMxsChunk;        // (uniform over the work-group: the barriers are)

    // the Q fragment and its scale byte, once
    const int klo = qb == 8 ? 16 * g : 32 * g, khi = qb == 8 ? 64 + 16 * g : 32 * g + 16;
    const u32x4 qlo = mxf_load16(a.q, rin && klo < d, qrow * d + klo, d - klo < 16 ? d - klo : 16, a.vec);
    const u32x4 qhi = mxf_load16(a.q, rin && khi < d, qrow * d + khi, d - khi < 16 ? d - khi : 16, a.vec);
    const i32x8 fq = qb == 8 ? mxf_frag<8>(qlo, qhi) : (qb == 6 ? mxf_frag<6>(qlo, qhi) : mxf_frag<4>(qlo, qhi));
    const int sq = (int)mx_scale(a.qs, rin && g < nkb, qrow * nkb + g);

    const float ninf = __uint_as_float(0xff800000u);
    float m = ninf, Z = 0.0f;
    bool bad = false;
    f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    MxrSource<PAGED> src(a, b, hk, L, c_end);
    u32x4 reg[4];                                               // the pieces in flight: K chunk c + 1, then vt chunk c + 1
    uint32_t rs = 0;                                            // ... and their two scale bytes
    if (c_end > 0) {
        src.table_load(0);
        src.table_take();
        src.table_load(1);
        src.fetch_k(reg, rs, 0, tid);
        mxr_stage(ktile, reg, tid, qb);
        *(uint16_t*)(sk + 2 * tid) = (uint16_t)rs;
        src.fetch_vt(reg, rs, 0, tid);
    }

    for (int c = 0; c < c_end; ++c) {
        const int64_t key0 = (int64_t)c * kMxsChunk;
        const bool more = c + 1 < c_end;                        // (uniform over the work-group)
        mxr_stage(vtile, reg, tid, vb);                         // vt chunk c (free since barrier B of the chunk before)
        *(uint16_t*)(sv + 2 * tid) = (uint16_t)rs;
        if (c == 0) __syncthreads();                            // (the K tile of the prologue)
        if (more) {                                             // in flight through phases 1 and 2
            src.table_take();                                   // the pages of chunk c + 1, loaded an iteration ago
            src.fetch_k(reg, rs, key0 + kMxsChunk, tid);
        }

        // ---- phase 1 -----------------------------------------------------------------------------------------------------------
        f32x4 s[8];
        switch (a.qk_format) {                                  // (kernel-uniform)
            case QS_MX_FP8_E4M3: mxr_scores<QS_MX_FP8_E4M3>(s, ktile, fq, sq, sk, i, g); break;
            case QS_MX_FP8_E5M2: mxr_scores<QS_MX_FP8_E5M2>(s, ktile, fq, sq, sk, i, g); break;
            case QS_MX_FP6_E2M3: mxr_scores<QS_MX_FP6_E2M3>(s, ktile, fq, sq, sk, i, g); break;
            case QS_MX_FP6_E3M2: mxr_scores<QS_MX_FP6_E3M2>(s, ktile, fq, sq, sk, i, g); break;
            default: mxr_scores<QS_MX_FP4_E2M1>(s, ktile, fq, sq, sk, i, g); break;
        }

        // ---- phase 2: qs_mx_flash_stream.h's, with the row's limit for the mask ---------------------------------------------------
        float mc = ninf;
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            const int64_t c0 = key0 + 16 * f + 4 * g;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float w = s[f][r] * a.scale;
                w = c0 + r < Lim ? w : ninf;                    // (a select: a NaN at or behind the limit is dropped)
                s[f][r] = w;
                bad |= w != w || w == __uint_as_float(0x7f800000u);
                mc = fmaxf(mc, w);                              // (a NaN is skipped here and kept in `bad`)
            }
        }
        mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
        mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
        const float m2 = fmaxf(m, mc);
        const float alpha = msx_exp(m - m2);                    // (-inf - -inf is a NaN: E gives +0)

        float P[8];                                             // partial sum 4 f + g of the row sum over 128 columns
#pragma unroll
        for (int f = 0; f < 8; ++f) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s[f][r] = msx_exp(s[f][r] - m2);
            P[f] = 0.0f + ((s[f][0] + s[f][1]) + (s[f][2] + s[f][3]));
        }
#pragma unroll
        for (int h = 4; h >= 1; h >>= 1)
#pragma unroll
            for (int f = 0; f < h; ++f) P[f] = P[f] + P[f + h];
        float z = P[0];
        z = z + __shfl_xor(z, 32, 64);
        z = z + __shfl_xor(z, 16, 64);

        uint32_t sw = 0x7f7f7f7fu;                              // the scale bytes of the row's four blocks; 127: a block wholly past L
#pragma unroll
        for (int bk = 0; bk < 4; ++bk) {
            uint32_t pc[2] = {0u, 0u};
            if (key0 + 32 * bk < L) {                           // (uniform over the work-group)
                uint32_t am = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t ab = mx_abs_bits(s[2 * bk + h][r]);
                        am = ab > am ? ab : am;
                    }
#pragma unroll
                for (int off = 16; off < 64; off <<= 1) {
                    const uint32_t o = (uint32_t)__shfl_xor((int)am, off, 64);
                    am = o > am ? o : am;
                }
                const MxScale sc = mx_scale(am, fp);
                sw = (sw & ~(0xffu << (8 * bk))) | (sc.byte << (8 * bk));
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        uint32_t sg;
                        const float qv = mx_round_abs(s[2 * bk + h][r], sc, fp, sg);
                        pc[h] |= mx_code(qv, sg, sc, fp) << (8 * r);
                    }
            }
            *(uint32_t*)(row + 32 * bk + 4 * g) = pc[0];
            *(uint32_t*)(row + 32 * bk + 16 + 4 * g) = pc[1];
        }

        __syncthreads();                                        // A: the vt tile and the bounce are written, every wave is past phase 1
        if (more) {
            mxr_stage(ktile, reg, tid, qb);
            *(uint16_t*)(sk + 2 * tid) = (uint16_t)rs;
            src.fetch_vt(reg, rs, key0 + kMxsChunk, tid);       // in flight through phase 3
            src.table_load(c + 2);                              // ... and so are the entries of the chunk after it
        }

        // ---- phase 3 -----------------------------------------------------------------------------------------------------------
        f32x4 o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        mxr_pv_p(a.p_format, a.v_format, o, vtile, row, (int)((sw >> (8 * g)) & 0xffu), sv, dv, i, g);       // (kernel-uniform switches)

        const bool live = key0 < Lim;                           // else the row's limit admits no column of this chunk: its state stays
        m = live ? m2 : m;
        Z = live ? Z * alpha + z : Z;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (16 * j < dv)                                    // (kernel-uniform)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[j][r] = live ? acc[j][r] * alpha + o[j][r] : acc[j][r];
        __syncthreads();                                        // B: the K tile is written, every wave is done with the vt tile and the bounce
    }

    // ---- epilogue: lane 16 g + i holds the columns 16 j + 4 g + {0..3} of row rho -----------------------------------------------------
    int badi = (int)bad;
    badi |= __shfl_xor(badi, 16, 64);
    badi |= __shfl_xor(badi, 32, 64);
    if (!rin) return;
    const bool rownan = badi != 0 || Z == 0.0f;                 // a NaN or +inf in u, or nothing admitted
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = 16 * j + 4 * g;
        if (n >= dv) continue;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = rownan ? __uint_as_float(0x7fc00000u) : acc[j][r] / Z;
        mx_store4(a.y, a.ydt, qrow * dv + n, v, n, dv, a.y_vec);
    }
}

}  // namespace qs
