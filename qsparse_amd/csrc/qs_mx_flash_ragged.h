// Grouped-query attention on MX codes for a RAGGED batch of new tokens against the cache they were appended to (include/qsparse_hip.h,
// "MX flash attention, ragged"): the flat token axis q [Ttot, Hq, d] -- token-major, as a QKV projection writes it -- is cut into B
// sequences by cu_seqlens, read on the device; sequence b's T_b tokens see the first L_b keys of ITS cache rows or table row.  One launch
// for any mix of lengths.  The numerics are qs_mx_flash_prefill.h's, sequence by sequence: every byte is mx_flash_prefill_kernel's on
// that sequence alone.
//
// Item map (new here).  Sequence b has ceil(r T_b / 64) tiles of 64 packed rows rho = t r + h % r, as the prefill kernel packs them.
// The grid is `items` work-groups per kv head, items = ceil(r Ttot / 64) + B >= sum_b ceil(r T_b / 64) for every cu_seqlens -- a function
// of the shapes alone, never B tiles(T_max).  blockIdx.x = q Hkv + hk; the work-group's item is items - 1 - q: items are taken in
// DESCENDING order, so the surplus work-groups (past the total: they return behind the search, before any operand is touched) leave
// first, then the last sequence's last tile -- within a sequence the tiles latest in T, which walk the most chunks under `causal`, are
// still dispatched first (the prefill kernel's block order, per sequence).  The (b, tile) of an item comes from qs_mx_ragged_map.h: wave
// 0 scans cu_seqlens in rounds of 64 entries, a ballot finds the owner, the result reaches the other waves through LDS behind ONE
// barrier, in front of the prologue.  cu_seqlens, kv_len and the table are read with vector loads and made uniform by readfirstlane.
//
// Token-major rows.  Row rho of the tile is token lo_b + rho / r, query head hk r + rho % r: row (lo_b + rho / r) Hq + hk r + rho % r of
// q [Ttot Hq, d] and of y.  The r heads of a token are ADJACENT rows, so the 16 rows of a wave are runs of r d contiguous bytes per
// token (r dv elements of y): the lanes' 16-byte Q loads and 4-element stores coalesce across heads, where the head-major layout put
// neighbouring rows T d bytes apart.
//
// Chunk loop.  mx_flash_prefill_kernel's as it stands -- K and vt staged in LDS once per tile for all r heads, the next chunk in
// registers, barriers A and B, the length, limit and page rules (MxrSource) -- with T_b in the place of T.  The loop is the body of that
// kernel and cannot be included; it is stated here a second time.  mxr_stage, mxr_scores, mxr_pv_p, MxrArgs and MxrSource are templates
// or inline and ARE included (qs_mx_flash_prefill.h stays byte for byte).
#pragma once
#include "qs_mx_flash_prefill.h"
#include "qs_mx_ragged_map.h"

namespace qs {

struct MxgArgs : MxrArgs {                                      // T, R, tiles, heads are not read: they differ per sequence
    const int32_t* __restrict__ cu;                             // [B + 1]
    int B, Hq, Ttot, items;                                     // items: work-groups per kv head
};

template <bool PAGED>
__global__ __launch_bounds__(kMxgThreads, 2) void mx_flash_ragged_kernel(MxFormat fp, MxgArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxrLds];
    __shared__ int slot[5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int hk = (int)(blockIdx.x % (unsigned)a.Hkv);
    const unsigned item = (unsigned)a.items - 1u - blockIdx.x / (unsigned)a.Hkv;       // descending: the surplus work-groups first
    const int r = a.r;
    MxRaggedItem it;
    if (!mxrg_item(slot, a.cu, a.B, a.Ttot, item, [r](int T) { return (r * T + kMxfRows - 1) / kMxfRows; }, it)) return;
    const int b = it.b, tile = it.idx, T = it.T, R = r * T;
    const int S = a.S, d = a.d, dv = a.dv;
    const int nkb = (d + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    uint8_t* ktile = lds;
    uint8_t* vtile = lds + kMxfTile;
    uint8_t* sk = lds + 2 * kMxfTile;
    uint8_t* sv = sk + kMxrScales;
    uint8_t* row = sv + kMxrScales + wave * kMxfBounce + i * kMxfBounceRow;         // this lane's row in the wave's bounce
    const int qb = mxg_bits(a.qk_format), vb = mxg_bits(a.v_format);

    // this lane's packed row, token-major: token lo + rho / r, query head hk r + rho % r
    const int rho = kMxfRows * tile + 16 * wave + i;
    const bool rin = rho < R;
    const int tok = rin ? rho / r : 0;
    const int64_t qrow = ((int64_t)it.lo + tok) * a.Hq + (int64_t)hk * r + (rin ? rho % r : 0);    // row of q [Ttot Hq, d] and of y

    // L: one vector load (the address is the lane's own), then uniform
    const int raw = a.kv_len[b + (int)__builtin_amdgcn_mbcnt_lo(0u, 0u)];         // (+ 0, in a vector register)
    const int L = __builtin_amdgcn_readfirstlane(raw < 0 ? 0 : (raw > S ? S : raw));
    int Lim = !rin ? 0 : L;                                     // the row admits the keys j < Lim
    if (a.causal && rin) Lim = L - T + tok + 1 < 0 ? 0 : L - T + tok + 1;
    // limits ascend with rho: the tile's largest is its last row's
    const int rlast = kMxfRows * tile + kMxfRows - 1 < R ? kMxfRows * tile + kMxfRows - 1 : R - 1;
    int top = L;
    if (a.causal) top = L - T + rlast / r + 1 < 0 ? 0 : L - T + rlast / r + 1;
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
            for (int e = 0; e < 4; ++e) {
                float w = s[f][e] * a.scale;
                w = c0 + e < Lim ? w : ninf;                    // (a select: a NaN at or behind the limit is dropped)
                s[f][e] = w;
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
            for (int e = 0; e < 4; ++e) s[f][e] = msx_exp(s[f][e] - m2);
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
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t ab = mx_abs_bits(s[2 * bk + h][e]);
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
                    for (int e = 0; e < 4; ++e) {
                        uint32_t sg;
                        const float qv = mx_round_abs(s[2 * bk + h][e], sc, fp, sg);
                        pc[h] |= mx_code(qv, sg, sc, fp) << (8 * e);
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
                for (int e = 0; e < 4; ++e) acc[j][e] = live ? acc[j][e] * alpha + o[j][e] : acc[j][e];
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
        for (int e = 0; e < 4; ++e) v[e] = rownan ? __uint_as_float(0x7fc00000u) : acc[j][e] / Z;
        mx_store4(a.y, a.ydt, qrow * dv + n, v, n, dv, a.y_vec);
    }
}

}  // namespace qs
