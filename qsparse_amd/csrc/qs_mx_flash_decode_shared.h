// mx_flash_decode_paged_kernel (qs_mx_flash_decode_paged.h) for sequences that share a PREFIX of their paged cache (include/qsparse_hip.h,
// "MX flash attention, shared-prefix paged decode"): the first Ls keys of every sequence live in the pages of ONE table, shared_table, and
// are read once per 16 query rows of the BATCH, not once per sequence.  Ls = u floor(clamp(shared_len[0], 0, cap) / u) with u = max(128,
// page) and cap = min(NPs, NP) page: a whole number of chunks and of pages, read on the device, wave-uniform.
//
// Work split.  The unit of work is a wave, as in the paged kernel, and one launch holds two kinds of wave item, n = sp + so records per row:
//   - SHARED item ((hk tiles_s + tile) sp + run), tiles_s = ceil(B R / 16): lane i of every 16 owns the global row gamma = 16 tile + i of kv
//     head hk -- sequence b = gamma / R, packed row rho = gamma % R -- so a tile holds rows of up to 16 sequences and a sequence may
//     straddle two tiles.  What the paged kernel holds once per wave is per lane here: L_b (one kv_len load per lane), the row's limit,
//     qrow, the Q fragment and its scale byte, the record's address.  The wave walks the chunks [run cps_s, (run + 1) cps_s) below Cs = Ls /
//     128 and below the tile's last admitted key, against K and vt found through shared_table: the MFMA's 16 columns are 16 rows of the
//     batch against the same 128 keys, which is what cuts the prefix reads from B to ceil(B R / 16) per kv head and fills the instruction.
//   - OWN item (((b Hkv + hk) tiles + tile) so + run) - items_s: the paged kernel's item on block_table row b, from chunk Cs + run cps on.
//     Its record is sp + run.
// Every row's n records are written -- an item with no chunk writes the empty state -- and mx_flash_decode_combine_kernel combines them
// unchanged.  No barrier, no atomic, no wave waits for another; the grid is a function of the shapes alone.
//
// What is wave-uniform in a shared item.  The chunk recurrence is independent per row, so rows of different sequences sit side by side
// exactly as rows of different query heads do.  The length that the LOADS see is the tile's: Lt = min(max over its rows of L_b, Ls).  It
// bounds the table window, clears vt columns at or behind it and gates the quantizer's blocks.  A row with L_b < Lt is served by its limit
// alone: its scores at or behind L_b are -inf by select, its weights there are zero codes, and they multiply vt codes that are live keys of
// another row of the tile.  (Those must not be NaN codes or NaN scale bytes -- the one place where a row sees another sequence's bytes.)
//
// The table register, page broadcast, dead-page predication and the VEC / PLAIN routes are MxdPaged's, pointed at shared_table with NP =
// NPs in a shared item.  Table and length reads are vector loads followed by readlane / readfirstlane.
#pragma once
#include "qs_mx_flash_decode_paged.h"

namespace qs {

struct MxdSharedArgs : MxdPagedArgs {                           // n = sp + so; tiles, cps: of the own items; items: of both kinds
    const int32_t* __restrict__ stable;                         // [NPs]
    const int32_t* __restrict__ slen;                           // [1]
    int64_t items_s;                                            // Hkv tiles_s sp
    int B, NPs, cap, ulg;                                       // cap = min(NPs, NP) page; ulg = log2(max(128, page))
    int sp, cps_s, tiles_s;                                     // shared runs, chunks per shared run, tiles of 16 of the B R rows
};

__global__ __launch_bounds__(kMxgThreads, 1) void mx_flash_decode_shared_kernel(MxFormat fp, MxdSharedArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kMxfBounce];
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    if (item >= a.items) return;                                // (no barrier anywhere: a wave may leave)
    const bool sh = item < a.items_s;                           // (wave-uniform)
    const int T = a.T, S = a.S, d = a.d, dv = a.dv, R = a.R, so = a.n - a.sp;
    const int nkb = (d + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    uint8_t* row = lds + wave * kMxfBounce + i * kMxfBounceRow; // this lane's row in the wave's bounce
    const int qb = mxg_bits(a.qk_format), vb = mxg_bits(a.v_format);
    const int klo = qb == 8 ? 16 * g : 32 * g, khi = qb == 8 ? 64 + 16 * g : 32 * g + 16;
    const int vlo = vb == 8 ? 16 * g : 32 * g, vhi = vb == 8 ? 64 + 16 * g : 32 * g + 16;

    // Ls: one vector load (the address is the lane's own), then wave-uniform
    const int sraw = a.slen[(int)__builtin_amdgcn_mbcnt_lo(0u, 0u)];                      // (+ 0, in a vector register)
    const int Ls = (__builtin_amdgcn_readfirstlane(sraw < 0 ? 0 : (sraw > a.cap ? a.cap : sraw)) >> a.ulg) << a.ulg;
    const int Cs = Ls / kMxsChunk;

    // the item, and this lane's sequence b and packed row rho of kv head hk
    int hk, idx, c_begin, runlen, b, rho;
    bool rin;
    if (sh) {
        idx = (int)(item % a.sp);
        const int tile = (int)(item / a.sp % a.tiles_s);
        hk = (int)(item / a.sp / a.tiles_s);
        const int64_t gamma = (int64_t)16 * tile + i;
        rin = gamma < (int64_t)a.B * R;
        b = rin ? (int)(gamma / R) : 0, rho = rin ? (int)(gamma % R) : 0;
        c_begin = idx * a.cps_s, runlen = a.cps_s;
    } else {
        const int64_t it = item - a.items_s;
        const int split = (int)(it % so), tile = (int)(it / so % a.tiles);
        const int64_t bh = it / so / a.tiles;                   // b Hkv + hk
        b = (int)(bh / a.Hkv), hk = (int)(bh % a.Hkv);
        rho = 16 * tile + i, rin = rho < R;
        idx = a.sp + split;
        c_begin = Cs + split * a.cps, runlen = a.cps;
    }
    const int tok = rin ? rho % T : 0;
    const int64_t qrow = ((int64_t)b * a.Hkv * a.r + hk * a.r + (rin ? rho / T : 0)) * T + tok;      // row of q [B Hq T, d]

    // this lane's L_b and limit; Lt, what the wave's loads see: the sequence's L in an own item, min(the tile's largest L_b, Ls) in a shared
    const int raw = a.kv_len[b + (int)__builtin_amdgcn_mbcnt_lo(0u, 0u)];                 // (+ 0: a vector load in either kind of item)
    const int Lb = raw < 0 ? 0 : (raw > S ? S : raw);
    int Lim = !rin ? 0 : Lb;                                    // the row admits the keys j < Lim
    if (a.causal && rin) Lim = Lb - T + tok + 1 < 0 ? 0 : Lb - T + tok + 1;
    int top = Lim, Lt = sh && !rin ? 0 : Lb;                    // the tile's last admitted key + 1, the tile's last live key + 1
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const int o = __shfl_xor(top, off, 64), p = __shfl_xor(Lt, off, 64);
        top = o > top ? o : top, Lt = p > Lt ? p : Lt;
    }
    top = __builtin_amdgcn_readfirstlane(top), Lt = __builtin_amdgcn_readfirstlane(Lt);
    if (sh) Lt = Lt < Ls ? Lt : Ls;
    const int L = Lt;
    int c_end = (top + kMxsChunk - 1) / kMxsChunk;
    c_end = c_end < c_begin + runlen ? c_end : c_begin + runlen;
    if (sh) c_end = c_end < Cs ? c_end : Cs;

    // the Q fragment and its scale byte, once
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

    u32x4 kreg[16], vreg[16];                                   // the pieces of K chunk c (then c + 1) and of vt chunk c
    uint32_t ksc[8], vsc[8];
    MxdPaged src(a, sh ? 0 : __builtin_amdgcn_readfirstlane(b), hk);
    if (sh) src.tab = a.stable, src.NP = a.NPs;
    src.open(L, c_end);
    if (c_begin < c_end) src.fetch_k(kreg, ksc, (int64_t)c_begin * kMxsChunk, L, klo, khi, i, g, a.vec);

    for (int c = c_begin; c < c_end; ++c) {
        const int64_t key0 = (int64_t)c * kMxsChunk;
        src.fetch_vt(vreg, vsc, key0, L, vlo, vhi, i, g, a.vec);                          // in flight through phases 1 and 2

        // ---- phase 1 -----------------------------------------------------------------------------------------------------------
        f32x4 s[8];
        switch (a.qk_format) {                                  // (kernel-uniform)
            case QS_MX_FP8_E4M3: mxd_scores<QS_MX_FP8_E4M3>(s, kreg, ksc, fq, sq); break;
            case QS_MX_FP8_E5M2: mxd_scores<QS_MX_FP8_E5M2>(s, kreg, ksc, fq, sq); break;
            case QS_MX_FP6_E2M3: mxd_scores<QS_MX_FP6_E2M3>(s, kreg, ksc, fq, sq); break;
            case QS_MX_FP6_E3M2: mxd_scores<QS_MX_FP6_E3M2>(s, kreg, ksc, fq, sq); break;
            default: mxd_scores<QS_MX_FP4_E2M1>(s, kreg, ksc, fq, sq); break;
        }
        if (c + 1 < c_end)                                      // in flight through phases 2 and 3
            src.fetch_k(kreg, ksc, key0 + kMxsChunk, L, klo, khi, i, g, a.vec);

        // ---- phase 2: the paged kernel's, the mask by the lane's own limit ---------------------------------------------------------
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

        // the scale bytes of the row's four blocks; 127: a block wholly past Lt.  A row whose own L_b ends before the block has all-zero
        // weights there: zero codes under whatever byte the quantizer gives zero, the same product as the definition's byte 127
        uint32_t sw = 0x7f7f7f7fu;
#pragma unroll
        for (int bk = 0; bk < 4; ++bk) {
            uint32_t pc[2] = {0u, 0u};
            if (key0 + 32 * bk < L) {                           // (wave-uniform)
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
        // the bounce is the wave's own: its LDS operations complete in order, the fence keeps the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ---- phase 3 -----------------------------------------------------------------------------------------------------------
        f32x4 o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        mxd_pv_p(a.p_format, a.v_format, o, vreg, vsc, row, (int)((sw >> (8 * g)) & 0xffu), dv, g);       // (kernel-uniform switches)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the next chunk's codes are written behind these reads)
        __builtin_amdgcn_wave_barrier();

        const bool live = key0 < Lim;                           // else the row's limit admits no column of this chunk: its state stays
        m = live ? m2 : m;
        Z = live ? Z * alpha + z : Z;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (16 * j < dv)                                    // (kernel-uniform)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[j][r] = live ? acc[j][r] * alpha + o[j][r] : acc[j][r];
    }

    // ---- epilogue: lane 16 g + i holds the columns 16 j + 4 g + {0..3} of its row; always a record, n >= 2 --------------------------------
    int badi = (int)bad;
    badi |= __shfl_xor(badi, 16, 64);
    badi |= __shfl_xor(badi, 32, 64);
    if (!rin) return;
    float* rec = a.ws + ((((int64_t)b * a.Hkv + hk) * R + rho) * a.n + idx) * (dv + 3);
    if (g == 0) rec[0] = m, rec[1] = Z, rec[2] = badi ? 1.0f : 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (16 * j + 4 * g + r < dv) rec[3 + 16 * j + 4 * g + r] = acc[j][r];
}

}  // namespace qs
