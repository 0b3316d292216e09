// mx_flash_decode_kernel (qs_mx_flash_decode.h) on a PAGED cache (include/qsparse_hip.h, "MX flash attention, paged decode"): the keys of
// sequence b live in pages of `page` = 2^lg keys (>= 32) out of one pool, k_pool [P, Hkv, page, d] and vt_pool [P, Hkv, dv, page];
// position j is row / column j % page of pool page block_table[b, j / page].  The work split (a wave per (b, hk, 16 packed rows, split), no
// barrier), the lane map, phases 1, 2 and 3, the split workspace and mx_flash_decode_combine_kernel are qs_mx_flash_decode.h's.  Lifting
// that kernel's body -- or its phase 2 alone -- into a function both kernels call moved its register allocation (AGPRs 101 -> 106 /
// 104), so it stays as it is and the wave item is stated here a second time; the device functions are shared.
//
// What is new is address generation, and it keeps the dependent load entry -> page base -> K off the per-chunk path:
//   - The table lives in ONE vector register per wave: lane l holds the entry of page 64 w + l of the sequence, w the current window.  It
//     is loaded where (64 w + l) * page < min(L, 128 c_end) -- the wave's last admitted key, so an entry the definition calls dead is never
//     loaded -- and an entry outside [0, P) becomes -1 there and then.  One load at wave start serves 64 pages (2048 keys at page 32, the
//     whole split at page >= 128 up to 8192 keys); a longer split reloads in a wave-uniform branch when a chunk enters the next window.
//     A chunk never straddles a window: it spans 128 / page <= 4 pages from a page number that is a multiple of that.
//   - Per chunk the page numbers come out of that register by v_readlane into scalar registers: at most four per chunk (page 32), one
//     for page >= 128.  Page bases are wave-uniform scalar arithmetic; no vector register is added to the loop's live set for them.
//   - K row 16 j + i of the chunk lies in the chunk's page (16 j) >> lg, uniform per j.  A vt piece at column offset lo / hi lies in page
//     lo >> lg, which depends on g: a per-lane select among the (at most four) uniform page numbers.  The vt scale block g likewise.
//   - A dead page (entry -1) predicates its loads off: zero codes under the byte 127 for K and vt, no address formed from the entry.
//   - VEC route: d % 16 == 0 and q_codes, k_pool, vt_pool 16-byte aligned; page >= 32 keeps every page base and vt row aligned.
// Table reads are vector loads followed by readlane; nothing is written through the scalar path.
#pragma once
#include "qs_mx_flash_decode.h"

namespace qs {

struct MxdPagedArgs : MxdArgs {                                 // k, ks, vt, vts: the pool's; S = NP page
    const int32_t* __restrict__ table;                          // [B, NP]
    int P, NP, lg;                                              // pool pages, pages per sequence, log2(page)
};

__device__ __forceinline__ int mxp_sel4(const int (&v)[4], int q) { return q == 0 ? v[0] : (q == 1 ? v[1] : (q == 2 ? v[2] : v[3])); }

// the paged source of a wave's K and vt
struct MxdPaged {
    const uint8_t* __restrict__ k;
    const uint8_t* __restrict__ ks;
    const uint8_t* __restrict__ vt;
    const uint8_t* __restrict__ vts;
    const int32_t* __restrict__ tab;                            // row b of the table
    int P, NP, lg, d, dv, nkb, Hkv, hk;
    int ent, win, last;                                         // lane l: entry of page 64 win + l or -1; keys < last are needed

    __device__ __forceinline__ MxdPaged(const MxdPagedArgs& a, int b, int hk_)
        : k(a.k), ks(a.ks), vt(a.vt), vts(a.vts), tab(a.table + (int64_t)b * a.NP), P(a.P), NP(a.NP), lg(a.lg), d(a.d), dv(a.dv),
          nkb((a.d + QS_MX_BLOCK - 1) / QS_MX_BLOCK), Hkv(a.Hkv), hk(hk_), ent(-1), win(-1), last(0) {}

    // L and the wave's last chunk + 1 are known: the keys the wave may load
    __device__ __forceinline__ void open(int L, int c_end) {
        const int64_t e = (int64_t)c_end * kMxsChunk;
        last = e < L ? (int)e : L;
    }
    // the entry of page n (wave-uniform; n * page < 128 c_end): a pool page number, or -1 for a page that is dead or not needed
    __device__ __forceinline__ int entry(int n) {
        n = __builtin_amdgcn_readfirstlane(n);
        if ((n >> 6) != win) {                                  // (wave-uniform: once per 64 pages)
            win = n >> 6;
            const int64_t pn = (int64_t)win * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            int e = -1;
            if (pn < NP && (pn << lg) < last) e = tab[pn];
            ent = e >= 0 && e < P ? e : -1;
        }
        return __builtin_amdgcn_readlane(ent, n & 63);
    }
    // the pool pages of the chunk at key0: pg[q] for the chunk's page q; -1 where dead or behind the chunk's pages
    __device__ __forceinline__ void pages(int64_t key0, int (&pg)[4]) {
        const int npc = lg >= 7 ? 1 : kMxsChunk >> lg, n0 = (int)(key0 >> lg);
#pragma unroll
        for (int q = 0; q < 4; ++q) pg[q] = q < npc ? entry(n0 + q) : -1;
    }

    // mxd_fetch_k through the table
    __device__ __forceinline__ void fetch_k(u32x4 (&reg)[16], uint32_t (&sc)[8], int64_t key0, int L, int lo, int hi, int i, int g, int vec) {
        int pg[4];
        pages(key0, pg);
        const int pm = (1 << lg) - 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = mxp_sel4(pg, (16 * j) >> lg);         // (wave-uniform)
            const int64_t key = key0 + 16 * j + i;
            const bool in = key < L && p >= 0;
            const int64_t row = ((((int64_t)(p < 0 ? 0 : p) * Hkv + hk)) << lg) + ((int)key & pm);        // of k_pool [P Hkv page, d]
            reg[2 * j] = mxf_load16(k, in && lo < d, row * d + lo, d - lo < 16 ? d - lo : 16, vec);
            reg[2 * j + 1] = mxf_load16(k, in && hi < d, row * d + hi, d - hi < 16 ? d - hi : 16, vec);
            sc[j] = mx_scale(ks, in && g < nkb, row * nkb + g);
        }
    }

    // mxd_fetch_vt through the table: the pieces at lo / hi and the scale block g each pick their page per lane
    __device__ __forceinline__ void fetch_vt(u32x4 (&reg)[16], uint32_t (&sc)[8], int64_t key0, int L, int lo, int hi, int i, int g, int vec) {
        int pg[4];
        pages(key0, pg);
        const int pm = (1 << lg) - 1;
        const int64_t c0 = key0 + lo, c1 = key0 + hi, cs = key0 + QS_MX_BLOCK * g;
        const int n0 = (int)(L - c0 < 16 ? L - c0 : 16), n1 = (int)(L - c1 < 16 ? L - c1 : 16);      // (<= 0: nothing of the piece is valid)
        const bool cut = key0 + kMxsChunk > L;                  // (wave-uniform: the chunk that holds L)
        const int p0 = mxp_sel4(pg, lo >> lg), p1 = mxp_sel4(pg, hi >> lg), ps = mxp_sel4(pg, (QS_MX_BLOCK * g) >> lg);
        // row 0 of (page, hk) in vt_pool [P Hkv dv, page] and vt_pool_scales [P Hkv dv, page / 32], plus the column inside the page
        const int64_t b0 = ((((int64_t)(p0 < 0 ? 0 : p0) * Hkv + hk) * dv) << lg) + ((int)c0 & pm);
        const int64_t b1 = ((((int64_t)(p1 < 0 ? 0 : p1) * Hkv + hk) * dv) << lg) + ((int)c1 & pm);
        const int64_t bs = ((((int64_t)(ps < 0 ? 0 : ps) * Hkv + hk) * dv) << (lg - 5)) + (((int)cs & pm) >> 5);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (16 * j < dv) {                                  // (kernel-uniform)
                const int64_t row = 16 * j + i;
                const bool in = row < dv;
                u32x4 a = mxf_load16(vt, in && n0 > 0 && p0 >= 0, b0 + (row << lg), n0, vec);
                u32x4 b = mxf_load16(vt, in && n1 > 0 && p1 >= 0, b1 + (row << lg), n1, vec);
                if (cut) a = mxd_clip(a, n0), b = mxd_clip(b, n1);
                reg[2 * j] = a, reg[2 * j + 1] = b;
                sc[j] = mx_scale(vts, in && cs < L && ps >= 0, bs + (row << (lg - 5)));
            }
        }
    }
};

// (`inline`: qs_mx_flash_decode_shared.h includes this header into a second unit; the kernel's code is the same instruction for instruction)
inline __global__ __launch_bounds__(kMxgThreads, 1) void mx_flash_decode_paged_kernel(MxFormat fp, MxdPagedArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kMxfBounce];
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    if (item >= a.items) return;                                // (no barrier anywhere: a wave may leave)
    const int split = (int)(item % a.n), tile = (int)(item / a.n % a.tiles);
    const int64_t bh = item / a.n / a.tiles;                    // b Hkv + hk
    const int b = (int)(bh / a.Hkv), hk = (int)(bh % a.Hkv);
    const int T = a.T, S = a.S, d = a.d, dv = a.dv;
    const int nkb = (d + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    MxdPaged src(a, b, hk);
    uint8_t* row = lds + wave * kMxfBounce + i * kMxfBounceRow; // this lane's row in the wave's bounce
    const int qb = mxg_bits(a.qk_format), vb = mxg_bits(a.v_format);
    const int klo = qb == 8 ? 16 * g : 32 * g, khi = qb == 8 ? 64 + 16 * g : 32 * g + 16;
    const int vlo = vb == 8 ? 16 * g : 32 * g, vhi = vb == 8 ? 64 + 16 * g : 32 * g + 16;

    // this lane's packed row: query head hk r + rho / T, token rho % T
    const int rho = 16 * tile + i;
    const bool rin = rho < a.R;
    const int tok = rin ? rho % T : 0;
    const int64_t qrow = ((int64_t)b * a.Hkv * a.r + hk * a.r + (rin ? rho / T : 0)) * T + tok;      // row of q [B Hq T, d] and of y

    // L: one vector load (the address is the lane's own), then wave-uniform
    int L = S;
    if (a.kv_len) {
        const int raw = a.kv_len[b + (int)__builtin_amdgcn_mbcnt_lo(0u, 0u)];     // (+ 0, in a vector register)
        L = __builtin_amdgcn_readfirstlane(raw < 0 ? 0 : (raw > S ? S : raw));
    }
    int Lim = !rin ? 0 : L;                                     // the row admits the keys j < Lim
    if (a.causal && rin) Lim = L - T + tok + 1 < 0 ? 0 : L - T + tok + 1;
    int top = Lim;                                              // the tile's last admitted key + 1
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const int o = __shfl_xor(top, off, 64);
        top = o > top ? o : top;
    }
    top = __builtin_amdgcn_readfirstlane(top);
    const int c_begin = split * a.cps;
    int c_end = (top + kMxsChunk - 1) / kMxsChunk;
    c_end = c_end < c_begin + a.cps ? c_end : c_begin + a.cps;

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

    // ---- epilogue: lane 16 g + i holds the columns 16 j + 4 g + {0..3} of row rho -----------------------------------------------------
    int badi = (int)bad;
    badi |= __shfl_xor(badi, 16, 64);
    badi |= __shfl_xor(badi, 32, 64);
    if (!rin) return;
    if (a.n == 1) {
        const bool rownan = badi != 0 || Z == 0.0f;             // a NaN or +inf in u, or nothing admitted
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = 16 * j + 4 * g;
            if (n >= dv) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = rownan ? __uint_as_float(0x7fc00000u) : acc[j][r] / Z;
            mx_store4(a.y, a.ydt, qrow * dv + n, v, n, dv, a.y_vec);
        }
    } else {
        float* rec = a.ws + ((bh * a.R + rho) * a.n + split) * (dv + 3);
        if (g == 0) rec[0] = m, rec[1] = Z, rec[2] = badi ? 1.0f : 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (16 * j + 4 * g + r < dv) rec[3 + 16 * j + 4 * g + r] = acc[j][r];
    }
}

}  // namespace qs
