// Grouped-query attention on MX codes for decoding (include/qsparse_hip.h, "MX flash attention, decode"): a few query tokens against a
// long cache, the key axis cut into `n` splits that run side by side, the valid length of each sequence read from device memory.
// The numerics inside a split are the streamed kernel's chunk recurrence (qs_mx_flash_stream.h) on the cache sliced to L_b keys.
//
// Work split.  The unit of work is a WAVE, not a work-group: wave item = ((b Hkv + hk) tiles + tile) n + split owns 16 of the R = r T
// packed query rows of one (sequence, kv head) and one split of its keys.  A (sequence, kv head) has at most 16 rows per MFMA tile, so
// a chunk of K or vt is consumed by ONE wave: staging it in LDS would buy no reuse, and there is no barrier in the kernel.  The four
// waves of a work-group are four independent items.
//
// Row packing.  Row rho of the group is query head hk r + rho / T, token rho % T.  The lane map is that of qs_mx_flash.h: lane 16 g + i
// holds row 16 tile + i in every accumulator, so m, Z, alpha, the shuffles by 16 / 32 and the quantizer's block maximum carry over.
//
// Operands.  K and vt fragments go from global memory straight into the MFMA's SrcA registers, as the Q fragment always did: for tile j
// lane 16 g + i loads row key0 + 16 j + i of K (row 16 j + i of vt, from column key0) in two 16-byte pieces, mxf_frag packs them.  The
// four g lanes of a row cover whole 128-byte rows of FP8 codes.  The scale byte of block g comes per lane.
//
// Prefetch, in registers: TWO sets of 16 pieces + 8 scale bytes.  vt of chunk c is issued at the top of iteration c and lands while
// phases 1 and 2 run; K of chunk c + 1 is issued behind phase 1 (its registers are free then) and lands while phases 2 and 3 run.
//
// Length.  L = clamp(kv_len[b], 0, S), one vector load per wave.  Keys >= L are loaded as zero codes under the byte 127 and get u = -inf
// by select; vt codes at columns >= L are cleared at the load (only the chunk that holds L pays for the byte masks), a vt scale block
// wholly past L reads 127.  The loop ends at min(split end, chunk holding L - 1, chunk holding the tile's last admitted key); a wave
// with nothing to do writes the empty state.  Row t's limit is L (or, causal, bottom-right: clamp(L - T + t + 1, 0, L)).
//
// Output.  n == 1: the wave divides and writes y.  n > 1: it writes (m, Z, bad, acc[dv]) in float32 to the workspace record
// ((b Hkv + hk) R + rho) n + split of dv + 3 floats, and mx_flash_decode_combine_kernel -- one thread per (row, 4 columns) -- combines the
// n records in ascending order, a multiply and an add each, divides and rounds to ydt.  No atomics, no counters.
//
// LDS: the per-wave bounce of p's codes (4 x 2.25 KB), nothing else.  Formats: kernel-uniform run-time switches, as qs_mx_flash_stream.h.
#pragma once
#include "qs_mx_flash.h"

namespace qs {

constexpr int kMxdMaxRows = 64;                                 // R = r T
constexpr int kMxsChunk = 128;                                  // keys per chunk, as qs_mx_flash_stream.h: part of the definition

struct MxdArgs {
    const uint8_t* __restrict__ q;
    const uint8_t* __restrict__ qs;
    const uint8_t* __restrict__ k;
    const uint8_t* __restrict__ ks;
    const uint8_t* __restrict__ vt;
    const uint8_t* __restrict__ vts;
    const int32_t* __restrict__ kv_len;                         // [B] or null
    float* __restrict__ ws;                                     // the split states; read only with n > 1
    void* __restrict__ y;
    int64_t items;                                              // B Hkv tiles n
    int T, S, d, dv, Hkv, r, R, tiles, n, cps;                  // cps: chunks per split
    float scale;
    int qk_format, p_format, v_format, ydt, causal, vec, y_vec;
};

// the first `nvalid` of the piece's 16 codes, the others cleared
__device__ __forceinline__ u32x4 mxd_clip(u32x4 v, int nvalid) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int nb = nvalid - 4 * w;
        v[w] = nb >= 4 ? v[w] : (nb <= 0 ? 0u : v[w] & ((1u << (8 * nb)) - 1u));
    }
    return v;
}

// the lane's pieces and scale bytes of the 128 keys from key0: rows key0 + 16 j + i of k [L.., d], pieces at lo / hi along d
__device__ __forceinline__ void mxd_fetch_k(u32x4 (&reg)[16], uint32_t (&sc)[8], const uint8_t* __restrict__ k, const uint8_t* __restrict__ ks,
                                            int64_t key0, int L, int d, int nkb, int lo, int hi, int i, int g, int vec) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t key = key0 + 16 * j + i;
        const bool in = key < L;
        reg[2 * j] = mxf_load16(k, in && lo < d, key * d + lo, d - lo < 16 ? d - lo : 16, vec);
        reg[2 * j + 1] = mxf_load16(k, in && hi < d, key * d + hi, d - hi < 16 ? d - hi : 16, vec);
        sc[j] = mx_scale(ks, in && g < nkb, key * nkb + g);
    }
}

// ... of the 128 columns from key0 of vt [dv, S], rows 16 j + i, pieces at key0 + lo / hi along S; columns >= L cleared, a scale block
// wholly past L read as 127
__device__ __forceinline__ void mxd_fetch_vt(u32x4 (&reg)[16], uint32_t (&sc)[8], const uint8_t* __restrict__ vt,
                                             const uint8_t* __restrict__ vts, int64_t key0, int L, int S, int dv, int nsb, int lo, int hi, int i,
                                             int g, int vec) {
    const int64_t c0 = key0 + lo, c1 = key0 + hi, kb = key0 / QS_MX_BLOCK + g;
    const int n0 = (int)(L - c0 < 16 ? L - c0 : 16), n1 = (int)(L - c1 < 16 ? L - c1 : 16);      // (<= 0: nothing of the piece is valid)
    const bool cut = key0 + kMxsChunk > L;                      // (wave-uniform: the chunk that holds L)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (16 * j < dv) {                                      // (kernel-uniform)
            const int64_t row = 16 * j + i;
            const bool in = row < dv;
            u32x4 a = mxf_load16(vt, in && n0 > 0, row * S + c0, n0, vec), b = mxf_load16(vt, in && n1 > 0, row * S + c1, n1, vec);
            if (cut) a = mxd_clip(a, n0), b = mxd_clip(b, n1);
            reg[2 * j] = a, reg[2 * j + 1] = b;
            sc[j] = mx_scale(vts, in && kb * QS_MX_BLOCK < L, row * nsb + kb);
        }
    }
}

// phase 1 for the format FQ of q and k: the wave's 16 rows against the 128 keys whose pieces `reg` holds
template <int FQ>
__device__ __forceinline__ void mxd_scores(f32x4 (&s)[8], const u32x4 (&reg)[16], const uint32_t (&sc)[8], const i32x8& fq, int sq) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
        s[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(mxf_frag<mxg_bits(FQ)>(reg[2 * j], reg[2 * j + 1]), fq,
                                                                f32x4{0.0f, 0.0f, 0.0f, 0.0f}, FQ, FQ, 0, (int)sc[j], 0, sq);
}

// phase 3 for the formats FP of p and FV of vt: `row` the lane's row's 128 codes in the bounce, sp its scale byte of block g
template <int FP, int FV>
__device__ __forceinline__ void mxd_pv(f32x4 (&o)[8], const u32x4 (&reg)[16], const uint32_t (&sc)[8], const uint8_t* row, int sp, int dv,
                                       int g) {
    constexpr int PB = mxg_bits(FP);
    const int plo = PB == 8 ? 16 * g : 32 * g, phi = PB == 8 ? 64 + 16 * g : 32 * g + 16;
    const i32x8 fpv = mxf_frag<PB>(*(const u32x4*)(row + plo), *(const u32x4*)(row + phi));
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (16 * j < dv)                                        // (kernel-uniform)
            o[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(mxf_frag<mxg_bits(FV)>(reg[2 * j], reg[2 * j + 1]), fpv,
                                                                    f32x4{0.0f, 0.0f, 0.0f, 0.0f}, FV, FP, 0, (int)sc[j], 0, sp);
}

template <int FP, class... A>
__device__ __forceinline__ void mxd_pv_v(int v_format, A&&... args) {
    switch (v_format) {
#define X(F) case F: mxd_pv<FP, F>(args...); break;
        QS_MXF_FORMATS(X)
#undef X
        default: mxd_pv<FP, QS_MX_FP4_E2M1>(args...); break;
    }
}

template <class... A>
__device__ __forceinline__ void mxd_pv_p(int p_format, int v_format, A&&... args) {
    switch (p_format) {
#define X(F) case F: mxd_pv_v<F>(v_format, args...); break;
        QS_MXF_FORMATS(X)
#undef X
        default: mxd_pv_v<QS_MX_FP4_E2M1>(v_format, args...); break;
    }
}

// (`inline`, here and on the combine kernel: qs_mx_flash_decode_paged.h includes this header into a second unit)
inline __global__ __launch_bounds__(kMxgThreads, 1) void mx_flash_decode_kernel(MxFormat fp, MxdArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kMxfBounce];
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    if (item >= a.items) return;                                // (no barrier anywhere: a wave may leave)
    const int split = (int)(item % a.n), tile = (int)(item / a.n % a.tiles);
    const int64_t bh = item / a.n / a.tiles;                    // b Hkv + hk
    const int b = (int)(bh / a.Hkv), hk = (int)(bh % a.Hkv);
    const int T = a.T, S = a.S, d = a.d, dv = a.dv;
    const int nkb = (d + QS_MX_BLOCK - 1) / QS_MX_BLOCK, nsb = (S + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    const uint8_t* __restrict__ k = a.k + bh * S * d;
    const uint8_t* __restrict__ ks = a.ks + bh * S * nkb;
    const uint8_t* __restrict__ vt = a.vt + bh * dv * S;
    const uint8_t* __restrict__ vts = a.vts + bh * dv * nsb;
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
    if (c_begin < c_end) mxd_fetch_k(kreg, ksc, k, ks, (int64_t)c_begin * kMxsChunk, L, d, nkb, klo, khi, i, g, a.vec);

    for (int c = c_begin; c < c_end; ++c) {
        const int64_t key0 = (int64_t)c * kMxsChunk;
        mxd_fetch_vt(vreg, vsc, vt, vts, key0, L, S, dv, nsb, vlo, vhi, i, g, a.vec);      // in flight through phases 1 and 2

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
            mxd_fetch_k(kreg, ksc, k, ks, key0 + kMxsChunk, L, d, nkb, klo, khi, i, g, a.vec);

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

// y from the n split states of each row, in the definition's order: M = max m_i, a_i = E(m_i - M), Z = Z_0 a_0 (+ Z_i a_i ...), acc
// likewise, every multiply and add on its own; one thread per (output row, 4 columns)
inline __global__ __launch_bounds__(256) void mx_flash_decode_combine_kernel(MxdArgs a, int64_t quads) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int nq = (a.dv + 3) / 4;
    if (e >= quads) return;
    const int n0 = (int)(e % nq) * 4;
    const int64_t orow = e / nq;                                // row of y: (b Hq + h) T + t
    const int t = (int)(orow % a.T);
    const int64_t bhq = orow / a.T;                             // b Hq + h = (b Hkv + hk) r + h % r
    const int64_t bh = bhq / a.r;
    const int rho = (int)(bhq % a.r) * a.T + t;
    const float* __restrict__ rec = a.ws + (bh * a.R + rho) * a.n * (a.dv + 3);
    const int stride = a.dv + 3;
    float M = __uint_as_float(0xff800000u);
    for (int s = 0; s < a.n; ++s) M = fmaxf(M, rec[(int64_t)s * stride]);
    float Z = 0.0f, v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool bad = false;
    for (int s = 0; s < a.n; ++s) {
        const float* __restrict__ p = rec + (int64_t)s * stride;
        const float w = msx_exp(p[0] - M);
        bad |= p[2] != 0.0f;
        Z = s == 0 ? p[1] * w : Z + p[1] * w;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (n0 + r < a.dv) v[r] = s == 0 ? p[3 + n0 + r] * w : v[r] + p[3 + n0 + r] * w;
    }
    const bool rownan = bad || Z == 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = rownan ? __uint_as_float(0x7fc00000u) : v[r] / Z;
    mx_store4(a.y, a.ydt, orow * a.dv + n0, v, n0, a.dv, a.y_vec);
}

}  // namespace qs
