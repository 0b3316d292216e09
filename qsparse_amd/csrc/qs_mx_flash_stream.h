// Attention on MX codes in ONE launch for ANY key length (include/qsparse_hip.h, "MX flash attention, streamed"): the key axis is
// walked in chunks of 128 with a running maximum m, a running sum Z and a rescaled accumulator acc[dv] per query row -- registers
// and LDS do not depend on S.  The numerics are the header's chunk recurrence, NOT the chain's: e = E(u - m') is quantized to
// p_format unnormalised, the division by Z happens once, after the last chunk.
//
// Work split.  As qs_mx_flash.h: one work-group of 4 waves per (slice, 64 query rows), wave w owns the 16 rows t0 + 16 w ..; lane
// 16 g + i holds query i in every accumulator (scores: keys 16 f + 4 g + {0..3}; o and acc: columns 16 j + 4 g + {0..3} of dv), so m,
// Z, alpha and the flags are per lane and agree across the four g lanes of a query.
//
// Per chunk c (a run-time loop, nothing unrolled over S):
//   phase 1  s[8] = 8 MFMAs of the K tile (SrcA) against the wave's Q fragment (SrcB, loaded once, global -> register), each from a
//            zeroed accumulator: mx_bmm's bits on that slice of k.
//   phase 2  u = s * scale (+ mask), -inf at and behind the row's limit; the chunk maximum in-lane + __shfl_xor 16 / 32; m' =
//            max(m, .); e = E(u - m'), alpha = E(m - m'); z in _row_sum's order on 128 columns (quad, + fragments 4 / 2 / 1 apart,
//            __shfl_xor 32 / 16 -- the steps 64 and 32 add +0 and are dropped); e's blocks of 32 (two fragments x four g) through
//            qs_mx.h's scale and encode; a block wholly past S is zero codes under the byte 127.
//   phase 3  p's codes cross the per-wave LDS bounce of qs_mx_flash.h into mxg_pack16; o[8] = 8 MFMAs of the vt tile against them,
//            again from ZERO (the instruction's sum with an incoming C is no float32 add: profiles/mx_mfma_scale_probe.txt, 4), then
//            acc = acc * alpha + o and Z = Z * alpha + z on the VALU, a multiply and an add each (-ffp-contract=off).
//   A row whose causal limit lies at or before the chunk's first key keeps m, Z, acc by select.  With `causal` the loop ends at the
//   chunk that holds column t0 + 63; a mask elides nothing.
//
// Data movement.  ONE LDS tile per operand (K: 16 KB, vt: 16 KB), their scale bytes (128 rows x 4 blocks each: a thread brings two
// bytes, no wave reads a byte from memory that another one reads too) and the bounce (9 KB) = 42 KB: three work-groups per CU.  The
// next chunk is double-buffered in REGISTERS instead of LDS: K chunk c + 1 is issued at the top of iteration c, lands while phases 1
// and 2 run and is staged behind barrier A (every wave is past phase 1); vt chunk c + 1 is issued there, lands while phase 3 runs and
// is staged at the top of iteration c + 1, behind barrier B (every wave is done with the vt tile).  The two never live together: 16
// VGPRs.  Cost against two LDS buffers per operand: two barriers per chunk instead of one; gain: 42 KB instead of 75 KB.
//
// `vec` and the formats: as qs_mx_flash.h -- phase 1 is a function template on the format of q and k, phase 3 on those of p and vt,
// each behind a kernel-uniform switch at its one call inside the loop; the staging is switched on the code width alone.
#pragma once
#include "qs_mx_flash.h"

namespace qs {

constexpr int kMxsChunk = 128;                                  // keys per chunk: part of the definition
constexpr int kMxsScales = kMxsChunk * 4;                        // the scale bytes of a tile: 128 rows x 4 blocks
constexpr int kMxsLds = 2 * kMxfTile + 2 * kMxsScales + 4 * kMxfBounce;

// the thread's four 16-code pieces of the chunk of 128 rows from row0 and 128 codes from k0 of `codes` [rows, K], as mxg_stage takes them
__device__ __forceinline__ void mxs_fetch(u32x4 (&reg)[4], const uint8_t* __restrict__ codes, int64_t rows, int64_t K, int64_t row0,
                                          int64_t k0, int tid, int vec) {
    const int64_t kk = k0 + (tid & 7) * 16;
    const int left = (int)(K - kk < 16 ? K - kk : 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + (tid >> 3) + 32 * i;
        reg[i] = mxf_load16(codes, row < rows && kk < K, row * K + kk, left, vec);
    }
}

// the thread's two scale bytes of that chunk: blocks b0 + 2 (tid & 1) + {0, 1} of row row0 + (tid >> 1) of `scales` [rows, nb]; 127 outside
__device__ __forceinline__ uint32_t mxs_fetch_scales(const uint8_t* __restrict__ scales, int64_t rows, int64_t nb, int64_t row0, int64_t b0,
                                                     int tid) {
    const int64_t r = row0 + (tid >> 1), b = b0 + 2 * (tid & 1);
    return mx_scale(scales, r < rows && b < nb, r * nb + b) | (mx_scale(scales, r < rows && b + 1 < nb, r * nb + b + 1) << 8);
}

__device__ __forceinline__ void mxs_stage(uint8_t* tile, const u32x4 (&reg)[4], int tid, int bits) {      // (kernel-uniform)
    if (bits == 8) mxg_stage<8>(tile, reg, tid);
    else if (bits == 6) mxg_stage<6>(tile, reg, tid);
    else mxg_stage<4>(tile, reg, tid);
}

// phase 1 for the format FQ of q and k: the wave's 16 queries against the 128 keys of the tile, sk[4 r + b] the scale byte of block b
// of its row r
template <int FQ>
__device__ __forceinline__ void mxs_scores(f32x4 (&s)[8], const uint8_t* tile, const i32x8& fq, int sq, const uint8_t* sk, int i, int g) {
    using L = MxgLds<mxg_bits(FQ)>;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        s[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(L::get(tile, 16 * j + i, g), fq, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, FQ, FQ, 0,
                                                                (int)sk[4 * (16 * j + i) + g], 0, sq);
}

// phase 3 for the formats FP of p and FV of vt: o[j] = the wave's 16 queries against the rows 16 j .. of the vt tile over this chunk;
// `row`: the lane's query's 128 codes in the bounce, sp its scale byte of block g, sv[4 r + b] that of block b of the tile's row r
template <int FP, int FV>
__device__ __forceinline__ void mxs_pv(f32x4 (&o)[8], const uint8_t* tile, const uint8_t* row, int sp, const uint8_t* sv, int64_t dv, int i,
                                       int g) {
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
__device__ __forceinline__ void mxs_pv_v(int v_format, A&&... args) {
    switch (v_format) {
#define X(F) case F: mxs_pv<FP, F>(args...); break;
        QS_MXF_FORMATS(X)
#undef X
        default: mxs_pv<FP, QS_MX_FP4_E2M1>(args...); break;
    }
}

template <class... A>
__device__ __forceinline__ void mxs_pv_p(int p_format, int v_format, A&&... args) {
    switch (p_format) {
#define X(F) case F: mxs_pv_v<F>(v_format, args...); break;
        QS_MXF_FORMATS(X)
#undef X
        default: mxs_pv_v<QS_MX_FP4_E2M1>(v_format, args...); break;
    }
}

__global__ __launch_bounds__(kMxgThreads, 2) void mx_flash_stream_kernel(MxFormat fp, MxfArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxsLds];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int64_t slice = blockIdx.x / (unsigned)a.tiles, t0 = (int64_t)(blockIdx.x % (unsigned)a.tiles) * kMxfRows;
    const int64_t T = a.T, S = a.S, d = a.d, dv = a.dv;
    const int64_t nkb = (d + QS_MX_BLOCK - 1) / QS_MX_BLOCK, nsb = (S + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    const uint8_t* __restrict__ q = a.q + slice * T * d;
    const uint8_t* __restrict__ qs = a.qs + slice * T * nkb;
    const uint8_t* __restrict__ k = a.k + slice * S * d;
    const uint8_t* __restrict__ ks = a.ks + slice * S * nkb;
    const uint8_t* __restrict__ vt = a.vt + slice * dv * S;
    const uint8_t* __restrict__ vts = a.vts + slice * dv * nsb;
    uint8_t* ktile = lds;
    uint8_t* vtile = lds + kMxfTile;
    uint8_t* sk = lds + 2 * kMxfTile;
    uint8_t* sv = sk + kMxsScales;
    uint8_t* row = sv + kMxsScales + wave * kMxfBounce + i * kMxfBounceRow;         // this lane's query in the wave's bounce
    const int qb = mxg_bits(a.qk_format), vb = mxg_bits(a.v_format);
    const int64_t t = t0 + 16 * wave + i;                       // this lane's query row
    const bool tin = t < T;

    // the Q fragment and its scale byte, once
    const int64_t klo = qb == 8 ? 16 * g : 32 * g, khi = qb == 8 ? 64 + 16 * g : 32 * g + 16;
    const u32x4 qlo = mxf_load16(q, tin && klo < d, t * d + klo, (int)(d - klo < 16 ? d - klo : 16), a.vec);
    const u32x4 qhi = mxf_load16(q, tin && khi < d, t * d + khi, (int)(d - khi < 16 ? d - khi : 16), a.vec);
    const i32x8 fq = qb == 8 ? mxf_frag<8>(qlo, qhi) : (qb == 6 ? mxf_frag<6>(qlo, qhi) : mxf_frag<4>(qlo, qhi));
    const int sq = (int)mx_scale(qs, tin && g < nkb, t * nkb + g);

    // no row of the work-group admits a column at or behind s_end: the loop ends at the chunk that holds column s_end - 1
    const int64_t s_end = (a.causal && t0 + kMxfRows < S) ? t0 + kMxfRows : S;
    const int64_t chunks = (s_end + kMxsChunk - 1) / kMxsChunk;
    // a row past T admits nothing (and reads no mask): it is never stored
    const int64_t Lim = !tin ? 0 : ((a.causal && t + 1 < S) ? t + 1 : S);
    const int64_t mbase = a.mask ? ((slice * T + (tin ? t : 0)) % a.mask_rows) * S : 0;
    const float ninf = __uint_as_float(0xff800000u);

    u32x4 reg[4];                                               // the pieces in flight: K chunk c + 1, then vt chunk c + 1
    uint32_t rs;                                                // ... and their two scale bytes
    mxs_fetch(reg, k, S, d, 0, 0, tid, a.vec);
    rs = mxs_fetch_scales(ks, S, nkb, 0, 0, tid);
    mxs_stage(ktile, reg, tid, qb);
    *(uint16_t*)(sk + 2 * tid) = (uint16_t)rs;
    mxs_fetch(reg, vt, dv, S, 0, 0, tid, a.vec);
    rs = mxs_fetch_scales(vts, dv, nsb, 0, 0, tid);

    float m = ninf, Z = 0.0f;
    bool bad = false;
    f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int64_t c = 0; c < chunks; ++c) {
        const int64_t key0 = c * kMxsChunk;
        const bool more = c + 1 < chunks;                       // (uniform over the work-group)
        mxs_stage(vtile, reg, tid, vb);                         // vt chunk c (free since barrier B of the chunk before)
        *(uint16_t*)(sv + 2 * tid) = (uint16_t)rs;
        if (c == 0) __syncthreads();                            // (the K tile of the prologue)
        if (more) {                                             // in flight through phases 1 and 2
            mxs_fetch(reg, k, S, d, key0 + kMxsChunk, 0, tid, a.vec);
            rs = mxs_fetch_scales(ks, S, nkb, key0 + kMxsChunk, 0, tid);
        }

        // ---- phase 1 -----------------------------------------------------------------------------------------------------------
        f32x4 s[8];
        switch (a.qk_format) {                                  // (kernel-uniform)
            case QS_MX_FP8_E4M3: mxs_scores<QS_MX_FP8_E4M3>(s, ktile, fq, sq, sk, i, g); break;
            case QS_MX_FP8_E5M2: mxs_scores<QS_MX_FP8_E5M2>(s, ktile, fq, sq, sk, i, g); break;
            case QS_MX_FP6_E2M3: mxs_scores<QS_MX_FP6_E2M3>(s, ktile, fq, sq, sk, i, g); break;
            case QS_MX_FP6_E3M2: mxs_scores<QS_MX_FP6_E3M2>(s, ktile, fq, sq, sk, i, g); break;
            default: mxs_scores<QS_MX_FP4_E2M1>(s, ktile, fq, sq, sk, i, g); break;
        }

        // ---- phase 2 -----------------------------------------------------------------------------------------------------------
        float mc = ninf;
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            const int64_t c0 = key0 + 16 * f + 4 * g;
            float am[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (a.mask) {
                if (a.vec) {                                    // (S % 16 == 0: the four are inside the row together; the limit cuts anywhere)
                    if (c0 < Lim) {
                        const u32x4 w = *(const u32x4*)(a.mask + mbase + c0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) am[r] = __uint_as_float(w[r]);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (c0 + r < Lim) am[r] = a.mask[mbase + c0 + r];
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float w = s[f][r] * a.scale;
                if (a.mask) w = w + am[r];                      // (kernel-uniform; an absent mask is not added)
                w = c0 + r < Lim ? w : ninf;
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

        uint32_t sw = 0x7f7f7f7fu;                              // the scale bytes of the query's four blocks; 127: a block wholly past S
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            uint32_t pc[2] = {0u, 0u};
            if (key0 + 32 * b < S) {                            // (kernel-uniform)
                uint32_t am = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t ab = mx_abs_bits(s[2 * b + h][r]);
                        am = ab > am ? ab : am;
                    }
#pragma unroll
                for (int off = 16; off < 64; off <<= 1) {
                    const uint32_t o = (uint32_t)__shfl_xor((int)am, off, 64);
                    am = o > am ? o : am;
                }
                const MxScale sc = mx_scale(am, fp);
                sw = (sw & ~(0xffu << (8 * b))) | (sc.byte << (8 * b));
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        uint32_t sg;
                        const float qv = mx_round_abs(s[2 * b + h][r], sc, fp, sg);
                        pc[h] |= mx_code(qv, sg, sc, fp) << (8 * r);
                    }
            }
            *(uint32_t*)(row + 32 * b + 4 * g) = pc[0];
            *(uint32_t*)(row + 32 * b + 16 + 4 * g) = pc[1];
        }

        __syncthreads();                                        // A: the vt tile and the bounce are written, every wave is past phase 1
        if (more) {
            mxs_stage(ktile, reg, tid, qb);
            *(uint16_t*)(sk + 2 * tid) = (uint16_t)rs;
            mxs_fetch(reg, vt, dv, S, 0, key0 + kMxsChunk, tid, a.vec);         // in flight through phase 3
            rs = mxs_fetch_scales(vts, dv, nsb, 0, 4 * (c + 1), tid);
        }

        // ---- phase 3 -----------------------------------------------------------------------------------------------------------
        f32x4 o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        mxs_pv_p(a.p_format, a.v_format, o, vtile, row, (int)((sw >> (8 * g)) & 0xffu), sv, dv, i, g);     // (kernel-uniform switches)

        const bool live = !a.causal || key0 < t + 1;            // else the row's limit admits no column of this chunk: its state stays
        m = live ? m2 : m;
        Z = live ? Z * alpha + z : Z;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (16 * j < dv)                                    // (kernel-uniform)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[j][r] = live ? acc[j][r] * alpha + o[j][r] : acc[j][r];
        __syncthreads();                                        // B: the K tile is written, every wave is done with the vt tile and the bounce
    }

    // ---- epilogue: lane 16 g + i holds the columns 16 j + 4 g + {0..3} of row t ------------------------------------------------------
    int badi = (int)bad;
    badi |= __shfl_xor(badi, 16, 64);
    badi |= __shfl_xor(badi, 32, 64);
    if (!tin) return;
    const bool rownan = badi != 0 || Z == 0.0f;                 // a NaN or +inf in u, or nothing admitted
    void* y = (uint8_t*)a.y + slice * T * dv * (a.ydt == QS_F32 ? 4 : 2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t n = 16 * j + 4 * g;
        if (n >= dv) continue;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = rownan ? __uint_as_float(0x7fc00000u) : acc[j][r] / Z;
        mx_store4(y, a.ydt, t * dv + n, v, n, dv, a.y_vec);
    }
}

}  // namespace qs
