// Attention on MX codes in ONE launch (include/qsparse_hip.h, "MX flash attention"): for every slice g and query row t
//   s   = mx_bmm(q, k)                                  float32 [T, S]      (qs_mx_bmm.h)
//   p   = mx_softmax_quantize(s, mask, scale, causal)   codes of p_format   (qs_mx_softmax.h)
//   out = mx_bmm(p, vt)                                 [T, dv] in ydt
// bit for bit, and neither s, nor p, nor p's codes ever exist in memory.  The kernel keeps a whole row of scores on chip: S <= 512,
// d <= 128, dv <= 128.
//
// Work split.  One work-group of 4 waves per (slice, 64 query rows), the slice folded into the linear block index as MxbBlock does;
// wave w owns the 16 query rows t0 + 16 w .. and the whole key axis.  T = 197 pads to 208 rows, not 256.
//
// Phase 1, scores.  Keys on SrcA, queries on SrcB, as mx_gemm_kernel puts B and A (lane maps: head of qs_mx_gemm.h): ONE step along d
// (d <= 128), zero codes and the scale byte 127 past d or S, accumulators zeroed first -- so a score is mx_bmm's bits.  K goes through
// LDS in chunks of 128 keys shared by the four waves (mxg_stage / MxgLds, one buffer, two barriers per chunk); a wave's Q fragment is
// loaded once, global -> register.  One MFMA per 16 keys leaves fragment f in 4 registers: lane 16 g + i holds query i and the keys
// 16 f + 4 g + {0..3} -- one quad of the softmax definition's row sum.  NF = 16 (S <= 256) or 32 (S <= 512) fragments are
// instantiated; fragments at or past ceil(S / 16) are skipped by a wave-uniform test.  With `causal` the chunks that start at or behind
// t0 + 64 are not loaded or multiplied: every column there lies behind every row's limit L, where u is -inf whatever s holds.
//
// Phase 2, softmax in the accumulator layout, every float32 operation of the definition on its own (-ffp-contract=off):
//   u = s * scale (+ mask); -inf at columns >= L, whose mask is not read.  m: in-lane, then __shfl_xor 16 and 32 (the 4 lanes of a
//   query).  e = msx_exp(u - m).  Z in the definition's order with no reordering: the quad sum (r0 + r1) + (r2 + r3) is in-lane, partial
//   sum j = 4 f + g is +0 + quad, the tree steps 64, 32, 16, 8, 4 over partial sums are register adds of fragments f and f + 16, 8, 4, 2,
//   1 (the NF = 16 form drops the step 64: it adds +0 to a sum that is never -0), the steps 2 and 1 are __shfl_xor 32 and 16.
//   p = e / Z; a block of 32 is two fragments x four g: its maximum is 8 values in-lane and two shuffles, then qs_mx.h's scale and
//   encode.  A lane keeps its 4 codes of a fragment in one register and every scale byte of its query in NF / 8 registers.
//   Exceptional rows (a NaN in u, m = +-inf) are the definition's: NaN as a whole through the scale byte 0xFF and zero codes.
//
// Phase 3, P . V.  vt on SrcA, p on SrcB, as mx_bmm(p, vt) puts them; S is walked in steps of 128 in ascending order, vt staged through
// the LDS buffer of phase 1.  SrcB wants 16 (FP8: 2 x 16) consecutive keys of one query per lane, the codes sit as 4 consecutive
// keys per lane across the four g lanes: they are exchanged through a 2.25 KB per-wave LDS bounce (16 queries x 128 codes, rows padded
// to 144 bytes) and packed with mxg_pack16.  The scale byte of block g is already in the lane.  Blocks wholly past S take the byte 127,
// codes past S are zero.  The epilogue is mx_epilogue's rounding and store (mx_store4); nothing past T or dv is written.
// No chunk of phase 3 is skipped under `causal`: an all-zero p block times a NaN scale byte or an Inf code of vt is NaN in mx_bmm.
//
// `vec` (kernel-uniform): d % 16 == 0, S % 16 == 0 and q, k, vt, mask 16-byte aligned -- 16-byte loads of codes and mask; otherwise
// byte / element loads each predicated on its own index: any d, S, base, the same bits.
//
// Formats.  The kernel is instantiated TWICE, on NF alone.  Phase 2 -- most of its text -- knows no format but p's run-time
// descriptor; phase 1 is a function template on the format of q and k, phase 3 one on the formats of p and vt, each reached through a
// kernel-uniform switch at its one call (5 and 25 cases of a few dozen instructions).  Templating the kernel on (p, vt) instead -- 50
// instantiations, each with its own copy of phase 2 -- gave the same registers and took 10 min 24 s to compile.
#pragma once
#include "qs_mx_host.h"
#include "qs_mx_softmax.h"

namespace qs {

constexpr int kMxfRows = 64;                                    // query rows per work-group: 16 per wave
constexpr int kMxfMaxS = 512, kMxfMaxD = 128;
constexpr int kMxfTile = MxgLds<8>::kBytes;                     // the K / vt chunk at its widest: 128 rows x 128 bytes
constexpr int kMxfBounceRow = 144;                              // 128 codes of a query + 16: rows spread over the banks, stay 16-byte aligned
constexpr int kMxfBounce = 16 * kMxfBounceRow;                  // per wave

struct MxfArgs {
    const uint8_t* __restrict__ q;
    const uint8_t* __restrict__ qs;
    const uint8_t* __restrict__ k;
    const uint8_t* __restrict__ ks;
    const uint8_t* __restrict__ vt;
    const uint8_t* __restrict__ vts;
    const float* __restrict__ mask;
    void* __restrict__ y;
    int64_t T, S, d, dv;
    int64_t mask_rows;                                          // T ([T, S] shared by the slices) or G T; read only with a mask
    float scale;
    int qk_format, p_format, v_format, ydt, causal, vec, y_vec, tiles;      // tiles: work-groups per slice
};

// the operand registers of one lane from its two 16-code pieces: what MxgLds<BITS>::put of both followed by ::get hands out
template <int BITS>
__device__ __forceinline__ i32x8 mxf_frag(u32x4 lo, u32x4 hi) {
    const u32x4 a = mxg_pack16<BITS>(lo), b = mxg_pack16<BITS>(hi);
    if constexpr (BITS == 8) return i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
    else if constexpr (BITS == 4) return i32x8{(int)a[0], (int)a[1], (int)b[0], (int)b[1], 0, 0, 0, 0};
    else return i32x8{(int)a[0], (int)a[1], (int)a[2], (int)b[0], (int)b[1], (int)b[2], 0, 0};
}

__device__ __forceinline__ u32x4 mxf_load16(const uint8_t* __restrict__ codes, bool in, int64_t off, int left, int vec) {
    return vec ? mx_load16<true>(codes, in, off, left) : mx_load16<false>(codes, in, off, left);
}

// the chunk of 128 rows from row0 and 128 codes from k0 of `codes` [rows, K] into the LDS tile: thread's pieces as mxg_stage takes them
template <int BITS>
__device__ __forceinline__ void mxf_stage(uint8_t* tile, const uint8_t* __restrict__ codes, int64_t rows, int64_t K, int64_t row0,
                                          int64_t k0, int tid, int vec) {
    u32x4 reg[4];
    const int64_t kk = k0 + (tid & 7) * 16;
    const int left = (int)(K - kk < 16 ? K - kk : 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + (tid >> 3) + 32 * i;
        reg[i] = mxf_load16(codes, row < rows && kk < K, row * K + kk, left, vec);
    }
    mxg_stage<BITS>(tile, reg, tid);
}

// phase 1 for the format FQ of q and k: s[f] = the scores of this wave's 16 queries (from row tq of the slice) against keys 16 f ..
template <int FQ, int NF>
__device__ __forceinline__ void mxf_scores(f32x4 (&s)[NF], const MxfArgs& a, const uint8_t* __restrict__ q, const uint8_t* __restrict__ qs,
                                           const uint8_t* __restrict__ k, const uint8_t* __restrict__ ks, int64_t tq, int64_t s_end,
                                           uint8_t* tile, int tid) {
    constexpr int BITS = mxg_bits(FQ);
    using L = MxgLds<BITS>;
    const int lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int64_t nkb = (a.d + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    const int64_t t = tq + i;
    const int64_t klo = BITS == 8 ? 16 * g : 32 * g, khi = BITS == 8 ? 64 + 16 * g : 32 * g + 16;
    const bool tin = t < a.T;
    const i32x8 fq = mxf_frag<BITS>(mxf_load16(q, tin && klo < a.d, t * a.d + klo, (int)(a.d - klo < 16 ? a.d - klo : 16), a.vec),
                                    mxf_load16(q, tin && khi < a.d, t * a.d + khi, (int)(a.d - khi < 16 ? a.d - khi : 16), a.vec));
    const int sq = (int)mx_scale(qs, tin && g < nkb, t * nkb + g);
#pragma unroll
    for (int c = 0; c < NF / 8; ++c) {
        if (c * 128 < s_end) {                                  // (uniform over the work-group: the barriers are)
            if (c) __syncthreads();                             // every wave is done with the chunk before
            mxf_stage<BITS>(tile, k, a.S, a.d, c * 128, 0, tid, a.vec);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int64_t key = c * 128 + 16 * j + i;
                if (c * 128 + 16 * j < s_end) {
                    const int sk = (int)mx_scale(ks, key < a.S && g < nkb, key * nkb + g);
                    s[8 * c + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(L::get(tile, 16 * j + i, g), fq,
                                                                                    f32x4{0.0f, 0.0f, 0.0f, 0.0f}, FQ, FQ, 0, sk, 0, sq);
                }
            }
        }
    }
}

// phase 3 for the formats FP of p and FV of vt: acc[j] = the wave's 16 queries against the rows 16 j .. of vt, over the whole of S.
// pc[f]: this lane's 4 codes of fragment f; sw[c]: the scale bytes of its query's blocks 4 c .. 4 c + 3
template <int FP, int FV, int NF>
__device__ __forceinline__ void mxf_pv(f32x4 (&acc)[8], const uint32_t (&pc)[NF], const uint32_t (&sw)[NF / 8],
                                       const uint8_t* __restrict__ vt, const uint8_t* __restrict__ vts, int64_t S, int64_t dv, uint8_t* lds,
                                       int tid, int vec) {
    constexpr int PB = mxg_bits(FP), VB = mxg_bits(FV);
    using LV = MxgLds<VB>;
    const int lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int64_t nsb = (S + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    uint8_t* bounce = lds + kMxfTile + wave * kMxfBounce;
    const int plo = PB == 8 ? 16 * g : 32 * g, phi = PB == 8 ? 64 + 16 * g : 32 * g + 16;
#pragma unroll
    for (int c = 0; c < NF / 8; ++c) {
        if (c * 128 < S) {                                      // (kernel-uniform)
            __syncthreads();                                    // every wave is done with what the tile and the bounce held
            mxf_stage<VB>(lds, vt, dv, S, 0, c * 128, tid, vec);
#pragma unroll
            for (int ff = 0; ff < 8; ++ff) *(uint32_t*)(bounce + i * kMxfBounceRow + 16 * ff + 4 * g) = pc[8 * c + ff];
            __syncthreads();
            const i32x8 fpv = mxf_frag<PB>(*(const u32x4*)(bounce + i * kMxfBounceRow + plo), *(const u32x4*)(bounce + i * kMxfBounceRow + phi));
            const int sp = (int)((sw[c] >> (8 * g)) & 0xffu);
            const int64_t kb = 4 * c + g;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (16 * j < dv) {                              // (kernel-uniform)
                    const int64_t n = 16 * j + i;
                    const int sv = (int)mx_scale(vts, n < dv && kb < nsb, n * nsb + kb);
                    acc[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(LV::get(lds, 16 * j + i, g), fpv, acc[j], FV, FP, 0, sv, 0, sp);
                }
            }
        }
    }
}

#define QS_MXF_FORMATS(X) X(QS_MX_FP8_E4M3) X(QS_MX_FP8_E5M2) X(QS_MX_FP6_E2M3) X(QS_MX_FP6_E3M2)

template <int FP, int NF, class... A>
__device__ __forceinline__ void mxf_pv_v(int v_format, A&&... args) {
    switch (v_format) {
#define X(F) case F: mxf_pv<FP, F, NF>(args...); break;
        QS_MXF_FORMATS(X)
#undef X
        default: mxf_pv<FP, QS_MX_FP4_E2M1, NF>(args...); break;
    }
}

template <int NF, class... A>
__device__ __forceinline__ void mxf_pv_p(int p_format, int v_format, A&&... args) {
    switch (p_format) {
#define X(F) case F: mxf_pv_v<F, NF>(v_format, args...); break;
        QS_MXF_FORMATS(X)
#undef X
        default: mxf_pv_v<QS_MX_FP4_E2M1, NF>(v_format, args...); break;
    }
}

template <int NF>
__global__ __launch_bounds__(kMxgThreads) void mx_flash_kernel(MxFormat fp, MxfArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kMxfTile + 4 * kMxfBounce];
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
    const int64_t t = t0 + 16 * wave + i;                       // this lane's query row

    // ---- phase 1 ---------------------------------------------------------------------------------------------------------------
    f32x4 s[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) s[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int64_t s_end = (a.causal && t0 + kMxfRows < S) ? t0 + kMxfRows : S;      // no row of the work-group admits a column at or behind it
    switch (a.qk_format) {                                      // (kernel-uniform)
        case QS_MX_FP8_E4M3: mxf_scores<QS_MX_FP8_E4M3, NF>(s, a, q, qs, k, ks, t0 + 16 * wave, s_end, lds, tid); break;
        case QS_MX_FP8_E5M2: mxf_scores<QS_MX_FP8_E5M2, NF>(s, a, q, qs, k, ks, t0 + 16 * wave, s_end, lds, tid); break;
        case QS_MX_FP6_E2M3: mxf_scores<QS_MX_FP6_E2M3, NF>(s, a, q, qs, k, ks, t0 + 16 * wave, s_end, lds, tid); break;
        case QS_MX_FP6_E3M2: mxf_scores<QS_MX_FP6_E3M2, NF>(s, a, q, qs, k, ks, t0 + 16 * wave, s_end, lds, tid); break;
        default: mxf_scores<QS_MX_FP4_E2M1, NF>(s, a, q, qs, k, ks, t0 + 16 * wave, s_end, lds, tid); break;
    }

    // ---- phase 2 ---------------------------------------------------------------------------------------------------------------
    const float ninf = __uint_as_float(0xff800000u);
    // a row past T admits nothing (and reads no mask): it is NaN as a whole and never stored
    const int64_t Lim = t >= T ? 0 : ((a.causal && t + 1 < S) ? t + 1 : S);
    const int64_t mbase = a.mask ? ((slice * T + (t < T ? t : 0)) % a.mask_rows) * S : 0;
    float m = ninf;
    bool bad = false;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        if (16 * f < S) {                                       // (wave-uniform)
            const int64_t c0 = 16 * f + 4 * g;
            float am[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (a.mask) {
                if (a.vec) {                                    // (S % 16 == 0: the four are inside the row together; L cuts anywhere)
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
                bad |= w != w;
                m = fmaxf(m, w);                                // (a NaN is skipped here and kept in `bad`)
            }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    int badi = (int)bad;
    badi |= __shfl_xor(badi, 16, 64);
    badi |= __shfl_xor(badi, 32, 64);
    const bool rownan = badi != 0 || mx_abs_bits(m) >= 0x7f800000u;

    float P[NF];                                                // partial sum 4 f + g of the definition's row sum
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        if (16 * f < S) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s[f][r] = msx_exp(s[f][r] - m);
            P[f] = 0.0f + ((s[f][0] + s[f][1]) + (s[f][2] + s[f][3]));
        } else {
            P[f] = 0.0f;
        }
    }
#pragma unroll
    for (int h = NF / 2; h >= 1; h >>= 1)
#pragma unroll
        for (int f = 0; f < h; ++f) P[f] = P[f] + P[f + h];
    float Z = P[0];
    Z = Z + __shfl_xor(Z, 32, 64);
    Z = Z + __shfl_xor(Z, 16, 64);

    uint32_t pc[NF], sw[NF / 8];                                // a fragment's 4 codes; the scale bytes of the query's blocks 4 j .. 4 j + 3
#pragma unroll
    for (int j = 0; j < NF / 8; ++j) sw[j] = 0x7f7f7f7fu;       // (127: what a block wholly past S takes)
#pragma unroll
    for (int b = 0; b < NF / 2; ++b) {
        pc[2 * b] = pc[2 * b + 1] = 0u;
        if (32 * b < S) {
            float p[2][4];
            uint32_t am = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool in = 32 * b + 16 * h + 4 * g + r < S;
                    // (a fragment wholly past S was never formed: its registers are not read)
                    const float e = 16 * (2 * b + h) < S ? s[2 * b + h][r] : 0.0f;
                    p[h][r] = in ? (rownan ? __uint_as_float(0x7fc00000u) : e / Z) : 0.0f;
                    const uint32_t ab = mx_abs_bits(p[h][r]);
                    am = ab > am ? ab : am;
                }
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)am, off, 64);
                am = o > am ? o : am;
            }
            const MxScale sc = mx_scale(am, fp);
            sw[b >> 2] = (sw[b >> 2] & ~(0xffu << (8 * (b & 3)))) | (sc.byte << (8 * (b & 3)));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint32_t w = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    uint32_t sg;
                    const float qv = mx_round_abs(p[h][r], sc, fp, sg);
                    w |= mx_code(qv, sg, sc, fp) << (8 * r);
                }
                pc[2 * b + h] = w;
            }
        }
    }

    // ---- phase 3 ---------------------------------------------------------------------------------------------------------------
    f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    mxf_pv_p<NF>(a.p_format, a.v_format, acc, pc, sw, vt, vts, S, dv, lds, tid, a.vec);       // (kernel-uniform switches)

    // ---- epilogue: lane 16 g + i holds the columns 16 j + 4 g + {0..3} of row t ------------------------------------------------------
    if (t >= T) return;
    void* y = (uint8_t*)a.y + slice * T * dv * (a.ydt == QS_F32 ? 4 : 2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t n = 16 * j + 4 * g;
        if (n >= dv) continue;
        const float v[4] = {acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
        mx_store4(y, a.ydt, t * dv + n, v, n, dv, a.y_vec);
    }
}

}  // namespace qs
