// Scale, mask, softmax and the MX quantizer in ONE launch (include/qsparse_hip.h, "MX softmax quantizer"): s [G, T, S] leaves as the
// row pair of p = softmax(s * scale (+ mask)) over S; neither u = s * scale + mask, nor e, nor the float p ever exists in memory.
//
//   mx_softmax_quant_kernel   one WAVE per row (four rows per work-group, no LDS, no barrier -- as mx_norm_stats_kernel).  A lane takes
//     8 consecutive elements per pass of 512 (one 16-byte load for two-byte inputs, two for float32, and two for the mask, on the VEC
//     route).  The wave walks the row three times:
//       1. u_j and the maximum m: a lane maximum, six __shfl_xor steps; a NaN is noted beside it (one ballot);
//       2. e_j = E(u_j - m) and Z: the lane's two quad sums go to its two partial sums, the 128 partial sums are folded by
//          mxn_add_quads / mxn_fold of qs_mx_norm.h -- the header's row sum, a function of S alone;
//       3. p_j = e_j / Z, the block maximum (a block of 32 is 4 adjacent lanes: two __shfl_xor steps), qs_mx.h's scale and encode,
//          one scale byte per block and the lane's 8 codes (one 8-byte store on the VEC route).
//     RES (S <= kMsxResPasses * 512 = 1024): all three walks run on the lane's registers -- 16 floats -- and s and the mask are read from
//     memory once, every load issued before the first use.  Longer rows form u again from memory for walks 2 and 3 (served from the
//     cache, as layer mode's second walk of the norm statistics); E(u_j - m) is then evaluated twice, to the same bits.
//   A causal row loads nothing at or behind its limit L = min(t + 1, S): those u_j are -inf by construction.
// Every operation of the definition is a float32 operation of its own: the build compiles with -ffp-contract=off (no FMA is formed),
// `/` is the correctly rounded division (the build's default for HIP), rintf is v_rndne_f32, and 2^n is assembled from its exponent
// field -- no exp / exp2 / ldexp of a library, no approximate reciprocal.
// VEC = false is the same text with element accesses, each predicated on its own index: any T, S >= 1, any element-aligned base.
#pragma once
#include "qs_mx_norm.h"

namespace qs {

constexpr int kMsxRows = kMxq2Threads / 64;                     // rows per work-group: one per wave
constexpr int kMsxResPasses = 2;                                // passes of 512 a wave keeps in registers: S <= 1024 is read once
constexpr int kMsxLpb = QS_MX_BLOCK / 8;                        // 4 lanes per block of 32

// E(t) of the header for t <= 0 (or NaN: a row that is NaN as a whole, whose e is never used): Cody-Waite reduction by
// ln 2 = 0.693359375 - 2.12194440e-4, a degree-7 Horner polynomial, an exact scaling by 2^n.  t >= -87 gives n in [-126, 0] and, at
// n = -126, P > 1: the product is a normal number and exact.
__device__ __forceinline__ float msx_exp(float t) {
    const bool live = t >= -87.0f;                              // (false for -inf and for a NaN)
    const float tc = live ? t : -87.0f;
    const float n = rintf(tc * 1.44269504f);                    // ties to even
    const float r = (tc - n * 0.693359375f) - n * -2.12194440e-4f;
    float P = (float)(1.0 / 5040.0);
    P = P * r + (float)(1.0 / 720.0);
    P = P * r + (float)(1.0 / 120.0);
    P = P * r + (float)(1.0 / 24.0);
    P = P * r + (float)(1.0 / 6.0);
    P = P * r + 0.5f;
    P = P * r + 1.0f;
    P = P * r + 1.0f;
    const float two_n = __uint_as_float((uint32_t)((int)n + 127) << 23);
    return live ? P * two_n : 0.0f;
}

// u of the 8 elements [c, c + 8) of the row of s at `sbase` (of mask at `mbase`): s_j * scale (+ a_j) below the limit L <= S, -inf at
// and behind it -- nothing there is loaded
template <int XDT, bool VEC>
__device__ __forceinline__ void msx_load_u(const void* __restrict__ s, const float* __restrict__ mask, int64_t sbase, int64_t mbase,
                                           int64_t c, int64_t L, float scale, float (&u)[8]) {
    float v[8], a[8];
    if constexpr (VEC) {                                        // (S % 8 == 0: the 8 are inside the row together; L cuts anywhere)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = a[j] = 0.0f;
        if (c < L) {
            unpack8<XDT>(load8_raw<XDT, false>(s, (sbase + c) >> 3), v);
            if (mask) unpack8<QS_F32>(load8_raw<QS_F32, false>(mask, (mbase + c) >> 3), a);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = c + j < L;
            v[j] = in ? load1<XDT>(s, sbase + c + j) : 0.0f;
            a[j] = (mask && in) ? mask[mbase + c + j] : 0.0f;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float w = v[j] * scale;
        if (mask) w = w + a[j];                                 // (kernel-uniform; an absent mask is not added)
        u[j] = c + j < L ? w : __uint_as_float(0xff800000u);
    }
}

// `mask_rows`: T for a mask [T, S] shared by the slices, R = G T for one [G, T, S] (read only with a mask)
template <int XDT, bool VEC, bool RES>
__global__ __launch_bounds__(kMxq2Threads) void mx_softmax_quant_kernel(MxFormat f, const void* __restrict__ s,
                                                                        const float* __restrict__ mask, uint8_t* __restrict__ codes,
                                                                        uint8_t* __restrict__ scales, int64_t R, int64_t T, int64_t S,
                                                                        int64_t mask_rows, float scale, int causal) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kMsxRows + (threadIdx.x >> 6);
    if (r >= R) return;                                         // (wave-uniform; the kernel has no barrier)
    const int64_t t = r % T;
    const int64_t L = (causal && t + 1 < S) ? t + 1 : S;        // top-left aligned
    const int64_t sbase = r * S, mbase = (r % mask_rows) * S, nb = (S + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    auto load = [&](int64_t c, float (&u)[8]) { msx_load_u<XDT, VEC>(s, mask, sbase, mbase, c, L, scale, u); };

    constexpr int NU = RES ? kMsxResPasses : 1;
    float u[NU][8];

    // ---- walk 1: u and its maximum ---------------------------------------------------------------------------------------------
    float m = __uint_as_float(0xff800000u);
    bool bad = false;
    auto scan = [&](const float (&v)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            bad |= v[j] != v[j];
            m = fmaxf(m, v[j]);                                 // (a NaN is skipped here and kept in `bad`)
        }
    };
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < NU; ++k)
            if (k * kMxnPass < S) load(k * kMxnPass + lane * 8, u[k]);        // (wave-uniform, as every pass condition below)
#pragma unroll
        for (int k = 0; k < NU; ++k)
            if (k * kMxnPass < S) scan(u[k]);
    } else {
        for (int64_t c0 = 0; c0 < S; c0 += kMxnPass) {
            load(c0 + lane * 8, u[0]);
            scan(u[0]);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    // a NaN in the row, m = +inf, m = -inf (nothing admitted): the row is NaN as a whole
    const bool rownan = __any((int)bad) || mx_abs_bits(m) >= 0x7f800000u;

    // ---- walk 2: e and Z ---------------------------------------------------------------------------------------------------------
    float pa = 0.0f, pb = 0.0f;                                 // the partial sums 2 lane and 2 lane + 1
    auto to_e = [&](float (&v)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = msx_exp(v[j] - m);
    };
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < NU; ++k)
            if (k * kMxnPass < S) {
                to_e(u[k]);
                mxn_add_quads(u[k], pa, pb);
            }
    } else {
        for (int64_t c0 = 0; c0 < S; c0 += kMxnPass) {
            load(c0 + lane * 8, u[0]);
            to_e(u[0]);
            mxn_add_quads(u[0], pa, pb);
        }
    }
    const float Z = mxn_fold(pa, pb);

    // ---- walk 3: p, its blocks' scales, the codes ----------------------------------------------------------------------------------
    auto emit = [&](int64_t c, const float (&e)[8]) {
        float p[8];
        uint32_t am = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            p[j] = c + j < S ? (rownan ? __uint_as_float(0x7fc00000u) : e[j] / Z) : 0.0f;
            const uint32_t a = mx_abs_bits(p[j]);
            am = a > am ? a : am;
        }
        const MxScale sc = mx_scale(mxq2_block_max<kMsxLpb>(am), f);
        uint32_t cd[8];
        mx_encode_run<8, false, false>(p, sc, f, MxSrKey{0u, 0u}, 0u, 0ull, cd);
        if (c < S) {
            if ((lane % kMsxLpb) == 0) scales[r * nb + (c >> 5)] = (uint8_t)sc.byte;
            mxq2_store_row<8, false>(codes + sbase + c, cd, VEC, c, S);
        }
    };
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < NU; ++k)
            if (k * kMxnPass < S) emit(k * kMxnPass + lane * 8, u[k]);
    } else {
        for (int64_t c0 = 0; c0 < S; c0 += kMxnPass) {
            load(c0 + lane * 8, u[0]);
            to_e(u[0]);
            emit(c0 + lane * 8, u[0]);
        }
    }
}

}  // namespace qs
