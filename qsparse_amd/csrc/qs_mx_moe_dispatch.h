// The two permutations around the expert products of a mixture-of-experts layer (include/qsparse_hip.h, "MX MoE dispatch" and "MX MoE
// combine"), both driven by inv [T, k] of the routing: row inv[t, j] of the expert-sorted buffer belongs to slot j of token t.
//
//   mx_moe_dispatch_kernel        read once, write k times.  One WAVE per token: the lane's 8 elements of the row are loaded and widened
//     once per pass of 512 (one 16-byte load for two-byte inputs, two for float32), a block of 32 is 4 adjacent lanes (two __shfl_xor
//     steps for its maximum), scale and codes come from qs_mx.h's mx_scale / mx_round_abs / mx_code -- the quantizer's own functions, so
//     the bytes are mx_inner_vec_kernel's.  The token's k destinations are loaded once (lane j holds inv[t, j]) and broadcast one by one:
//     a wave-uniform row index, one 8-byte code store per lane and one scale byte per block for each.  No float copy of the row exists.
//     VEC = false: one element per lane and pass of 64, a block is half a wave, every access predicated on its own index.
//   mx_moe_dispatch_copy_kernel   the same for an input that is MX bytes already: the codes and scale bytes of a row copied to its k rows.
//   mx_moe_combine_kernel         out[t] = ((g_0 y_0) + (g_1 y_1)) + ... with y_j = y[inv[t, j]]: one wave per token, one thread per 4
//     columns and pass of 256, the k row indices and gates broadcast from the lanes that loaded them; every product and sum a float32
//     instruction of its own (the build forms no FMA), one rounding to the output dtype.  No atomics: a token's k rows meet in registers.
// An inv entry outside [0, T k) is never dereferenced: dispatch stores nothing for it, combine takes its row as +0.
#pragma once
#include "qs_mx.h"

namespace qs {

constexpr int kMoeDThreads = 256;
constexpr int kMoeDTokens = kMoeDThreads / 64;                  // tokens per work-group: one per wave

struct MoeDispatchArgs {
    const void* x;               // [T, D] rows `stride` elements apart, or
    const uint8_t* xc;           // codes [T, D] and
    const uint8_t* xs;           // scales [T, nb] of an input that is MX bytes
    const int32_t* inv;
    uint8_t* codes;
    uint8_t* scales;
    int64_t stride, rows;        // rows = T k
    int T, D, k, nb;
};

template <int XDT, bool VEC>
__global__ __launch_bounds__(kMoeDThreads) void mx_moe_dispatch_kernel(MxFormat f, MoeDispatchArgs a) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * kMoeDTokens + (threadIdx.x >> 6);
    if (t >= a.T) return;                                       // (wave-uniform; no work-group barrier below)
    const int dst = lane < a.k ? a.inv[(int64_t)t * a.k + lane] : -1;
    const int64_t xrow = (int64_t)t * a.stride;
    if constexpr (VEC) {                                        // D % 8 == 0, stride % 8 == 0, 16-byte x, 8-byte codes
        for (int c0 = 0; c0 < a.D; c0 += 512) {
            const int c = c0 + lane * 8;
            const bool in = c < a.D;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.0f;
            if (in) unpack8<XDT>(load8_raw<XDT, false>(a.x, (xrow + c) >> 3), v);
            uint32_t am = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t b = mx_abs_bits(v[j]);
                am = b > am ? b : am;
            }
#pragma unroll
            for (int off = 1; off < 4; off <<= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)am, off, 64);
                am = o > am ? o : am;
            }
            const MxScale s = mx_scale(am, f);
            uint32_t q[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint32_t sg;
                const float r = mx_round_abs(v[j], s, f, sg);
                q[j] = mx_code(r, sg, s, f);
            }
            const u32x2 w = {q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24), q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24)};
            for (int j = 0; j < a.k; ++j) {
                const int d = __shfl(dst, j, 64);
                if ((uint64_t)(int64_t)d < (uint64_t)a.rows && in) {
                    *(u32x2*)(a.codes + (int64_t)d * a.D + c) = w;
                    if ((lane & 3) == 0) a.scales[(int64_t)d * a.nb + (c >> 5)] = (uint8_t)s.byte;
                }
            }
        }
    } else {
        for (int c0 = 0; c0 < a.D; c0 += 64) {
            const int c = c0 + lane;
            const bool in = c < a.D;
            const float v = in ? load1<XDT>(a.x, xrow + c) : 0.0f;
            uint32_t am = mx_abs_bits(v);
#pragma unroll
            for (int off = 1; off < 32; off <<= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)am, off, 64);
                am = o > am ? o : am;
            }
            const MxScale s = mx_scale(am, f);
            uint32_t sg;
            const float r = mx_round_abs(v, s, f, sg);
            const uint32_t q = mx_code(r, sg, s, f);
            for (int j = 0; j < a.k; ++j) {
                const int d = __shfl(dst, j, 64);
                if ((uint64_t)(int64_t)d < (uint64_t)a.rows && in) {
                    a.codes[(int64_t)d * a.D + c] = (uint8_t)q;
                    if ((lane & 31) == 0) a.scales[(int64_t)d * a.nb + (c >> 5)] = (uint8_t)s.byte;
                }
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kMoeDThreads) void mx_moe_dispatch_copy_kernel(MoeDispatchArgs a) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * kMoeDTokens + (threadIdx.x >> 6);
    if (t >= a.T) return;
    const int dst = lane < a.k ? a.inv[(int64_t)t * a.k + lane] : -1;
    constexpr int W = VEC ? 16 : 1;                             // VEC: D % 16 == 0, 16-byte xc and codes
    for (int c0 = 0; c0 < a.D; c0 += 64 * W) {
        const int c = c0 + lane * W;
        const bool in = c < a.D;
        u32x4 w = {0u, 0u, 0u, 0u};
        if (in) {
            if constexpr (VEC) w = *(const u32x4*)(a.xc + (int64_t)t * a.D + c);
            else w[0] = a.xc[(int64_t)t * a.D + c];
        }
        for (int j = 0; j < a.k; ++j) {
            const int d = __shfl(dst, j, 64);
            if ((uint64_t)(int64_t)d < (uint64_t)a.rows && in) {
                if constexpr (VEC) *(u32x4*)(a.codes + (int64_t)d * a.D + c) = w;
                else a.codes[(int64_t)d * a.D + c] = (uint8_t)w[0];
            }
        }
    }
    for (int b0 = 0; b0 < a.nb; b0 += 64) {
        const int b = b0 + lane;
        const bool in = b < a.nb;
        const uint8_t byte = in ? a.xs[(int64_t)t * a.nb + b] : (uint8_t)0;
        for (int j = 0; j < a.k; ++j) {
            const int d = __shfl(dst, j, 64);
            if ((uint64_t)(int64_t)d < (uint64_t)a.rows && in) a.scales[(int64_t)d * a.nb + b] = byte;
        }
    }
}

struct MoeCombineArgs {
    const void* y;               // [T k, D] dense
    const int32_t* inv;
    const float* gates;
    void* out;                   // [T, D] dense
    int64_t rows;
    int T, D, k, odt;
};

// 4 consecutive elements of a dense tensor from element index i (VEC: i % 4 == 0 and all four inside; else each predicated on n)
template <int DT, bool VEC>
__device__ __forceinline__ void moe_load4(const void* p, int64_t i, int n, float (&v)[4]) {
    if constexpr (VEC) {
        if constexpr (DT == QS_F32) {
            const u32x4 w = *((const u32x4*)p + (i >> 2));
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = __uint_as_float(w[q]);
        } else {
            const u32x2 w = *((const u32x2*)p + (i >> 2));
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                v[2 * q] = DT == QS_BF16 ? __uint_as_float(w[q] << 16) : f16_bits_to_f32(w[q] & 0xffffu);
                v[2 * q + 1] = DT == QS_BF16 ? __uint_as_float(w[q] & 0xffff0000u) : f16_bits_to_f32(w[q] >> 16);
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = q < n ? load1<DT>(p, i + q) : 0.0f;
    }
}

template <int DT, bool VEC>
__device__ __forceinline__ void moe_store4(void* p, int64_t i, int n, const float (&v)[4]) {
    if constexpr (VEC) {
        if constexpr (DT == QS_F32) {
            *((u32x4*)p + (i >> 2)) = u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
        } else {
            uint32_t h[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) h[q] = DT == QS_BF16 ? f32_to_bf16_bits(v[q]) : f32_to_f16_bits(v[q]);
            *((u32x2*)p + (i >> 2)) = u32x2{h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < n) store1<DT>(p, i + q, v[q]);
    }
}

template <int YDT, bool VEC>
__global__ __launch_bounds__(kMoeDThreads) void mx_moe_combine_kernel(MoeCombineArgs a) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * kMoeDTokens + (threadIdx.x >> 6);
    if (t >= a.T) return;                                       // (wave-uniform)
    const int dst = lane < a.k ? a.inv[(int64_t)t * a.k + lane] : -1;
    const float gate = lane < a.k ? a.gates[(int64_t)t * a.k + lane] : 0.0f;
    for (int c0 = 0; c0 < a.D; c0 += 256) {
        const int c = c0 + lane * 4, n = a.D - c;               // n <= 0: the lane is past the row
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < a.k; ++j) {
            const int d = __shfl(dst, j, 64);
            const float g = __shfl(gate, j, 64);
            float yv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if ((uint64_t)(int64_t)d < (uint64_t)a.rows && n > 0) moe_load4<YDT, VEC>(a.y, (int64_t)d * a.D + c, n, yv);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float p = g * yv[q];
                acc[q] = j == 0 ? p : acc[q] + p;
            }
        }
        if (n > 0) {
            const int64_t o = (int64_t)t * a.D + c;
            if (a.odt == QS_F32) moe_store4<QS_F32, VEC>(a.out, o, n, acc);
            else if (a.odt == QS_BF16) moe_store4<QS_BF16, VEC>(a.out, o, n, acc);
            else moe_store4<QS_F16, VEC>(a.out, o, n, acc);
        }
    }
}

}  // namespace qs
