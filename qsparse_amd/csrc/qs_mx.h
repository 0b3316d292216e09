// MX block-scaled quantizer kernels (OCP Microscaling Formats v1.0; include/qsparse_hip.h, "MX block-scaled quantizer").
//
// One block = 32 consecutive elements along one axis sharing a power-of-two scale X = 2^e.  Everything is float32 bit and
// exponent arithmetic, no division, no transcendental:
//   e      from the exponent field of the block's abs-max (integer maximum of |x| bit patterns: a NaN sorts above Inf above every
//          finite value, so a non-finite block is recognised from the maximum alone)
//   x / X  a multiplication by 2^-e (exact: |x / X| < 2^(emax + 1), and what underflows lies far below half the format's smallest
//          subnormal)
//   RNE onto the format's grid: (|v| + C) - C with C = 2^(max(exponent(v), 1 - bias) + 23 - mbits) -- the float32 addition rounds
//          to nearest-even at exactly the grid's spacing in v's binade (the format's subnormal spacing below its smallest normal)
//          and the subtraction is exact -- then the clamp to the largest normal
//   q * X  a multiplication by 2^e (2^-127 is the float32 subnormal 0x00400000), exact
// The element format is a RUN-TIME descriptor (wave-uniform scalars: shift counts, two constants), so the kernels are templated on
// the input dtype alone: 3 kernels x 3 dtypes for the five formats.  Output dtype and `codes != nullptr` branch wave-uniformly.
//
// Stochastic rounding (include/qsparse_hip.h, "Stochastic rounding of the MX quantizers") replaces the RNE step alone, by
// mx_round_abs_sr: the 32-bit word of code j of an output tensor is word j & 3 of Philox4x32-10 (qs_philox.h) at counter
// (j >> 2, stream), key = seed + *step -- `step` is read from device memory by the kernel, so a captured launch draws fresh words on
// every replay.  The mode is the template parameter SR of every kernel: the SR = false instantiations are the kernels as they were.
#pragma once
#include "qs_common.h"
#include "qs_philox.h"

namespace qs {

struct MxFormat {
    int32_t emax;            // exponent of the largest normal
    int32_t mbits;           // mantissa bits
    int32_t min_exp_biased;  // float32-biased exponent of the format's smallest normal: (1 - bias) + 127
    uint32_t code_bias;      // (127 - bias) << mbits: float32 exponent|mantissa prefix -> the format's
    uint32_t sign_shift;     // 31 - (ebits + mbits): float32 sign bit -> the code's
    float max_normal;
    float sub_scale;         // 2^(bias - 1 + mbits): a subnormal value -> its mantissa
};

struct MxScale {
    float inv, X;            // 2^-e, 2^e
    uint32_t byte;           // E8M0: e + 127, 0xFF for a non-finite block
    bool nan;
};

// ---- host side: the descriptor of an enum qs_mx_format (shared by every unit that launches an MX quantizer kernel) ----------
// ebits, mbits, bias, emax, largest normal
struct MxSpec {
    int ebits, mbits, bias, emax;
    float max_normal;
};
constexpr MxSpec kMxSpecs[5] = {
    {4, 3, 7, 8, 448.0f},       // QS_MX_FP8_E4M3
    {5, 2, 15, 15, 57344.0f},   // QS_MX_FP8_E5M2
    {2, 3, 1, 2, 7.5f},         // QS_MX_FP6_E2M3
    {3, 2, 3, 4, 28.0f},        // QS_MX_FP6_E3M2
    {2, 1, 1, 2, 6.0f},         // QS_MX_FP4_E2M1
};

inline MxFormat mx_format(int format) {
    const MxSpec& sp = kMxSpecs[format];
    MxFormat f;
    f.emax = sp.emax;
    f.mbits = sp.mbits;
    f.min_exp_biased = 1 - sp.bias + 127;
    f.code_bias = (uint32_t)(127 - sp.bias) << sp.mbits;
    f.sign_shift = 31u - (uint32_t)(sp.ebits + sp.mbits);
    f.max_normal = sp.max_normal;
    f.sub_scale = (float)(1 << (sp.bias - 1 + sp.mbits));
    return f;
}

// the stochastic operands of a descriptor (host side): QS_ERR_ARG for an unknown mode or -- in either mode -- a `step` pointer off
// its 8-byte alignment or an index_base that is no multiple of 4
inline int mx_sr_check(int rounding, const int64_t* step, uint64_t index_base) {
    if (rounding != QS_MX_ROUND_NEAREST && rounding != QS_MX_ROUND_STOCHASTIC) return QS_ERR_ARG;
    if ((((uintptr_t)step) & 7u) != 0 || (index_base & 3u) != 0) return QS_ERR_ARG;
    return 0;
}

__device__ __forceinline__ uint32_t mx_abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// `am`: the maximum of the block's |x| bit patterns
__device__ __forceinline__ MxScale mx_scale(uint32_t am, const MxFormat& f) {
    MxScale s;
    s.nan = am >= 0x7f800000u;
    int eb = (int)(am >> 23) - f.emax;          // e + 127; a float32 subnormal or zero abs-max lands below 0: the clamp at -127
    eb = eb < 0 ? 0 : eb;                       // (the upper clamp cannot bind: eb <= 254 - emax)
    s.byte = s.nan ? 0xffu : (uint32_t)eb;
    s.X = __uint_as_float(eb ? ((uint32_t)eb << 23) : 0x00400000u);
    s.inv = __uint_as_float((uint32_t)(254 - eb) << 23);
    return s;
}

// |q| (on the grid, clamped) of one element and its sign bit; the caller forms y and the code
__device__ __forceinline__ float mx_round_abs(float x, const MxScale& s, const MxFormat& f, uint32_t& sign) {
    const uint32_t vb = __float_as_uint(x * s.inv);
    sign = vb & 0x80000000u;
    const uint32_t ab = vb & 0x7fffffffu;
    int ex = (int)(ab >> 23);
    ex = ex < f.min_exp_biased ? f.min_exp_biased : ex;
    const float C = __uint_as_float((uint32_t)(ex + 23 - f.mbits) << 23);
    const float r = (__uint_as_float(ab) + C) - C;
    return r > f.max_normal ? f.max_normal : r;
}

// ---- stochastic rounding ---------------------------------------------------------------------------------------------------
// what a launch carries (kernel argument); `step` is nullable (= 0) and only ever read
struct MxSr {
    uint64_t seed;
    const int64_t* step;
    uint64_t base;           // index_base, a multiple of 4
    uint32_t stream;         // third counter word: 0 one-way / row pair, 1 col pair (the two-way kernel sets it per phase)
};

struct MxSrKey {
    uint32_t k0, k1;
};

__device__ __forceinline__ MxSrKey mx_sr_key(const MxSr& sr) {
    const uint64_t k = sr.seed + (sr.step ? (uint64_t)*sr.step : 0ull);        // (wave-uniform load)
    return MxSrKey{(uint32_t)k, (uint32_t)(k >> 32)};
}

// the words of the four codes j .. j + 3, j % 4 == 0
__device__ __forceinline__ void mx_sr_words4(const MxSrKey& k, uint32_t stream, uint64_t j, uint32_t (&w)[4]) {
    const uint64_t q = j >> 2;
    const uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), stream, 0u};
    philox4x32_10(c, k.k0, k.k1, w);
}

// the word of code j, any j (one call per element: the routes that are correct, not tuned)
__device__ __forceinline__ uint32_t mx_sr_word(const MxSrKey& k, uint32_t stream, uint64_t j) {
    uint32_t w[4];
    mx_sr_words4(k, stream, j & ~3ull, w);
    const uint32_t i = (uint32_t)j & 3u;
    return i == 0 ? w[0] : i == 1 ? w[1] : i == 2 ? w[2] : w[3];
}

// mx_round_abs with the rounding step drawn from the word `w`: |v| = m 2^(E - 150) lies n = floor(m / 2^sh) grid steps of
// 2^(ex - 127 - mbits) above zero plus a remainder; T holds m / 2^sh with 32 fractional bits, so (T + w) >> 32 adds one step with
// probability remainder / step.  sh >= 20 always; with sh > 56 the value is below 2^-32 of a step and stays where it is (zero).
__device__ __forceinline__ float mx_round_abs_sr(float x, const MxScale& s, const MxFormat& f, uint32_t w, uint32_t& sign) {
    const uint32_t vb = __float_as_uint(x * s.inv);
    sign = vb & 0x80000000u;
    const uint32_t ab = vb & 0x7fffffffu;
    const uint32_t field = ab >> 23;
    const int E = field ? (int)field : 1;
    const uint32_t m = (ab & 0x7fffffu) | (field ? 0x800000u : 0u);
    const int ex = E < f.min_exp_biased ? f.min_exp_biased : E;
    const int sh = (23 - f.mbits) + (ex - E);
    const uint64_t T = sh <= 56 ? (((uint64_t)m << 32) >> sh) : 0ull;
    const uint32_t n = (uint32_t)((T + w) >> 32);                               // <= 2^(mbits + 1): exact as a float32
    const float r = (float)n * __uint_as_float((uint32_t)(ex - f.mbits) << 23); // n 2^(ex - 127 - mbits), exact
    return r > f.max_normal ? f.max_normal : r;
}

__device__ __forceinline__ float mx_value(float r, uint32_t sign, const MxScale& s) {
    return s.nan ? __uint_as_float(0x7fc00000u) : __uint_as_float(__float_as_uint(r * s.X) | sign);
}

__device__ __forceinline__ uint32_t mx_code(float r, uint32_t sign, const MxScale& s, const MxFormat& f) {
    const uint32_t rb = __float_as_uint(r);
    const uint32_t mag = (int)(rb >> 23) < f.min_exp_biased ? (uint32_t)(r * f.sub_scale) : (rb >> (23 - f.mbits)) - f.code_bias;
    return s.nan ? 0u : (mag | (sign >> f.sign_shift));
}

// ------------------------------------------------------------------------------------------------
// Innermost axis, aligned: n % 32 == 0 and 16-byte aligned bases, so blocks are aligned in flat memory.  One 16-byte load per
// lane (8 two-byte or 4 float32 elements): a block is 4 / 8 adjacent lanes, its maximum two / three __shfl_xor steps.  A wave owns
// 64 * V consecutive elements.  float32 results of two-byte inputs are transposed through a wave-private LDS region so that each
// store instruction of the wave covers one contiguous 1 KiB span (as ew_widen_kernel, qs_elementwise.h); the other
// combinations store what the lane holds, 16 bytes per lane.
// ------------------------------------------------------------------------------------------------
constexpr int kMxBlock = 256;

template <int XDT, bool SR>
__global__ __launch_bounds__(kMxBlock) void mx_inner_vec_kernel(MxFormat f, const void* __restrict__ x, void* __restrict__ y,
                                                                uint8_t* __restrict__ codes, uint8_t* __restrict__ scales,
                                                                int64_t numel, int ydt, MxSr sr) {
    constexpr int V = XDT == QS_F32 ? 4 : 8;      // elements per lane
    constexpr int LPB = QS_MX_BLOCK / V;          // lanes per block
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e_wave = ((int64_t)blockIdx.x * (kMxBlock / 64) + wave) * (64 * V);
    const int64_t e = e_wave + lane * V;
    const bool in = e < numel;                    // (numel % 32 == 0: the lanes of a block are inside or outside together)
    float v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = 0.0f;
    if (in) {
        if constexpr (XDT == QS_F32) {
            const u32x4 a = ld16<true>((const u32x4*)x + (e >> 2));
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(a[j]);
        } else {
            float w[8];
            unpack8<XDT>(load8_raw<XDT, true>(x, e >> 3), w);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = w[j];
        }
    }
    uint32_t am = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const uint32_t a = mx_abs_bits(v[j]);
        am = a > am ? a : am;
    }
#pragma unroll
    for (int off = 1; off < LPB; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)am, off, 64);
        am = o > am ? o : am;
    }
    const MxScale s = mx_scale(am, f);
    float r[V];
    uint32_t sg[V];
    if constexpr (SR) {                           // e % V == 0 and sr.base % 4 == 0: one Philox call per 4 of the lane's codes
        const MxSrKey key = mx_sr_key(sr);
#pragma unroll
        for (int q = 0; q < V; q += 4) {
            uint32_t w[4];
            mx_sr_words4(key, sr.stream, sr.base + (uint64_t)e + q, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) r[q + j] = mx_round_abs_sr(v[q + j], s, f, w[j], sg[q + j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = mx_round_abs(v[j], s, f, sg[j]);
    }
    if (scales && in && (lane & (LPB - 1)) == 0) scales[e >> 5] = (uint8_t)s.byte;
    if (codes && in) {
        uint32_t c[V];
#pragma unroll
        for (int j = 0; j < V; ++j) c[j] = mx_code(r[j], sg[j], s, f);
        const uint32_t lo = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
        if constexpr (V == 8) {
            const uint32_t hi = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
            *(u32x2*)(codes + e) = u32x2{lo, hi};
        } else {
            *(uint32_t*)(codes + e) = lo;
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = mx_value(r[j], sg[j], s);
    if constexpr (XDT == QS_F32) {
        if (in) st16<true>((u32x4*)y + (e >> 2), u32x4{__float_as_uint(r[0]), __float_as_uint(r[1]), __float_as_uint(r[2]), __float_as_uint(r[3])});
    } else {
        __shared__ __attribute__((aligned(16))) float stage[kMxBlock * 8];
        if (ydt == QS_F32) {
            float* yf = (float*)y;
            if (e_wave + 512 <= numel) {          // wave-uniform: the whole wave inside the tensor
                float* ws = stage + wave * 512;
                *(u32x4*)(ws + lane * 8) = u32x4{__float_as_uint(r[0]), __float_as_uint(r[1]), __float_as_uint(r[2]), __float_as_uint(r[3])};
                *(u32x4*)(ws + lane * 8 + 4) = u32x4{__float_as_uint(r[4]), __float_as_uint(r[5]), __float_as_uint(r[6]), __float_as_uint(r[7])};
                __builtin_amdgcn_wave_barrier();
                const u32x4 o0 = *(const u32x4*)(ws + lane * 4);
                const u32x4 o1 = *(const u32x4*)(ws + 256 + lane * 4);
                st16<true>((u32x4*)(yf + e_wave + lane * 4), o0);
                st16<true>((u32x4*)(yf + e_wave + 256 + lane * 4), o1);
            } else if (in) {
                float w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j] = r[j];
                store8<QS_F32, true>(y, e >> 3, w);
            }
        } else if (in) {
            float w[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = r[j];
            store8<XDT, true>(y, e >> 3, w);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Innermost axis, any line length and any element-aligned base: one element per lane, a block is half a wave (five __shfl_xor
// steps), every access coalesced.  `nb` = ceil(n / 32) blocks per line; lanes past the end of a line load nothing and store nothing.
// ------------------------------------------------------------------------------------------------
template <int XDT, bool SR>
__global__ __launch_bounds__(kMxBlock) void mx_inner_plain_kernel(MxFormat f, const void* __restrict__ x, void* __restrict__ y,
                                                                  uint8_t* __restrict__ codes, uint8_t* __restrict__ scales,
                                                                  int64_t nblocks, int64_t n, int64_t nb, int ydt, MxSr sr) {
    const int64_t b = ((int64_t)blockIdx.x * kMxBlock + threadIdx.x) >> 5;       // block index = line * nb + kb
    const int sub = threadIdx.x & 31;
    const bool okb = b < nblocks;
    const int64_t line = okb ? b / nb : 0;
    const int64_t k = (b - line * nb) * QS_MX_BLOCK + sub;
    const bool in = okb && k < n;
    const int64_t e = line * n + k;
    const float v = in ? load1<XDT>(x, e) : 0.0f;
    uint32_t am = mx_abs_bits(v);
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)am, off, 64);
        am = o > am ? o : am;
    }
    const MxScale s = mx_scale(am, f);
    uint32_t sg;
    float r;
    if constexpr (SR) r = mx_round_abs_sr(v, s, f, mx_sr_word(mx_sr_key(sr), sr.stream, sr.base + (uint64_t)e), sg);
    else r = mx_round_abs(v, s, f, sg);
    if (scales && okb && sub == 0) scales[b] = (uint8_t)s.byte;
    if (!in) return;
    if (codes) codes[e] = (uint8_t)mx_code(r, sg, s, f);
    const float out = mx_value(r, sg, s);
    if (ydt == QS_F32) store1<QS_F32>(y, e, out);
    else store1<XDT>(y, e, out);
}

// ------------------------------------------------------------------------------------------------
// Strided axis: the tensor is [outer, n, inner] with inner > 1 and blocks along n.  Lanes run along `inner` (stride 1), so every
// load and store of a wave is coalesced; a thread walks the <= 32 elements of its block at stride `inner` and keeps them in
// registers.  Thread t = (o * nb + kb) * inner + i, which is also the index of its scale byte.
// ------------------------------------------------------------------------------------------------
template <int XDT, bool SR>
__global__ __launch_bounds__(kMxBlock) void mx_strided_kernel(MxFormat f, const void* __restrict__ x, void* __restrict__ y,
                                                              uint8_t* __restrict__ codes, uint8_t* __restrict__ scales,
                                                              int64_t total, int64_t n, int64_t inner, int64_t nb, int ydt, MxSr sr) {
    const int64_t t = (int64_t)blockIdx.x * kMxBlock + threadIdx.x;
    if (t >= total) return;
    const int64_t ob = t / inner, i = t - ob * inner;
    const int64_t o = ob / nb, kb = ob - o * nb;
    const int64_t base = (o * n + kb * QS_MX_BLOCK) * inner + i;
    const int cnt = (int)((n - kb * QS_MX_BLOCK) < QS_MX_BLOCK ? (n - kb * QS_MX_BLOCK) : QS_MX_BLOCK);
    float v[QS_MX_BLOCK];
#pragma unroll
    for (int j = 0; j < QS_MX_BLOCK; ++j) v[j] = j < cnt ? load1<XDT>(x, base + j * inner) : 0.0f;
    uint32_t am = 0;
#pragma unroll
    for (int j = 0; j < QS_MX_BLOCK; ++j) {
        const uint32_t a = mx_abs_bits(v[j]);
        am = a > am ? a : am;
    }
    const MxScale s = mx_scale(am, f);
    if (scales) scales[t] = (uint8_t)s.byte;
    MxSrKey key = {0u, 0u};
    if constexpr (SR) key = mx_sr_key(sr);
#pragma unroll
    for (int j = 0; j < QS_MX_BLOCK; ++j) {
        if (j < cnt) {
            uint32_t sg;
            const int64_t e = base + j * inner;
            float r;
            if constexpr (SR) r = mx_round_abs_sr(v[j], s, f, mx_sr_word(key, sr.stream, sr.base + (uint64_t)e), sg);
            else r = mx_round_abs(v[j], s, f, sg);
            if (codes) codes[e] = (uint8_t)mx_code(r, sg, s, f);
            const float out = mx_value(r, sg, s);
            if (ydt == QS_F32) store1<QS_F32>(y, e, out);
            else store1<XDT>(y, e, out);
        }
    }
}

}  // namespace qs
