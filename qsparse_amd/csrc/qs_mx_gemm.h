// Matrix product on MX codes (include/qsparse_hip.h, "MX matrix product"): y[M, N] = A[M, K] . B[N, K]^T on the byte codes and
// E8M0 block scales the MX quantizer writes, through v_mfma_scale_f32_16x16x128_f8f6f4 -- FP8 / FP6 / FP4 operands of either format
// on either side, one scale byte per 32 elements of K, float32 accumulation.
//
// Lane maps of the instruction (measured: tools/probes/probe_mfma_scale.py, profiles/mx_mfma_scale_probe.txt).
// D[16, 16] = SrcA[16, 128] . SrcB[128, 16]; lane l = 16 g + i holds row i of SrcA / column i of SrcB:
//   FP6, FP4  k = 32 g + j, j = 0..31: one MX block, element j in bits [w j, w j + w) of the lane's operand registers taken as one
//             little-endian bit string (w = 6 / 4: 6 / 4 registers)
//   FP8       registers 0..3: k = 16 g + j, registers 4..7: k = 64 + 16 g + j, j = 0..15 (one byte each, ascending): HALF of block
//             g >> 1 and half of block 2 + (g >> 1)
//   scale     byte 0 (opsel 0) of lane l's scale register is the E8M0 byte of block g of row / column i, 2^(byte - 127), for EVERY
//             format -- for FP8 it therefore scales elements that sit in other lanes' registers.  0xFF: NaN in every output of
//             that row / column, whatever the codes (zero codes included), so the kernel adds no handling of its own
//   C / D     col = l & 15, row = 4 (l >> 4) + register
// The kernel puts the WEIGHT (B, [N, K]) on SrcA and the ACTIVATION (A, [M, K]) on SrcB: a lane then holds four CONSECUTIVE n of
// one output row m in its four accumulator registers and writes them with one 16-byte (float32) store.
//
// One work-group of 4 waves (2 along n x 2 along m) owns a 128 (m) x 128 (n) tile of y and walks K in steps of 128.  Per step each
// thread brings four 16-code pieces of either operand from global memory into registers (the loads of step t + 1 are issued
// before the products of step t), packs them to the operand width (FP8 as is, FP6 16 -> 12 bytes, FP4 16 -> 8 bytes) and writes
// them to the other of two LDS buffers so that the two pieces a lane needs lie side by side (FP8: pieces g and 4 + g, FP6 / FP4:
// 2 g and 2 g + 1); a lane reads them back as one packed fragment (32 / 24 / 16 bytes) and issues 16 MFMAs into 16 independent
// accumulators.  The LDS image of a row is its four fragments in an order XOR-ed with the row number so that the 16 rows a fragment
// read touches spread over the banks.  One barrier per step.  Scale bytes go global -> register.
//   VEC   (K % 16 == 0, both code bases 16-byte aligned): every piece is one 16-byte load, wholly inside or wholly outside K
//   !VEC  any K, any base: the same kernel with byte loads, each predicated on its own k
// Rows past M / N and codes past K are zero codes (value +0 in every format), their scale byte 127; nothing outside the operands
// is read or written.
#pragma once
#include "qs_common.h"
#include "qs_mx.h"

namespace qs {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMxgTile = 128;      // rows of A and of B per work-group
constexpr int kMxgK = 128;         // K per step = K of one MFMA
constexpr int kMxgThreads = 256;

__host__ __device__ constexpr int mxg_bits(int format) { return format <= QS_MX_FP8_E5M2 ? 8 : (format <= QS_MX_FP6_E3M2 ? 6 : 4); }

// 16 codes (one per byte) -> 2 * BITS bytes in the low registers of the result
template <int BITS>
__device__ __forceinline__ u32x4 mxg_pack16(u32x4 x) {
    if constexpr (BITS == 8) {
        return x;
    } else if constexpr (BITS == 4) {
        u32x4 t;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t m = x[i] & 0x0f0f0f0fu;
            t[i] = m | (m >> 4);                   // bytes 0 and 2: two codes each
        }
        return u32x4{__builtin_amdgcn_perm(t[1], t[0], 0x06040200u), __builtin_amdgcn_perm(t[3], t[2], 0x06040200u), 0u, 0u};
    } else {
        uint32_t p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            p[i] = (x[i] & 0x3fu) | ((x[i] >> 2) & 0xfc0u) | ((x[i] >> 4) & 0x3f000u) | ((x[i] >> 6) & 0xfc0000u);     // 4 codes: 24 bits
        return u32x4{p[0] | (p[1] << 24), (p[1] >> 8) | (p[2] << 16), (p[2] >> 16) | (p[3] << 8), 0u};
    }
}

template <int BITS>
struct MxgLds {
    static constexpr int kRow = 16 * BITS;         // bytes of one row of 128 codes
    static constexpr int kPiece = 2 * BITS;        // bytes of 16 codes
    static constexpr int kBytes = kMxgTile * kRow;
    // the position of lane group f's fragment (0..3) of row r among the row's four fragment slots
    static __device__ __forceinline__ int slot(int r, int f) { return f ^ ((BITS == 4 ? r >> 2 : r >> 1) & 3); }

    static __device__ __forceinline__ void put(uint8_t* tile, int r, int c, u32x4 raw) {      // piece c (0..7) of row r
        const u32x4 v = mxg_pack16<BITS>(raw);
        const int f = BITS == 8 ? c & 3 : c >> 1, h = BITS == 8 ? c >> 2 : c & 1;      // whose fragment, which half of it
        uint8_t* p = tile + r * kRow + (slot(r, f) * 2 + h) * kPiece;
        if constexpr (BITS == 8) {
            *(u32x4*)p = v;
        } else if constexpr (BITS == 4) {
            *(u32x2*)p = u32x2{v[0], v[1]};
        } else {
            uint32_t* q = (uint32_t*)p;
            q[0] = v[0], q[1] = v[1], q[2] = v[2];
        }
    }

    static __device__ __forceinline__ i32x8 get(const uint8_t* tile, int r, int f) {           // lane group f's operand of row r
        const uint8_t* p = tile + r * kRow + slot(r, f) * 2 * kPiece;
        i32x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (BITS == 8) {
            const u32x4 a = *(const u32x4*)p, b = *(const u32x4*)(p + 16);
            o = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
        } else if constexpr (BITS == 4) {
            const u32x4 a = *(const u32x4*)p;
            o[0] = (int)a[0], o[1] = (int)a[1], o[2] = (int)a[2], o[3] = (int)a[3];
        } else {
            const u32x2 a = *(const u32x2*)p, b = *(const u32x2*)(p + 8), c = *(const u32x2*)(p + 16);
            o[0] = (int)a[0], o[1] = (int)a[1], o[2] = (int)b[0], o[3] = (int)b[1], o[4] = (int)c[0], o[5] = (int)c[1];
        }
        return o;
    }
};

// 16 codes from codes + off if `in`, else zeros; `left` (1..16) of them exist (!VEC: the bytes past it are not read)
template <bool VEC>
__device__ __forceinline__ u32x4 mx_load16(const uint8_t* __restrict__ codes, bool in, int64_t off, int left) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if constexpr (VEC) {                           // an unconditional load from a clamped address, then a select: no branch per piece
        const u32x4 w = *(const u32x4*)(codes + (in ? off : 0));
        v = in ? w : v;
    } else if (in) {
        const uint8_t* p = codes + off;
#pragma unroll
        for (int b = 0; b < 16; ++b)
            if (b < left) v[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    }
    return v;
}

// the scale byte at scales + off if `in`, else 127 (2^0); clamped address + select, as the pieces
__device__ __forceinline__ uint32_t mx_scale(const uint8_t* __restrict__ scales, bool in, int64_t off) {
    const uint32_t b = scales[in ? off : 0];
    return in ? b : 127u;
}

// the four pieces a thread stages per step: piece q = thread + 256 i is piece (q & 7) of tile row (q >> 3) = (thread >> 3) + 32 i
template <int BITS>
__device__ __forceinline__ void mxg_stage(uint8_t* tile, const u32x4 (&reg)[4], int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid + kMxgThreads * i;
        MxgLds<BITS>::put(tile, q >> 3, q & 7, reg[i]);
    }
}

template <int FA, int FB>
constexpr int kMxTileLds = 2 * (MxgLds<mxg_bits(FA)>::kBytes + MxgLds<mxg_bits(FB)>::kBytes);       // two buffers of both operands

// The K loop of the implicit-GEMM products on MX codes, parameterised by its operands (the loop of mx_gemm_kernel below, which
// keeps a statement of its own).  An OPERAND is one side of the product seen through the tile; it has
//   fetch<VEC>(reg, step)   the four 16-code pieces this thread stages at K-step `step`: piece (thread & 7) of the tile rows
//                           (thread >> 3) + 32 i
//   scales(s, step)         the scale bytes of block (lane >> 4) of that step for this lane's four fragments: the tile rows
//                           w + 16 j + (lane & 15), w the wave's corner
//   advance()               called once before the fetch of each step after the first, in ascending order
// Models: MxcOperand (qs_mx_conv.h; an image or a weight under a convolution's window), MxctOperand (qs_mx_conv_t.h; an image under
// a transposed convolution's).  A is the activation (SrcB of the instruction, tile
// rows m, corner wm), B the weight (SrcA, rows n, corner wn).  The loop walks the steps [t0, t1), t0 < t1, from whatever `acc`
// holds: the loads of step t + 1 are issued before the 16 MFMAs of step t and staged into the other buffer after them, one barrier
// per step; the buffer of step t is (t - t0) & 1.
template <int FA, int FB, bool VEC, class OpA, class OpB>
__device__ __forceinline__ void mx_tile_loop(f32x4 (&acc)[4][4], OpA& A, OpB& B, int64_t t0, int64_t t1, uint8_t* lds, int tid, int wm,
                                             int wn) {
    using LA = MxgLds<mxg_bits(FA)>;
    using LB = MxgLds<mxg_bits(FB)>;
    constexpr int kBuf = LA::kBytes + LB::kBytes;
    const int lane = tid & 63;

    u32x4 ra[4], rb[4];
    uint32_t sa[4], sb[4], sa_next[4], sb_next[4];
    A.template fetch<VEC>(ra, t0);
    B.template fetch<VEC>(rb, t0);
    A.scales(sa, t0);
    B.scales(sb, t0);
    mxg_stage<mxg_bits(FA)>(lds, ra, tid);
    mxg_stage<mxg_bits(FB)>(lds + LA::kBytes, rb, tid);
    __syncthreads();

    for (int64_t t = t0; t < t1; ++t) {
        const bool more = t + 1 < t1;
        if (more) {
            A.advance();
            B.advance();
            A.template fetch<VEC>(ra, t + 1);
            B.template fetch<VEC>(rb, t + 1);
            A.scales(sa_next, t + 1);
            B.scales(sb_next, t + 1);
        }
        const uint8_t* cur = lds + ((t - t0) & 1) * kBuf;
        i32x8 fa[4], fb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fa[j] = LA::get(cur, wm + 16 * j + (lane & 15), lane >> 4);
            fb[j] = LB::get(cur + LA::kBytes, wn + 16 * j + (lane & 15), lane >> 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[i], fa[j], acc[i][j], FB, FA, 0, (int)sb[i], 0, (int)sa[j]);
        if (more) {
            uint8_t* nxt = lds + ((t + 1 - t0) & 1) * kBuf;
            mxg_stage<mxg_bits(FA)>(nxt, ra, tid);
            mxg_stage<mxg_bits(FB)>(nxt + LA::kBytes, rb, tid);
#pragma unroll
            for (int j = 0; j < 4; ++j) sa[j] = sa_next[j], sb[j] = sb_next[j];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void mx_zero(f32x4 (&acc)[4][4]) {       // [i: 16 n][j: 16 m]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// v[0..3] rounded once to ydt at y[e .. e + 3], the elements (m, n .. n + 3) of y [M, N]; those with n + r >= N are not written.
// y_vec: N % 4 == 0 and y 16-byte (float32) / 8-byte aligned, so n + 3 < N and one aligned store takes the four
__device__ __forceinline__ void mx_store4(void* __restrict__ y, int ydt, int64_t e, const float (&v)[4], int64_t n, int64_t N, int y_vec) {
    if (y_vec) {
        if (ydt == QS_F32) {
            *(u32x4*)((float*)y + e) = u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
        } else if (ydt == QS_BF16) {
            *(u32x2*)((uint16_t*)y + e) = u32x2{f32_to_bf16_bits(v[0]) | (f32_to_bf16_bits(v[1]) << 16),
                                                f32_to_bf16_bits(v[2]) | (f32_to_bf16_bits(v[3]) << 16)};
        } else {
            *(u32x2*)((uint16_t*)y + e) = u32x2{f32_to_f16_bits(v[0]) | (f32_to_f16_bits(v[1]) << 16),
                                                f32_to_f16_bits(v[2]) | (f32_to_f16_bits(v[3]) << 16)};
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (n + r >= N) break;
            if (ydt == QS_F32) ((float*)y)[e + r] = v[r];
            else if (ydt == QS_BF16) ((uint16_t*)y)[e + r] = (uint16_t)f32_to_bf16_bits(v[r]);
            else ((uint16_t*)y)[e + r] = (uint16_t)f32_to_f16_bits(v[r]);
        }
    }
}

// bias in float32, one rounding to ydt, the stores of a wave's 64 (m, from mw) x 64 (n, from nw) corner of y [M, N]
__device__ __forceinline__ void mx_epilogue(const f32x4 (&acc)[4][4], const float* __restrict__ bias, void* __restrict__ y, int ydt,
                                            int64_t M, int64_t N, int64_t mw, int64_t nw, int lane, int y_vec) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t n = nw + 16 * i + 4 * (lane >> 4);
        float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (bias) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < N) bv[r] = bias[n + r];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t m = mw + 16 * j + (lane & 15);
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = bias ? acc[i][j][r] + bv[r] : acc[i][j][r];
            if (m >= M || n >= N) continue;
            mx_store4(y, ydt, m * N + n, v, n, N, y_vec);
        }
    }
}

// The quantizing epilogue (include/qsparse_hip.h, "MX products that write MX codes"): bias in float32, the optional ReLU, then the MX
// quantizer of qs_mx.h on the wave's 64 (m, from mw) x 64 (n, from nw) corner with blocks of 32 along n -- codes [M, N] and scale
// bytes [M, ceil(N / 32)] instead of y.  A block is one row m and the 32 columns nw + 32 b ..: the accumulators acc[2 b][j] and
// acc[2 b + 1][j] (4 consecutive n each) of the four lanes l, l + 16, l + 32, l + 48 that share m = mw + 16 j + (l & 15).  So its
// abs-max is the maximum over 8 values in the lane and two __shfl_xor steps (lane bits 4 and 5); every lane then holds the block's
// scale and rounds its own 8 values.  nw is a multiple of 64: no block straddles two waves.  Columns n >= N of a short last block
// are taken as +0 whatever the accumulator holds (zero codes and no bias give +0 there, but a row of A that holds an Inf code
// gives Inf * 0 = NaN), so they leave the maximum alone, as the quantizer's padding does.  Rows m >= M, columns n >= N and blocks
// that start at or past N are never written.
// c_vec: N % 4 == 0 and codes 4-byte aligned, so n + 3 < N and one aligned 4-byte store takes a lane's four codes
__device__ __forceinline__ void mx_epilogue_codes(const f32x4 (&acc)[4][4], const float* __restrict__ bias, int relu, const MxFormat& f,
                                                  uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t M, int64_t N,
                                                  int64_t mw, int64_t nw, int lane, int c_vec) {
    const int64_t nb = (N + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int64_t n0 = nw + QS_MX_BLOCK * b;                    // the block's first column
        float bv[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
        if (bias) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t n = n0 + 16 * h + 4 * (lane >> 4) + r;
                    if (n < N) bv[h][r] = bias[n];
                }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t m = mw + 16 * j + (lane & 15);
            float u[2][4];
            uint32_t am = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = bias ? acc[2 * b + h][j][r] + bv[h][r] : acc[2 * b + h][j][r];
                    if (relu) v = v > 0.0f ? v : (v != v ? v : 0.0f);
                    if (n0 + 16 * h + 4 * (lane >> 4) + r >= N) v = 0.0f;       // (an Inf code in row m times the zero codes past N: NaN)
                    u[h][r] = v;
                    const uint32_t a = mx_abs_bits(v);
                    am = a > am ? a : am;
                }
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) {               // (every lane of the wave takes part: before any early exit)
                const uint32_t o = (uint32_t)__shfl_xor((int)am, off, 64);
                am = o > am ? o : am;
            }
            if (m >= M || n0 >= N) continue;
            const MxScale s = mx_scale(am, f);
            if ((lane >> 4) == 0) scales[m * nb + (n0 >> 5)] = (uint8_t)s.byte;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t n = n0 + 16 * h + 4 * (lane >> 4);
                if (n >= N) continue;
                uint32_t c[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    uint32_t sg;
                    const float q = mx_round_abs(u[h][r], s, f, sg);
                    c[r] = mx_code(q, sg, s, f);
                }
                uint8_t* p = codes + m * N + n;
                if (c_vec) {
                    *(uint32_t*)p = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n + r < N) p[r] = (uint8_t)c[r];
                }
            }
        }
    }
}

// mx_gemm_kernel and mx_gemm_partial_kernel (qs_mx_gemm_splitk.h) state the fetch, the loop and the epilogue themselves, statement
// for statement what mx_load16 / mx_scale / mx_tile_loop / mx_epilogue say: built on those, with a row-major operand of their own,
// they gave the same bits from fewer registers but were 3-17 % slower where K is short or the tiles are few.
// Outside the loop a call stands only where the assembly stays the written-out text's: mx_zero in mx_gemm_kernel.
// Its epilogue, and the zeroing and the store of mx_gemm_partial_kernel, stay written out: each call reschedules all 50 instantiations.
// the four 16-code pieces this thread stages per step: piece q = thread + 256 i is piece (q & 7) of tile row (q >> 3)
template <bool VEC>
__device__ __forceinline__ void mxg_fetch(u32x4 (&reg)[4], const uint8_t* __restrict__ codes, int64_t row0, int64_t rows, int64_t K,
                                          int64_t k0, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid + kMxgThreads * i;
        const int64_t row = row0 + (q >> 3), k = k0 + (q & 7) * 16;
        const bool in = row < rows && k < K;
        u32x4 v = {0u, 0u, 0u, 0u};
        if constexpr (VEC) {                       // an unconditional load from a clamped address, then a select: no branch per piece
            const u32x4 w = *(const u32x4*)(codes + (in ? row * K + k : 0));
            v = in ? w : v;
        } else if (in) {
            const uint8_t* p = codes + row * K + k;
            const int left = (int)(K - k < 16 ? K - k : 16);
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (b < left) v[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
        }
        reg[i] = v;
    }
}

// the scale bytes of this lane's four fragments (rows r0 + 16 j + (lane & 15)) at block kb; 127 (2^0) where there is none
__device__ __forceinline__ void mxg_scales(uint32_t (&s)[4], const uint8_t* __restrict__ scales, int64_t r0, int64_t rows, int64_t nkb,
                                           int64_t kb, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t row = r0 + 16 * j + (lane & 15);
        const bool in = row < rows && kb < nkb;
        const uint32_t b = scales[in ? row * nkb + kb : 0];       // (clamped address + select, as the pieces)
        s[j] = in ? b : 127u;
    }
}

template <int FA, int FB, bool VEC>
__global__ __launch_bounds__(kMxgThreads) void mx_gemm_kernel(const uint8_t* __restrict__ a_codes, const uint8_t* __restrict__ a_scales,
                                                              const uint8_t* __restrict__ b_codes, const uint8_t* __restrict__ b_scales,
                                                              const float* __restrict__ bias, void* __restrict__ y, int ydt, int64_t M,
                                                              int64_t N, int64_t K, int tiles_n, int y_vec) {
    using LA = MxgLds<mxg_bits(FA)>;
    using LB = MxgLds<mxg_bits(FB)>;
    constexpr int kBuf = LA::kBytes + LB::kBytes;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kBuf];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * kMxgTile, n0 = (int64_t)(blockIdx.x % tiles_n) * kMxgTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;          // this wave's 64 x 64 corner of the tile
    const int64_t nkb = (K + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    const int64_t steps = (K + kMxgK - 1) / kMxgK;

    f32x4 acc[4][4];                                                // [i: 16 n][j: 16 m]
    mx_zero(acc);

    u32x4 ra[4], rb[4];
    uint32_t sa[4], sb[4], sa_next[4], sb_next[4];
    mxg_fetch<VEC>(ra, a_codes, m0, M, K, 0, tid);
    mxg_fetch<VEC>(rb, b_codes, n0, N, K, 0, tid);
    mxg_scales(sa, a_scales, m0 + wm, M, nkb, lane >> 4, lane);
    mxg_scales(sb, b_scales, n0 + wn, N, nkb, lane >> 4, lane);
    mxg_stage<mxg_bits(FA)>(lds, ra, tid);
    mxg_stage<mxg_bits(FB)>(lds + LA::kBytes, rb, tid);
    __syncthreads();

    for (int64_t t = 0; t < steps; ++t) {
        const bool more = t + 1 < steps;
        if (more) {
            mxg_fetch<VEC>(ra, a_codes, m0, M, K, (t + 1) * kMxgK, tid);
            mxg_fetch<VEC>(rb, b_codes, n0, N, K, (t + 1) * kMxgK, tid);
            mxg_scales(sa_next, a_scales, m0 + wm, M, nkb, (t + 1) * 4 + (lane >> 4), lane);
            mxg_scales(sb_next, b_scales, n0 + wn, N, nkb, (t + 1) * 4 + (lane >> 4), lane);
        }
        const uint8_t* cur = lds + (t & 1) * kBuf;
        i32x8 fa[4], fb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fa[j] = LA::get(cur, wm + 16 * j + (lane & 15), lane >> 4);
            fb[j] = LB::get(cur + LA::kBytes, wn + 16 * j + (lane & 15), lane >> 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[i], fa[j], acc[i][j], FB, FA, 0, (int)sb[i], 0, (int)sa[j]);
        if (more) {
            uint8_t* nxt = lds + ((t + 1) & 1) * kBuf;
            mxg_stage<mxg_bits(FA)>(nxt, ra, tid);
            mxg_stage<mxg_bits(FB)>(nxt + LA::kBytes, rb, tid);
#pragma unroll
            for (int j = 0; j < 4; ++j) sa[j] = sa_next[j], sb[j] = sb_next[j];
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t n = n0 + wn + 16 * i + 4 * (lane >> 4);
        float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (bias) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < N) bv[r] = bias[n + r];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t m = m0 + wm + 16 * j + (lane & 15);
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = bias ? acc[i][j][r] + bv[r] : acc[i][j][r];
            if (m >= M || n >= N) continue;
            const int64_t e = m * N + n;
            if (y_vec) {                           // N % 4 == 0 and y 16-byte (float32) / 8-byte aligned: n + 3 < N, aligned store
                if (ydt == QS_F32) {
                    *(u32x4*)((float*)y + e) = u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
                } else if (ydt == QS_BF16) {
                    *(u32x2*)((uint16_t*)y + e) = u32x2{f32_to_bf16_bits(v[0]) | (f32_to_bf16_bits(v[1]) << 16),
                                                        f32_to_bf16_bits(v[2]) | (f32_to_bf16_bits(v[3]) << 16)};
                } else {
                    *(u32x2*)((uint16_t*)y + e) = u32x2{f32_to_f16_bits(v[0]) | (f32_to_f16_bits(v[1]) << 16),
                                                        f32_to_f16_bits(v[2]) | (f32_to_f16_bits(v[3]) << 16)};
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (n + r >= N) break;
                    if (ydt == QS_F32) ((float*)y)[e + r] = v[r];
                    else if (ydt == QS_BF16) ((uint16_t*)y)[e + r] = (uint16_t)f32_to_bf16_bits(v[r]);
                    else ((uint16_t*)y)[e + r] = (uint16_t)f32_to_f16_bits(v[r]);
                }
            }
        }
    }
}

}  // namespace qs
