// Top-k routing of a mixture-of-experts layer (include/qsparse_hip.h, "MX MoE routing"): logits [T, E] leave as the gates, the expert
// ids, and the stable counting sort of the T k flat ids by expert (order, its inverse inv, the cumulative ends offs) -- without an
// atomic and without a work-group that waits for another: the result is the same on every run, and nothing can spin.
//
//   mx_moe_route_select_kernel   a work-group owns a TILE of kMoeTile tokens.
//     select   a wave holds one token's logits in registers, lane l the experts l + 64 i (NI of them, a template parameter).  An
//              element is a 64-bit key: the high word is the order-preserving integer image of the float (a NaN at the top, -0 as +0),
//              the low word ~e, so among equal values the LOWER index is the larger key.  Each of the k picks is one wave-wide maximum
//              (the lane's NI keys, then six __shfl_xor steps); the lane that owns the winner retires it (key 0, below every live key).
//              Lane j keeps pick j.  Lanes 0 .. k - 1 evaluate the gates: u_j = top_j - top_0, e_j = msx_exp(u_j), Z summed by the
//              definition's balanced tree over 32 slots -- five __shfl_xor steps, both partners of a step add the same two
//              numbers --, e_j / Z.
//     rank     the tile's ids lie in LDS in flat order.  Wave w ranks the contiguous run [w R, (w + 1) R) of them 64 at a time: a lane
//              reads its expert's running count of the run (s_cnt[w][e]), the wave loops over the DISTINCT experts of the 64 -- the
//              first pending lane's expert, one ballot of the lanes that hold it -- and an id's rank is that count plus the population
//              count of the ballot below the lane; the last lane of every ballot writes the count back.  All reads of a pass precede
//              all its writes (a wave barrier between).
//     prefix   one thread per expert turns the four waves' counts into exclusive bases and the tile's histogram.
//     ONE      (the whole problem is this tile) a block scan over E of the histogram gives offs and the experts' starts, and the
//              kernel writes inv and order itself: one launch, no workspace.
//     TILED    the kernel writes the in-tile rank into inv and hist[tile][e] into the workspace;
//   mx_moe_route_scan_kernel   ONE work-group, one thread per expert, walks the tiles in ascending order (coalesced across the threads)
//     and replaces hist[tile][e] by the exclusive sum over the tiles before it; a block scan of the totals gives offs and start[e];
//   mx_moe_route_place_kernel  pos = start[e] + base[tile][e] + rank; inv[i] = pos, order[pos] = i.
// The sub-wave mappings for E <= 16 / E <= 64 (several tokens per wave) are not built: NI = 1 serves E <= 64 with one token per wave.
#pragma once
#include "qs_mx_softmax.h"      // msx_exp: the definition's exponential, the same text for every unit

namespace qs {

constexpr int kMoeThreads = 256;
constexpr int kMoeWaves = kMoeThreads / 64;
constexpr int kMoeTile = 64;                                    // tokens per tile
constexpr int kMoeMaxE = 1024;
constexpr int kMoeMaxK = 32;
constexpr int kMoeTileIds = kMoeTile * kMoeMaxK;                // 2048: an in-tile rank fits 16 bits
constexpr int kMoeScanThreads = 1024;                           // one per expert

struct MoeRouteArgs {
    const void* logits;
    int64_t stride;              // elements between rows of logits
    float* gates;
    int32_t* experts;
    int32_t* offs;
    int32_t* order;
    int32_t* inv;
    int32_t* hist;               // TILED: [ntiles][E] histograms (then bases), followed by start [E]
    int T, E, k, ntiles;
};

__device__ __forceinline__ uint64_t moe_shfl_xor64(uint64_t v, int off) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    return ((uint64_t)hi << 32) | lo;
}

// inclusive scan of one int per thread over the work-group (blockDim.x / 64 <= 16 waves); `total`: the sum.  Every thread calls it.
__device__ __forceinline__ int moe_block_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    __syncthreads();                                            // (the previous call's reads of s_w)
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    int add = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        const int x = s_w[w];
        add += w < wave ? x : 0;
        tot += x;
    }
    total = tot;
    return v + add;
}

// one token by one wave: the k picks, the gates; the ids go to gates / experts [t, :] and to s_e[0 .. k)
template <int XDT, int NI>
__device__ __forceinline__ void moe_select_token(const MoeRouteArgs& a, int t, int lane, uint16_t* s_e) {
    uint64_t key[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int e = lane + 64 * i;
        key[i] = 0;
        if (e < a.E) {
            uint32_t u = __float_as_uint(load1<XDT>(a.logits, (int64_t)t * a.stride + e));
            u = u == 0x80000000u ? 0u : u;                      // -0 ranks as +0
            key[i] = ((uint64_t)f32_to_key(__uint_as_float(u)) << 32) | (uint32_t)~(uint32_t)e;
        }
    }
    float top = 0.0f;
    int mine = 0;
    for (int j = 0; j < a.k; ++j) {
        uint64_t m = key[0];
#pragma unroll
        for (int i = 1; i < NI; ++i) m = key[i] > m ? key[i] : m;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = moe_shfl_xor64(m, off);
            m = o > m ? o : m;
        }
        const int e = (int)~(uint32_t)m;
#pragma unroll
        for (int i = 0; i < NI; ++i) key[i] = lane + 64 * i == e ? 0ull : key[i];
        if (lane == j) {
            top = key_to_f32((uint32_t)(m >> 32));
            mine = e;
        }
    }
    const float top0 = __shfl(top, 0, 64);
    const float ej = lane < a.k ? msx_exp(top - top0) : 0.0f;
    float Z = ej;                                               // the tree over 32 slots: every lane below 32 ends with the same sum
#pragma unroll
    for (int off = 1; off < kMoeMaxK; off <<= 1) Z = Z + __shfl_xor(Z, off, 64);
    float g = ej / Z;
    g = g != g ? __uint_as_float(0x7fc00000u) : g;
    if (lane < a.k) {
        const int64_t i = (int64_t)t * a.k + lane;
        a.gates[i] = g;
        a.experts[i] = mine;
        s_e[lane] = (uint16_t)mine;
    }
}

template <int XDT, int NI>
__global__ __launch_bounds__(kMoeThreads) void mx_moe_route_select_kernel(MoeRouteArgs a, int one) {
    __shared__ uint16_t s_e[kMoeTileIds], s_rank[kMoeTileIds];
    __shared__ int s_cnt[kMoeWaves * kMoeMaxE];
    __shared__ int s_start[kMoeMaxE];
    __shared__ int s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, t0 = tile * kMoeTile;
    const int ntok = a.T - t0 < kMoeTile ? a.T - t0 : kMoeTile, nid = ntok * a.k, E = a.E;
    for (int i = tid; i < kMoeWaves * E; i += kMoeThreads) s_cnt[i] = 0;
    for (int tl = wave; tl < ntok; tl += kMoeWaves) moe_select_token<XDT, NI>(a, t0 + tl, lane, s_e + tl * a.k);
    __syncthreads();
    // rank: wave w owns the ids [w R, (w + 1) R), R a multiple of 64
    const int R = (nid + kMoeThreads - 1) / kMoeThreads * 64;
    const int hi = (wave + 1) * R < nid ? (wave + 1) * R : nid;
    int* cnt = s_cnt + wave * E;
    for (int c = wave * R; c < hi; c += 64) {
        const int i = c + lane;
        const bool live = i < hi;
        const int e = live ? (int)s_e[i] : -1;
        const int base = live ? cnt[e] : 0;
        int rank = 0, total = 0;
        bool last = false;
        uint64_t todo = __ballot(live);
        while (todo) {
            const int el = __shfl(e, __ffsll((unsigned long long)todo) - 1, 64);
            const uint64_t grp = __ballot(e == el);
            if (e == el) {
                rank = base + __popcll(grp & ((1ull << lane) - 1ull));
                total = __popcll(grp);
                last = (grp >> lane) == 1ull;
            }
            todo &= ~grp;
        }
        __builtin_amdgcn_wave_barrier();
        if (live) s_rank[i] = (uint16_t)rank;
        if (last) cnt[e] = base + total;
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // the four waves' counts -> exclusive bases; the tile's histogram; ONE: its scan over E
    int carry = 0;
    for (int p = 0; p * kMoeThreads < E; ++p) {
        const int e = p * kMoeThreads + tid;
        int total = 0;
        if (e < E) {
#pragma unroll
            for (int w = 0; w < kMoeWaves; ++w) {
                const int cw = s_cnt[w * E + e];
                s_cnt[w * E + e] = total;
                total += cw;
            }
        }
        if (one) {
            int sum;
            const int incl = moe_block_scan(total, s_w, sum) + carry;
            if (e < E) {
                a.offs[e] = incl;
                s_start[e] = incl - total;
            }
            carry += sum;
        } else if (e < E) {
            a.hist[(int64_t)tile * E + e] = total;
        }
    }
    __syncthreads();
    for (int i = tid; i < nid; i += kMoeThreads) {
        const int e = s_e[i];
        const int rank = (int)s_rank[i] + s_cnt[(i / R) * E + e];
        const int gi = t0 * a.k + i;
        if (one) {
            const int pos = s_start[e] + rank;
            a.inv[gi] = pos;
            a.order[pos] = gi;
        } else {
            a.inv[gi] = rank;
        }
    }
}

inline __global__ __launch_bounds__(kMoeScanThreads) void mx_moe_route_scan_kernel(MoeRouteArgs a) {
    __shared__ int s_w[16];
    const int e = threadIdx.x, E = a.E;
    int run = 0;
    if (e < E) {
        for (int tile = 0; tile < a.ntiles; ++tile) {
            const int64_t idx = (int64_t)tile * E + e;
            const int h = a.hist[idx];
            a.hist[idx] = run;
            run += h;
        }
    }
    int sum;
    const int incl = moe_block_scan(run, s_w, sum);
    if (e < E) {
        a.offs[e] = incl;
        a.hist[(int64_t)a.ntiles * E + e] = incl - run;
    }
}

inline __global__ __launch_bounds__(kMoeThreads) void mx_moe_route_place_kernel(MoeRouteArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kMoeThreads + threadIdx.x, n = (int64_t)a.T * a.k;
    if (i >= n) return;
    const int tile = (int)(i / a.k) / kMoeTile, e = a.experts[i], E = a.E;
    const int64_t pos = (int64_t)a.hist[(int64_t)a.ntiles * E + e] + a.hist[(int64_t)tile * E + e] + a.inv[i];
    a.inv[i] = (int)pos;
    if ((uint64_t)pos < (uint64_t)n) a.order[pos] = (int)i;     // (always: the histograms count exactly these ids)
}

}  // namespace qs
