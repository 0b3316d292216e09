// The item map of the ragged launches (include/qsparse_hip.h, "MX flash attention, ragged" and "MX KV cache append, ragged"): a flat
// token axis [Ttot] cut into B sequences by cu_seqlens [B + 1] that only the device reads.  Sequence b owns n_b = count(T_b) items (tiles
// of 64 packed rows in the attention kernel, whole middle blocks of vt in the append); the grid is sized on the shapes alone, and every
// work-group finds the (b, index) of ITS item from the prefix sum of n_b, which it computes itself:
//   the 64 lanes of ONE wave take 64 entries of cu_seqlens per round (two vector loads each, clamped), n_b is summed over the wave by a
//   Hillis-Steele scan of six shuffles, a ballot over "my prefix <= item < my prefix + n_b" names the owner, three shuffles fetch its
//   sequence, first token and length; the round's total carries into the next.  The search ends in the round that holds the item, or
//   behind entry B - 1: the item lies past the total and its work-group has nothing to do.
// Every entry is clamped into [0, Ttot] and a negative length counts as 0, so the tokens [lo, lo + T_b) of whatever sequence is found
// lie inside the flat operands whatever cu_seqlens holds.  Counts are unsigned: a round adds at most 64 counts of at most 2^25 to a
// prefix that has not yet passed an item below 2^31.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qs {

struct MxRaggedItem {
    int b, idx, lo, T;                                          // the sequence, the item's index in it, its first flat token, its length
};

__device__ __forceinline__ int mxrg_clamp(int v, int Ttot) { return v < 0 ? 0 : (v > Ttot ? Ttot : v); }

// (lo, T_b) of sequence b < B: two vector loads (the address is the lane's own), then wave-uniform
__device__ __forceinline__ void mxrg_seq(const int32_t* __restrict__ cu, int b, int Ttot, int& lo, int& T) {
    const int z = (int)__builtin_amdgcn_mbcnt_lo(0u, 0u);       // (+ 0, in a vector register)
    const int l = __builtin_amdgcn_readfirstlane(mxrg_clamp(cu[b + z], Ttot));
    const int h = __builtin_amdgcn_readfirstlane(mxrg_clamp(cu[b + 1 + z], Ttot));
    lo = l, T = h > l ? h - l : 0;
}

// run by all 64 lanes of one wave: the item `item` (wave-uniform) of the map whose sequence b holds count(T_b) items; false: past the total
template <class F>
__device__ __forceinline__ bool mxrg_find(const int32_t* __restrict__ cu, int B, int Ttot, unsigned item, F count, MxRaggedItem& out) {
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    unsigned base = 0;                                          // the items of the rounds before (wave-uniform)
    for (int e0 = 0; e0 < B; e0 += 64) {
        const int e = e0 + lane;
        int lo = 0, T = 0;
        if (e < B) {
            lo = mxrg_clamp(cu[e], Ttot);
            const int hi = mxrg_clamp(cu[e + 1], Ttot);
            T = hi > lo ? hi - lo : 0;
        }
        const unsigned n = e < B ? (unsigned)count(T) : 0u;
        unsigned inc = n;                                       // the inclusive prefix over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = (unsigned)__shfl_up((int)inc, off, 64);
            inc += lane >= off ? up : 0u;
        }
        const unsigned start = base + inc - n;
        const unsigned long long owner = __ballot(item >= start && item - start < n);
        if (owner != 0ull) {                                    // (wave-uniform)
            const int src = __builtin_ctzll(owner);
            out.b = e0 + src;
            out.idx = (int)(item - (unsigned)__shfl((int)start, src, 64));
            out.lo = __shfl(lo, src, 64);
            out.T = __shfl(T, src, 64);
            return true;
        }
        base += (unsigned)__shfl((int)inc, 63, 64);
    }
    return false;
}

// the work-group's item: wave 0 searches, the others take the result from `slot` (five ints of LDS) behind one barrier
template <class F>
__device__ __forceinline__ bool mxrg_item(int* slot, const int32_t* __restrict__ cu, int B, int Ttot, unsigned item, F count,
                                          MxRaggedItem& out) {
    if (threadIdx.x < 64) {                                     // (wave-uniform)
        MxRaggedItem it{0, 0, 0, 0};
        const bool found = mxrg_find(cu, B, Ttot, item, count, it);
        if (threadIdx.x == 0) slot[0] = (int)found, slot[1] = it.b, slot[2] = it.idx, slot[3] = it.lo, slot[4] = it.T;
    }
    __syncthreads();
    out.b = __builtin_amdgcn_readfirstlane(slot[1]), out.idx = __builtin_amdgcn_readfirstlane(slot[2]);
    out.lo = __builtin_amdgcn_readfirstlane(slot[3]), out.T = __builtin_amdgcn_readfirstlane(slot[4]);
    return __builtin_amdgcn_readfirstlane(slot[0]) != 0;
}

}  // namespace qs
