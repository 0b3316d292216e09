// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; constants of Random123), the
// counter-based generator behind the stochastic rounding of the MX quantizers (include/qsparse_hip.h, "Stochastic rounding"; qs_mx.h).
// A pure function of (counter, key): no state, nothing read, nothing written -- the four output words of one call serve the four
// consecutive codes j = 4 q .. 4 q + 3 of an output tensor, so every path that computes a code (vectorised or element by element,
// GPU or CPU) derives the same word for it.
#pragma once
#include <cstdint>

namespace qs {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;       // round multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;       // key increments (Weyl sequence)

// o <- Philox4x32-10(counter c[0..3], key (k0, k1)); `o` may alias `c`
__device__ __forceinline__ void philox4x32_10(const uint32_t (&c)[4], uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
    uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
        const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    o[0] = c0, o[1] = c1, o[2] = c2, o[3] = c3;
}

}  // namespace qs
