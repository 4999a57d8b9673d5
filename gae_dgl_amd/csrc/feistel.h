// The keyed permutation behind every shuffled epoch (K27's mini-batch order, K38's walk order): four Feistel rounds on
// 2 `half` bits whose round function is a Philox block, cycle-walked into [0, count).
#pragma once
#include "common.h"

namespace gae {
namespace feistel {

// the smallest `half` with 4^half >= count (at least 1)
__host__ __device__ inline int half_bits(uint64_t count)
{
    int half = 1;
    while ((uint64_t(1) << (2 * half)) < count) ++half;
    return half;
}

// position p of epoch `epoch` -> an index of [0, ntr): four Feistel rounds on 2 `half` bits, cycle-walked
__device__ __forceinline__ uint32_t shuffled(uint32_t p, uint32_t ntr, int half, uint64_t seed, uint32_t epoch)
{
    const uint32_t mask = (1u << half) - 1u;
    uint32_t v = p;
    do {
        uint32_t hi = v >> half, lo = v & mask;
        for (uint32_t r = 0; r < 4; ++r) {
            uint32_t c[4];
            gae::philox4x32_10((uint64_t(r) << 32) | lo, (uint64_t(1) << 32) + epoch, seed, c);
            const uint32_t nx = hi ^ (c[0] & mask);
            hi = lo; lo = nx;
        }
        v = (hi << half) | lo;
    } while (v >= ntr);
    return v;
}

} // namespace feistel
} // namespace gae
