// amo_plan.h -- the atomic accumulate's launch shape (amo.hip). Host-only
// integer arithmetic, like launch_plan.h and prefix_plan.h: the library
// exports it as mi355_atomic_add_v_plan so that a CPU test can enumerate it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mi355k {

constexpr int kAddvBlock = 256;     // = kBlock
constexpr int kAddvUnroll = 4;      // source loads in flight per lane
constexpr int kAddvBlocksPerCU = 8; // 32 waves per CU: each holds at most 4 atomics outstanding

struct AddvPlan {
    unsigned grid;  // blocks; 0: nothing to launch
    uint64_t pass;  // elements one pass of the whole grid covers
};

// One block covers 256 x 4 elements per pass: slot u of lane t is element
// base + u * 256 + t, so every wave-instruction, load or atomic, touches 64
// consecutive elements (256 contiguous bytes of dwords, 512 of qwords)
// whatever the pointers' phases. Enough blocks to cover n once, capped at 8
// resident blocks per CU (grid_for's convention); the grid-stride loop takes
// the rest.
inline AddvPlan plan_atomic_add_v(uint64_t n, int cus) {
    const uint64_t per_block = (uint64_t)kAddvBlock * kAddvUnroll;
    if (n == 0) return {0, 0};
    const uint64_t want = (n + per_block - 1) / per_block;
    const uint64_t cap = (uint64_t)(cus > 0 ? cus : 1) * kAddvBlocksPerCU;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    return {grid, (uint64_t)grid * per_block};
}

}  // namespace mi355k
