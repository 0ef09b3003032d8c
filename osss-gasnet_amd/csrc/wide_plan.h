/* wide_plan.h -- host-only arithmetic of the widening fold (wide.hip,
 * mi355_combine_wide): which form a launch takes, its grid and what one pass
 * of that grid covers. Plain C, no HIP: wide.hip includes it, the library
 * exports the vector form's shape as mi355_combine_wide_plan, and
 * tests/native/wide_plan_check.c compiles it with gcc and the address and
 * undefined-behaviour sanitizers and enumerates it on the CPU. */
#ifndef MI355_WIDE_PLAN_H
#define MI355_WIDE_PLAN_H 1

#include <stddef.h>
#include <stdint.h>

#include "residency.h"

#define MI355_WIDE_MAX_SOURCES 32  /* sources of one call (= MI355_ORDERS_MAX_SOURCES) */
#define MI355_WIDE_BLOCK 256       /* threads per block (= launch.h kBlock) */
#define MI355_WIDE_PER_LANE 8       /* 16-bit output: elements of one 16-byte load, one 16-byte store */
#define MI355_WIDE_PER_LANE_FLOAT 4 /* float output: elements of one 8-byte load, one 16-byte store */
/* Blocks per CU a grid is capped at: 16 waves per CU, each lane with up to
 * 128 bytes of loads in flight (wide_kernels.h, kWideBatch). The cap stays
 * under the co-residency ceiling of residency.h, so a whole grid is resident
 * at once and a pass is one round of blocks, not several. */
#define MI355_WIDE_BLOCKS_PER_CU 4

#if MI355_WIDE_BLOCKS_PER_CU > MI355_FUSED_RESIDENT_PER_CU
#error "the widening fold's grid must fit the co-residency cap of residency.h"
#endif

enum mi355_wide_form {
    MI355_WIDE_VECTOR = 0,    /* the target 16-byte aligned, every source aligned to its unit: aligned loads */
    MI355_WIDE_UNALIGNED = 1, /* the target 16-byte aligned, some source not: unaligned loads */
    MI355_WIDE_ELEMENT = 2,   /* the target off the 16-byte phase, or less than one unit: one element per lane */
};

/* Elements of one lane's unit in the vector forms: its results are one
 * 16-byte store, its source bytes one load of 2 * per_lane bytes. */
static inline unsigned mi355_wide_per_lane (int float_out)
{
    return float_out ? MI355_WIDE_PER_LANE_FLOAT : MI355_WIDE_PER_LANE;
}

/* One launch. The vector forms: lane t of block b takes the units
 * (b * 256 + t) + k * grid * 256 of the nvec whole ones, k = 0, 1, ...; the
 * `tail` elements after them (< per_lane) go one each to the first lanes of
 * block 0. ELEMENT: the same with units of one element, nvec = n, no tail. */
typedef struct mi355_wide_plan {
    int form;
    unsigned per_lane; /* elements of one unit: 8 or 4 (vector forms), 1 (ELEMENT) */
    uint64_t nvec;     /* whole units */
    unsigned tail;     /* vector forms: elements after the last whole unit */
    unsigned grid;     /* blocks, at least 1 */
    uint64_t pass;     /* elements one pass of the whole grid covers: grid * 256 * per_lane */
} mi355_wide_plan;

/* The form the given pointers take. The target decides: units are stored as
 * aligned 16 bytes, so a target off the 16-byte phase runs element-wise;
 * sources off their unit's alignment (16 bytes, float output: 8) are read
 * with unaligned loads. */
static inline int mi355_wide_form_of (int float_out, const void *dst, const void *const *srcs, int nsrc, uint64_t n)
{
    const unsigned per_lane = mi355_wide_per_lane (float_out);
    if (((uintptr_t) dst & 15) != 0 || n < per_lane)
        return MI355_WIDE_ELEMENT;
    uintptr_t bits = 0;
    for (int j = 0; j < nsrc; ++j)
        bits |= (uintptr_t) srcs[j];
    return (bits & (2 * per_lane - 1)) == 0 ? MI355_WIDE_VECTOR : MI355_WIDE_UNALIGNED;
}

/* form: mi355_wide_form_of's answer; float_out: the output is binary32;
 * cus: the GPU's compute units. */
static inline mi355_wide_plan mi355_wide_plan_launch (int form, int float_out, uint64_t n, int cus)
{
    mi355_wide_plan p = {form, 1, n, 0, 1, 0};
    if (form != MI355_WIDE_ELEMENT) {
        p.per_lane = mi355_wide_per_lane (float_out);
        p.nvec = n / p.per_lane;
        p.tail = (unsigned) (n % p.per_lane);
    }
    /* enough blocks to cover the units once, at least one (a tail alone
     * still needs block 0); the grid-stride loop takes the rest */
    uint64_t want = (p.nvec + MI355_WIDE_BLOCK - 1) / MI355_WIDE_BLOCK;
    const uint64_t cap = (uint64_t) (cus > 0 ? cus : 1) * MI355_WIDE_BLOCKS_PER_CU;
    if (want < 1)
        want = 1;
    p.grid = (unsigned) (want < cap ? want : cap);
    p.pass = (uint64_t) p.grid * MI355_WIDE_BLOCK * p.per_lane;
    return p;
}

#endif /* MI355_WIDE_PLAN_H */
