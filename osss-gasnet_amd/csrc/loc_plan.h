/* loc_plan.h -- host-only arithmetic of the value-and-location fold
 * (loc.hip, mi355_combine_loc): which form a launch takes (16-byte vectors or
 * element per lane), its grid and what one pass of that grid covers, and how
 * a fold of more sources than one call takes is cut into chained calls.
 * Plain C, no HIP: loc.hip and reduce.c include it, and
 * tests/native/loc_plan_check.cpp compiles it with g++ and the address and
 * undefined-behaviour sanitizers and enumerates it on the CPU. */
#ifndef MI355_LOC_PLAN_H
#define MI355_LOC_PLAN_H 1

#include <stddef.h>
#include <stdint.h>

#define MI355_LOC_MAX_SOURCES 32  /* sources of one call (= MI355_ORDERS_MAX_SOURCES) */
#define MI355_LOC_BLOCK 256       /* threads per block (= launch.h kBlock) */
#define MI355_LOC_BLOCKS_PER_CU 8 /* the streaming cap of launch_plan.h */

enum mi355_loc_form {
    MI355_LOC_VECTOR = 0,  /* one 16-byte vector of values per lane and source, its locations as 16-byte vectors */
    MI355_LOC_ELEMENT = 1, /* one element per lane and source, from the pointers as given */
};

/* One launch. VECTOR: lane t of block b takes vectors (b * 256 + t) + k * pass
 * of the nvec whole ones (per_lane = 16 / es elements each); the `tail`
 * elements after them (< per_lane) go one each to the first lanes of block 0.
 * ELEMENT: the same with units of one element, nvec = n, no tail. */
typedef struct mi355_loc_plan {
    int form;
    unsigned per_lane; /* elements of one unit: 8, 4 or 2 (VECTOR), 1 (ELEMENT) */
    uint64_t nvec;     /* whole units */
    unsigned tail;     /* VECTOR: elements after the last whole vector */
    unsigned grid;     /* blocks; 0: nothing to launch (n == 0) */
    uint64_t pass;     /* units one pass of the whole grid covers: grid * 256 */
} mi355_loc_plan;

/* 1 when every given pointer is 16-byte aligned: the destination pair, every
 * value source and every non-null location source (src_locs itself, or any
 * entry of it, may be NULL: an implicit location reads nothing). */
static inline int mi355_loc_aligned (const void *dst_val, const void *dst_loc, const void *const *src_vals,
                                     const long *const *src_locs, int nsrc)
{
    uintptr_t bits = (uintptr_t) dst_val | (uintptr_t) dst_loc;
    for (int j = 0; j < nsrc; ++j) {
        bits |= (uintptr_t) src_vals[j];
        if (src_locs != NULL)
            bits |= (uintptr_t) src_locs[j];
    }
    return (bits & 15) == 0;
}

/* es: the element size (2, 4 or 8); aligned: mi355_loc_aligned's answer;
 * cus: the GPU's compute units (launch.h device_cus). */
static inline mi355_loc_plan mi355_loc_plan_launch (size_t es, int aligned, uint64_t n, int cus)
{
    mi355_loc_plan p = {aligned ? MI355_LOC_VECTOR : MI355_LOC_ELEMENT, 1, n, 0, 0, 0};
    if (n == 0)
        return p;
    if (aligned) {
        p.per_lane = (unsigned) (16 / es);
        p.nvec = n / p.per_lane;
        p.tail = (unsigned) (n % p.per_lane);
    }
    /* enough blocks to cover the units once, at least one (a tail alone
     * still needs block 0), at most 8 per CU: the grid-stride loop takes the rest */
    uint64_t want = (p.nvec + MI355_LOC_BLOCK - 1) / MI355_LOC_BLOCK;
    const uint64_t cap = (uint64_t) (cus > 0 ? cus : 1) * MI355_LOC_BLOCKS_PER_CU;
    if (want < 1)
        want = 1;
    p.grid = (unsigned) (want < cap ? want : cap);
    p.pass = (uint64_t) p.grid * MI355_LOC_BLOCK;
    return p;
}

/* A fold of nsrc > 32 sources as chained calls: the first takes sources
 * 0 .. 31; each later one has the previous call's output pair as its entry 0
 * (an explicit location array) and up to 31 further sources after it. Entry
 * k >= 1 of such a call is source first + k - 1, so where its location is
 * implicit (loc_base + entry index) the call's loc_base is the fold's plus
 * first - 1. The candidates meet the running winner in ascending source
 * order, as in one call: the same pair, ties included. */
typedef struct mi355_loc_chunk {
    int first;         /* first source that is new in this call */
    int take;          /* how many new sources it takes */
    int lead;          /* 1: entry 0 is the carry (the previous call's output), the new sources follow it */
    long loc_shift;    /* add to the fold's loc_base */
    int final;         /* the fold's last call */
} mi355_loc_chunk;

static inline int mi355_loc_chunk_count (int nsrc)
{
    const int L = MI355_LOC_MAX_SOURCES;
    return nsrc <= L ? 1 : 1 + (nsrc - L + (L - 2)) / (L - 1);
}

/* Chunk c, 0 <= c < mi355_loc_chunk_count (nsrc). */
static inline mi355_loc_chunk mi355_loc_chunk_at (int nsrc, int c)
{
    const int L = MI355_LOC_MAX_SOURCES;
    mi355_loc_chunk k;
    k.lead = c == 0 ? 0 : 1;
    k.first = c == 0 ? 0 : L + (c - 1) * (L - 1);
    k.take = nsrc - k.first;
    if (k.take > L - k.lead)
        k.take = L - k.lead;
    k.loc_shift = (long) k.first - k.lead;
    k.final = k.first + k.take == nsrc;
    return k;
}

#endif /* MI355_LOC_PLAN_H */
