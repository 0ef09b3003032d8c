/* wide_plan_check.c -- the widening fold's host arithmetic
 * (osss-gasnet_amd/csrc/wide_plan.h) enumerated on the CPU, built by
 * tests/test_wide_plan.py with the address and undefined-behaviour sanitizers
 * as an ordinary program. For every size around a vector, a block and a grid
 * pass, three CU counts, both outputs and the three forms it checks that the
 * grid is at least 1 and within the co-residency cap of residency.h, that a
 * pass is the grid times the elements of a block, and that the ranges the
 * kernels' index arithmetic hands out -- lane t of block b takes unit
 * (k * grid + b) * 256 + t of pass k, block 0's first lanes the tail -- tile
 * [0, n) exactly: in order, no gap, no overlap, nothing past n. It also walks
 * mi355_wide_form_of over every pointer phase. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "wide_plan.h"

static long violations, launches;

static void fail (const char *what, int form, int fo, uint64_t n, int cus)
{
    if (violations++ < 20)
        printf ("VIOLATION %s: form %d float_out %d n %llu cus %d\n", what, form, fo, (unsigned long long) n, cus);
}

static void check_launch (int form, int fo, uint64_t n, int cus)
{
    const mi355_wide_plan p = mi355_wide_plan_launch (form, fo, n, cus);
    const unsigned per_lane = form == MI355_WIDE_ELEMENT ? 1 : fo ? MI355_WIDE_PER_LANE_FLOAT : MI355_WIDE_PER_LANE;
    ++launches;
    if (p.form != form || p.per_lane != per_lane)
        fail ("form", form, fo, n, cus);
    if (p.grid < 1)
        fail ("grid < 1", form, fo, n, cus);
    if ((uint64_t) p.grid > (uint64_t) cus * MI355_FUSED_RESIDENT_PER_CU)
        fail ("grid above the co-residency cap", form, fo, n, cus);
    if (p.pass != (uint64_t) p.grid * MI355_WIDE_BLOCK * per_lane)
        fail ("pass", form, fo, n, cus);
    if (p.nvec * per_lane + p.tail != n || p.tail >= per_lane || p.tail > MI355_WIDE_BLOCK)
        fail ("units", form, fo, n, cus);
    /* a grid that covers the units once is no larger than it must be */
    if (p.grid > 1 && (uint64_t) (p.grid - 1) * MI355_WIDE_BLOCK >= p.nvec)
        fail ("an idle block", form, fo, n, cus);

    /* the blocks' ranges of every pass, in the order (pass, block): each is
     * 256 lanes x per_lane consecutive elements, cut at the last whole unit */
    uint64_t cursor = 0;
    const uint64_t units_per_pass = (uint64_t) p.grid * MI355_WIDE_BLOCK;
    for (uint64_t k = 0; k * units_per_pass < p.nvec; ++k)
        for (unsigned b = 0; b < p.grid; ++b) {
            const uint64_t first = (k * p.grid + b) * MI355_WIDE_BLOCK; /* lane 0's unit */
            if (first >= p.nvec)
                break;
            uint64_t last = first + MI355_WIDE_BLOCK; /* one past lane 255's */
            if (last > p.nvec)
                last = p.nvec;
            if (first * per_lane != cursor)
                fail ("a gap or an overlap", form, fo, n, cus);
            cursor = last * per_lane;
        }
    if (cursor != p.nvec * per_lane)
        fail ("whole units not covered", form, fo, n, cus);
    /* the tail: lane g < tail of block 0 takes element nvec * per_lane + g */
    for (unsigned g = 0; g < p.tail; ++g)
        if (p.nvec * per_lane + g != cursor++)
            fail ("tail", form, fo, n, cus);
    if (cursor != n)
        fail ("[0, n) not tiled", form, fo, n, cus);
}

static void check_forms (void)
{
    /* real storage: the function only looks at addresses, the sanitizer at us */
    char *base = (char *) aligned_alloc (64, 4096);
    if (base == NULL)
        abort ();
    for (int fo = 0; fo < 2; ++fo)
        for (int dp = 0; dp < 16; dp += 2)
            for (int s0 = 0; s0 < 16; s0 += 2)
                for (int s1 = 0; s1 < 16; s1 += 2)
                    for (uint64_t n = 1; n <= 17; ++n) {
                        /* a unit is 8 elements from 16 source bytes, or (float) 4 from 8 */
                        const int unit = fo ? 4 : 8;
                        const void *srcs[2] = {base + 1024 + s0, base + 2048 + s1};
                        const int form = mi355_wide_form_of (fo, base + dp, srcs, 2, n);
                        const int want = dp != 0 || n < (uint64_t) unit ? MI355_WIDE_ELEMENT
                                         : s0 % (2 * unit) == 0 && s1 % (2 * unit) == 0 ? MI355_WIDE_VECTOR
                                                                                        : MI355_WIDE_UNALIGNED;
                        if (form != want)
                            fail ("form_of", form, fo, n, dp * 256 + s0 * 16 + s1);
                    }
    free (base);
}

int main (void)
{
    static const int cus_list[3] = {1, 64, 256};
    for (int ci = 0; ci < 3; ++ci)
        for (int fo = 0; fo < 2; ++fo)
            for (int form = MI355_WIDE_VECTOR; form <= MI355_WIDE_ELEMENT; ++form) {
                const int cus = cus_list[ci];
                /* a saturating launch's pass, as mi355_combine_wide_plan reports it */
                const uint64_t pass = mi355_wide_plan_launch (form, fo, UINT64_C (1) << 40, cus).pass;
                const uint64_t sizes[] = {0, 1, 7, 8, 9, 2047, 2048, 2049, 2055, 4099, pass - 9, pass - 8, pass - 1,
                                          pass, pass + 1, pass + 7, pass + 8, pass + 9, pass + 4099, 2 * pass - 1,
                                          2 * pass, 2 * pass + 3};
                for (size_t i = 0; i < sizeof sizes / sizeof sizes[0]; ++i)
                    check_launch (form, fo, sizes[i], cus);
            }
    check_forms ();
    printf ("%ld launches, %ld violations\n", launches, violations);
    return violations != 0;
}
