/* prefix_plan.h -- host-only arithmetic of the prefix fold (scan): which
 * prefix a member of an inscan/exscan receives, and how a prefix fold of more
 * sources than one launch takes is cut into chained launches. Plain C, no
 * HIP: reduce.c and prefix_kernels.h include it, and
 * tests/native/prefix_plan_check.cpp compiles it with g++ and the address and
 * undefined-behaviour sanitizers and enumerates it on the CPU. */
#ifndef MI355_PREFIX_PLAN_H
#define MI355_PREFIX_PLAN_H 1

#include <stddef.h>

#define MI355_PREFIX_LAUNCH_SOURCES 8 /* sources of one launch (combine_kernels.h kMaxSrc) */
#define MI355_PREFIX_E_INVAL (-1)

/* inscan / exscan (exclusive = 0 / 1) over `size` members: the sources the
 * prefix fold reads are members 0 .. scan_sources - 1, and member q receives
 * output slot scan_slot (q) of it -- the fold of sources 0 .. slot. exscan's
 * member 0 receives nothing (slot -1) and the fold of all members is not
 * computed. */
static inline int mi355_scan_sources (int exclusive, int size) { return size - (exclusive ? 1 : 0); }
static inline int mi355_scan_slot (int exclusive, int q) { return q - (exclusive ? 1 : 0); }

/* Sources that matter: one past the last non-null output (0: none). The
 * prefixes after it are nobody's, so they are not computed. */
static inline int mi355_prefix_trim (void *const *dsts, int nsrc)
{
    int used = 0;
    for (int k = 0; k < nsrc; ++k)
        if (dsts[k] != NULL)
            used = k + 1;
    return used;
}

/* One launch of a chained prefix fold: nsrc sources, dst[k] (or NULL) gets
 * the fold of src[0 .. k]. From the second launch on src[0] is the carry --
 * the last output of the launch before -- and dst[0] is NULL (that prefix is
 * stored already). `final`: the call's last launch. */
typedef struct mi355_prefix_chunk {
    int nsrc;
    int final;
    const void *src[MI355_PREFIX_LAUNCH_SOURCES];
    void *dst[MI355_PREFIX_LAUNCH_SOURCES];
} mi355_prefix_chunk;

/* Launches for nsrc sources with a non-null dsts[nsrc - 1]: the first takes
 * 8 sources, each later one the carry and 7 more. */
static inline int mi355_prefix_chunk_count (int nsrc)
{
    const int L = MI355_PREFIX_LAUNCH_SOURCES;
    return nsrc <= L ? 1 : 1 + (nsrc - L + (L - 2)) / (L - 1);
}

/* Where a launch leaves its carry when its last output slot is NULL: the
 * last later non-null output that is no source's buffer (an in-place output
 * still holds a source that a later launch reads). It is overwritten with its
 * own prefix by the launch that owns it, which reads the carry from it at
 * the same positions it stores (the kernels load a position's every source
 * before they store to it). NULL: there is none. */
static inline void *mi355_prefix_carry_buffer (void *const *dsts, const void *const *srcs, int nsrc, int slot)
{
    for (int j = nsrc - 1; j > slot; --j) {
        if (dsts[j] == NULL)
            continue;
        int is_source = 0;
        for (int k = 0; k < nsrc; ++k)
            is_source |= (const void *) dsts[j] == srcs[k];
        if (!is_source)
            return dsts[j];
    }
    return NULL;
}

/* Chunk c (0 <= c < mi355_prefix_chunk_count (nsrc)) of the fold; nsrc is
 * trimmed (dsts[nsrc - 1] != NULL). `carry_in`: what the chunk before left
 * (ignored for c = 0); *carry_out: where this chunk's last prefix is (NULL
 * for the final chunk). Returns 0, or MI355_PREFIX_E_INVAL when a NULL slot
 * at the chunk's end finds no carry buffer. */
static inline int mi355_prefix_chunk_at (void *const *dsts, const void *const *srcs, int nsrc, int c,
                                         const void *carry_in, mi355_prefix_chunk *out, void **carry_out)
{
    const int L = MI355_PREFIX_LAUNCH_SOURCES;
    const int first = c == 0 ? 0 : L + (c - 1) * (L - 1); /* first source (and output slot) that is new here */
    const int lead = c == 0 ? 0 : 1;                      /* the carry's place */
    int take = nsrc - first;
    if (take > L - lead)
        take = L - lead;
    out->nsrc = lead + take;
    out->final = first + take == nsrc;
    if (lead) {
        out->src[0] = carry_in;
        out->dst[0] = NULL;
    }
    for (int k = 0; k < take; ++k) {
        out->src[lead + k] = srcs[first + k];
        out->dst[lead + k] = dsts[first + k];
    }
    for (int k = lead + take; k < L; ++k) {
        out->src[k] = NULL;
        out->dst[k] = NULL;
    }
    *carry_out = NULL;
    if (!out->final) {
        const int slot = first + take - 1;
        void *carry = dsts[slot];
        if (carry == NULL) {
            carry = mi355_prefix_carry_buffer (dsts, srcs, nsrc, slot);
            if (carry == NULL)
                return MI355_PREFIX_E_INVAL;
            out->dst[out->nsrc - 1] = carry;
        }
        *carry_out = carry;
    }
    return 0;
}

#endif /* MI355_PREFIX_PLAN_H */
