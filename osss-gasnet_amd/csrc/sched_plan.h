/* sched_plan.h -- which schedule a reduction or scan over symmetric heap
 * offsets runs: host-only integer arithmetic on the job's settings (struct
 * sched_env) and one request (struct sched_req). No HIP, no library state, no
 * allocation: reduce.c fills the two structs, asks plan_schedule once per call
 * and executes the answer, and tests/native/sched_plan_check.c compiles this
 * header with the address and undefined-behaviour sanitizers and enumerates
 * it on the CPU (tests/test_sched_plan.py). Plain C that is also C++. */
#ifndef SHMEMI_SCHED_PLAN_H
#define SHMEMI_SCHED_PLAN_H 1

#include <stddef.h>
#include <string.h>

#include "mi355_reduce.h"
#include "shmemx.h"

/* The job's state the choice depends on (reduce.c sched_env_now). */
struct sched_env {
    int order;      /* SHMEMX_ORDER_* */
    int algorithm;  /* SHMEMX_REDUCE_* */
    size_t fused_max, oneshot_max; /* SHMEM_FUSED_MAX_BYTES, SHMEM_ONESHOT_MAX_BYTES */
    size_t order_chunk;            /* bytes of one channel's version area */
    size_t scratch_chunk;          /* bytes of one scratch buffer */
    int npes;
    int have_sigmem;   /* the signal regions exist */
    int sig_broken;    /* peers' signal-region stores failed the init self-test */
    int dev_wait_slow; /* device-side waits across PEs are time-sliced */
    int p2p_broken;    /* peer heap reads failed the init self-test */
    int persistent;    /* the persistent fused server is enabled */
    int scan_direct;   /* SHMEM_SCAN_DIRECT: every scan takes the direct schedule */
};

enum sched_coll { COLL_REDUCE, COLL_INSCAN, COLL_EXSCAN };
enum sched_entry { ENTRY_BLOCKING, ENTRY_STREAM }; /* the scans have the blocking entry only */

struct sched_req {
    enum sched_coll coll;
    enum sched_entry entry;
    int op, dtype;
    size_t es;               /* bytes per element */
    size_t dst_off, src_off; /* symmetric heap offsets */
    size_t n;
    int size, me; /* the active set's members, and this PE's index among them */
    int in_heap;  /* the offsets address the members' heaps (not buffers mapped or staged for this call) */
    int chunk;    /* one chunk of a walk through scratch C (sched_plan.via_scratch): a multi-launch schedule */
};

/* The names shmemx_last_call_info reports (sched_name). A shard schedule that
 * runs several rounds is the enumerator after its one-round form. */
enum sched_id {
    SCHED_NONE, /* an error: nothing runs */
    SCHED_BARRIER_ONLY,
    SCHED_IDENTITY,
    SCHED_PERSISTENT, /* never planned: what a servable call reports when the resident server took it */
    SCHED_FUSED_ONESHOT,
    SCHED_FUSED_TWOSHOT,
    SCHED_P2P,
    SCHED_P2P_ROUNDS,
    SCHED_P2P_HOST,
    SCHED_P2P_HOST_ROUNDS,
    SCHED_EXACT,
    SCHED_STREAM_IDENTITY,
    SCHED_STREAM_FUSED_ONESHOT,
    SCHED_STREAM_FUSED_TWOSHOT,
    SCHED_STREAM_P2P,
    SCHED_STREAM_P2P_ROUNDS,
    SCHED_SCAN_LOCAL,
    SCHED_SCAN_DIRECT,
    SCHED_SCAN_P2P,
    SCHED_SCAN_P2P_ROUNDS,
    SCHED_SCAN_P2P_HOST,
    SCHED_SCAN_P2P_HOST_ROUNDS,
    SCHED_COUNT
};

static inline const char *sched_name (enum sched_id id)
{
    static const char *const names[SCHED_COUNT] = {
        "none", "barrier-only", "identity", "persistent", "fused-oneshot", "fused-twoshot", "p2p", "p2p-rounds",
        "p2p-host", "p2p-host-rounds", "exact", "stream-identity", "stream-fused-oneshot", "stream-fused-twoshot",
        "stream-p2p", "stream-p2p-rounds", "scan-local", "scan-direct", "scan-p2p", "scan-p2p-rounds", "scan-p2p-host",
        "scan-p2p-host-rounds"};
    return names[id];
}

/* How a shard schedule's members synchronise and which two legs it runs
 * (reduce.c shard_round has the table). */
enum shard_sync { SYNC_HOST, SYNC_DEV, SYNC_STREAM };
enum shard_legs { LEGS_FOLD, LEGS_ORDERS, LEGS_PAIR, LEGS_INSCAN, LEGS_EXSCAN };

/* Where the call cannot run; reduce.c plan_fatal has the messages. */
enum sched_err {
    SCHED_OK,
    SCHED_E_ORDER_AREA,     /* the version area is too small for the set */
    SCHED_E_P2P_BROKEN,     /* peer heap reads are broken and the set has more than one member */
    SCHED_E_STREAM_MEMBERS, /* a stream call beyond MI355_FUSED_MAX_MEMBERS (or the signal region's PEs) */
    SCHED_E_STREAM_PEERS,   /* a stream call of several members without working peer memory and signals */
    SCHED_E_STREAM_OVERLAP, /* a stream call whose buffers overlap without being equal */
    SCHED_E_STREAM_ORDER    /* an order-sensitive stream set beyond MI355_ORDERS_MAX_SOURCES */
};

struct sched_plan {
    enum sched_err err;  /* not SCHED_OK: sched is SCHED_NONE */
    enum sched_id sched; /* via_scratch: what the last chunk walked reports */
    enum shard_legs legs; /* the shard schedules' (SCHED_*P2P*) */
    enum shard_sync sync;
    int ordered;  /* every member's order: the fused kernel's flag; a shard schedule's version areas are in use */
    int oneshot;  /* fused and servable calls: fold whole arrays, no gather */
    size_t round; /* shard schedules: elements per round */
    int noop;     /* nothing moves (one member, in place or an exscan) */
    int servable; /* the persistent fused server may take the call (reduce.c fused_range) */
    int receives; /* this member's target is written (not exscan's member 0) */
    /* An overlap no schedule takes: chunks of chunk_elems go through scratch C
     * and from there to the target, top down when the target lies above the
     * source (memmove order). Each chunk is a request of its own (req.chunk). */
    int via_scratch, down;
    size_t chunk_elems;
};

/* An error carries nothing else. */
static inline void plan_fail (struct sched_plan *p, enum sched_err err)
{
    memset (p, 0, sizeof *p);
    p->err = err;
}

static inline int ranges_overlap (size_t a, size_t b, size_t nbytes)
{
    return a < b + nbytes && b < a + nbytes;
}

/* Elements per shard: ceil(n / size) rounded up so every shard starts on a
 * 256-byte boundary. */
static inline size_t shard_chunk (size_t n, size_t es, int size)
{
    size_t align = es >= 256 ? 1 : 256 / es;
    size_t chunk = (n + (size_t) size - 1) / (size_t) size;
    return (chunk + align - 1) / align * align;
}

/* Shard bounds of member i for n elements of es bytes over `size` members. */
static inline void shard_bounds (size_t n, size_t es, int size, int i, size_t *lo, size_t *hi)
{
    const size_t chunk = shard_chunk (n, es, size);
    size_t l = (size_t) i * chunk;
    *lo = l < n ? l : n;
    *hi = l + chunk < n ? l + chunk : n;
}

/* ---------------------------------------------------------------------- */
/* result order (shmemx.h, SHMEMX_ORDER_REFERENCE)                          */
/* ---------------------------------------------------------------------- */
/* The reference's members disagree on this reduction: floating point (the
 * integer and bitwise operators wrap, select identical bits or are exact, so
 * any order gives the same bits), and either 3+ members (the rounding follows
 * the order), min/max (`a < b ? a : b` picks by position when a NaN or a +-0
 * pair is involved, reduce-op.c:138-150, from 2 members on), or a two-member
 * float, double or complex sum/prod: a + b and b + a have the same value, but
 * where both operands are NaNs SSE returns the FIRST one (ops.h x86_result),
 * so the two members' results differ in payload. x87 long double returns the
 * NaN with the larger significand whatever the order (x80.h), so its
 * two-member sum/prod agree. So do half's and bfloat16's (shmemx.h): a NaN
 * out of their sum or prod is the canonical one whatever the operands were. */
static inline int order_sensitive (const struct sched_env *e, int op, int dtype, int size)
{
    if (e->order != SHMEMX_ORDER_REFERENCE || size < 2)
        return 0;
    if (dtype != MI355_FLOAT && dtype != MI355_DOUBLE && dtype != MI355_LONGDOUBLE && dtype != MI355_COMPLEXF &&
        dtype != MI355_COMPLEXD && dtype != MI355_HALF && dtype != MI355_BFLOAT16)
        return 0;
    return size > 2 || op == MI355_OP_MIN || op == MI355_OP_MAX ||
           (dtype != MI355_LONGDOUBLE && dtype != MI355_HALF && dtype != MI355_BFLOAT16);
}

/* The one-launch fused kernel and the persistent server (fused.hip) have no
 * instantiations for the 16-bit float types: their calls take the
 * multi-launch schedules at every size. */
static inline int fused_dtype (int dtype)
{
    return dtype != MI355_HALF && dtype != MI355_BFLOAT16;
}

/* The shard schedules deliver every member's order up to
 * MI355_ORDERS_MAX_SOURCES members (mi355_combine_orders); larger
 * order-sensitive active sets run the EXACT schedule instead. */
static inline int ordered_pair (const struct sched_env *e, int op, int dtype, int size)
{
    return order_sensitive (e, op, dtype, size) && size <= MI355_ORDERS_MAX_SOURCES;
}

/* Two members, float or double sum/prod, each member's own order: the
 * members' results differ only where both operands are NaNs (SSE keeps the
 * first). The multi-launch schedules then skip the version areas: each owner
 * folds its shard in ITS order (own source first) and the other member
 * gathers it NaN-patched from its own source (mi355_nan_patch_copy): one
 * output per shard, one more local read in the gather. (Complex types keep
 * the version areas: the imaginary part of gcc's float complex add takes the
 * incoming operand first, and Annex G's product is not a plain pair.) */
static inline int nan_pair (const struct sched_env *e, int op, int dtype, int size)
{
    return e->order == SHMEMX_ORDER_REFERENCE && size == 2 && (dtype == MI355_FLOAT || dtype == MI355_DOUBLE) &&
           (op == MI355_OP_SUM || op == MI355_OP_PROD);
}

/* Version areas: on every PE, one per signal-region channel, (size - 1)
 * slots of one shard each; slot s of owner i holds member q's version of
 * shard i, s = q < i ? q : q - 1. Each slot starts at the target's offset
 * within 256 bytes, so the gather copies run as aligned vectors.
 * Consecutive slots are VER_STAGGER bytes further apart than a shard needs:
 * the every-member fold writes all its outputs at the same element offset,
 * and outputs a power-of-two shard size apart land in the same HBM channels
 * (tools/probes/cold_probe orders_skew2, 8 x 32 MiB double sum: 0.62 of peak from
 * HBM with 256-byte gaps, 0.68-0.70 with 4 KiB-granular ones). */
#define VER_STAGGER 4096
static inline size_t ver_slot_bytes (size_t n, size_t es, int size)
{
    const size_t b = shard_chunk (n, es, size) * es;
    return (b + 255) / 256 * 256 + 256 + VER_STAGGER;
}

/* Elements per round of an ordered shard schedule: the largest message whose
 * versions fit one channel's version area (longer messages run in rounds).
 * 0: the area is too small for the set (SCHED_E_ORDER_AREA). */
static inline size_t ordered_round_elems (const struct sched_env *e, size_t es, int size)
{
    const size_t align = es >= 256 ? 1 : 256 / es;
    const size_t per_slot = e->order_chunk / (size_t) (size - 1);
    if (per_slot < 512 + VER_STAGGER + align * es)
        return 0;
    return (per_slot - 512 - VER_STAGGER) / es / align * align * (size_t) size;
}

/* The device-flag kernels can carry this active set's synchronization. */
static inline int device_flags_ok (const struct sched_env *e, int size)
{
    return size <= MI355_FUSED_MAX_MEMBERS && e->npes <= MI355_SIG_RSDONE && e->have_sigmem && !e->sig_broken &&
           !e->dev_wait_slow;
}

/* What keeps an active set from the stream-ordered entry points, whose every
 * schedule synchronises through device flags (SCHED_OK: nothing). */
static inline enum sched_err stream_set_error (const struct sched_env *e, int size)
{
    if (size > MI355_FUSED_MAX_MEMBERS || e->npes > MI355_SIG_RSDONE)
        return SCHED_E_STREAM_MEMBERS;
    if (size > 1 && (!e->have_sigmem || e->p2p_broken || e->sig_broken))
        return SCHED_E_STREAM_PEERS;
    return SCHED_OK;
}

/* The fused one-launch schedule (fused.hip) applies: small enough, few
 * enough members, 16-byte aligned symmetric offsets, dst == src or disjoint,
 * and (ordered) the versions fit the version area. An EXACT request binds
 * the blocking calls only. */
static inline int fused_eligible (const struct sched_env *e, const struct sched_req *r)
{
    return fused_dtype (r->dtype) && r->size > 1 && r->size <= MI355_FUSED_MAX_MEMBERS &&
           r->n * r->es <= e->fused_max && e->npes <= MI355_SIG_RSDONE && e->have_sigmem &&
           ((r->dst_off | r->src_off) & 15) == 0 && r->es <= 256 &&
           (r->dst_off == r->src_off || !ranges_overlap (r->dst_off, r->src_off, r->n * r->es)) &&
           (r->entry == ENTRY_STREAM || e->algorithm != SHMEMX_REDUCE_EXACT) &&
           (!ordered_pair (e, r->op, r->dtype, r->size) ||
            (size_t) (r->size - 1) * shard_chunk (r->n, r->es, r->size) * r->es <= e->order_chunk);
}

/* One-shot: every member folds the whole arrays. Not in place: it would
 * overwrite a source that others still read. */
static inline int oneshot_fits (const struct sched_env *e, const struct sched_req *r)
{
    return r->n * r->es <= e->oneshot_max && r->dst_off != r->src_off;
}

/* A scan takes the direct schedule (reduce.c, scan): the set is too large
 * for the prefix fold's every-member outputs, or by request. */
static inline int scan_is_direct (const struct sched_env *e, int size)
{
    return size > MI355_ORDERS_MAX_SOURCES || e->scan_direct;
}

/* The persistent server may take a fused call, or a one-member copy the
 * fused kernel could run: it addresses the members' heaps. */
static inline int servable (const struct sched_env *e, const struct sched_req *r)
{
    return e->persistent && r->in_heap && !r->chunk;
}

static inline void plan_fused (const struct sched_env *e, const struct sched_req *r, struct sched_plan *p)
{
    const int stream = r->entry == ENTRY_STREAM;
    p->oneshot = oneshot_fits (e, r);
    p->ordered = ordered_pair (e, r->op, r->dtype, r->size);
    p->servable = !stream && servable (e, r);
    p->sched = stream ? (p->oneshot ? SCHED_STREAM_FUSED_ONESHOT : SCHED_STREAM_FUSED_TWOSHOT)
                      : (p->oneshot ? SCHED_FUSED_ONESHOT : SCHED_FUSED_TWOSHOT);
}

/* The multi-launch shard schedule of a reduction or scan over [0, n). */
static inline void plan_shards (const struct sched_env *e, const struct sched_req *r, struct sched_plan *p)
{
    const int scan = r->coll != COLL_REDUCE;
    const int pair = !scan && nan_pair (e, r->op, r->dtype, r->size);
    p->ordered = scan || (ordered_pair (e, r->op, r->dtype, r->size) && !pair);
    p->legs = scan   ? (r->coll == COLL_EXSCAN ? LEGS_EXSCAN : LEGS_INSCAN)
              : pair ? LEGS_PAIR
                     : p->ordered ? LEGS_ORDERS : LEGS_FOLD;
    p->sync = r->entry == ENTRY_STREAM ? SYNC_STREAM : device_flags_ok (e, r->size) ? SYNC_DEV : SYNC_HOST;
    p->round = p->ordered ? ordered_round_elems (e, r->es, r->size) : r->n;
    if (p->round == 0) {
        plan_fail (p, SCHED_E_ORDER_AREA);
        return;
    }
    const enum sched_id one = scan                    ? (p->sync == SYNC_DEV ? SCHED_SCAN_P2P : SCHED_SCAN_P2P_HOST)
                              : p->sync == SYNC_STREAM ? SCHED_STREAM_P2P
                              : p->sync == SYNC_DEV    ? SCHED_P2P
                                                       : SCHED_P2P_HOST;
    p->sched = (enum sched_id) (one + (r->n > p->round));
}

static inline struct sched_plan plan_schedule (const struct sched_env *e, const struct sched_req *r);

/* Through scratch C; the plan reports what the walk's last chunk does. */
static inline void plan_scratch (const struct sched_env *e, const struct sched_req *r, struct sched_plan *p)
{
    const size_t per = e->scratch_chunk / r->es, nchunks = (r->n + per - 1) / per;
    struct sched_req last = *r;
    last.chunk = 1;
    last.dst_off = r->src_off + r->n * r->es; /* scratch C: clear of the source */
    last.n = r->dst_off > r->src_off ? (r->n < per ? r->n : per) : r->n - (nchunks - 1) * per;
    *p = plan_schedule (e, &last);
    if (p->err != SCHED_OK)
        return;
    p->via_scratch = 1;
    p->down = r->dst_off > r->src_off;
    p->chunk_elems = per;
}

static inline struct sched_plan plan_schedule (const struct sched_env *e, const struct sched_req *r)
{
    struct sched_plan p;
    memset (&p, 0, sizeof p);
    const int stream = r->entry == ENTRY_STREAM, scan = r->coll != COLL_REDUCE, excl = r->coll == COLL_EXSCAN;
    const int same = r->dst_off == r->src_off;
    const int overlap = ranges_overlap (r->dst_off, r->src_off, r->n * r->es);
    p.receives = !(excl && r->me == 0);
    if (stream && stream_set_error (e, r->size) != SCHED_OK) {
        plan_fail (&p, stream_set_error (e, r->size));
    } else if (r->n == 0) {
        /* the reference's barriers still run (reduce-op.c:230,266), nothing else */
        p.sched = SCHED_BARRIER_ONLY;
    } else if (stream && overlap && !same) {
        plan_fail (&p, SCHED_E_STREAM_OVERLAP);
    } else if (!stream && r->size > 1 && e->p2p_broken) {
        plan_fail (&p, SCHED_E_P2P_BROKEN);
    }
    if (p.err != SCHED_OK || p.sched != SCHED_NONE)
        return p;

    if (r->size == 1) {
        /* a one-member fold is the identity: target = source (reduce-op.c:226-229) */
        p.sched = stream ? SCHED_STREAM_IDENTITY : scan ? SCHED_SCAN_LOCAL : SCHED_IDENTITY;
        p.noop = same || excl;
        if (!p.noop && overlap) {
            if (!scan && e->algorithm == SHMEMX_REDUCE_EXACT)
                p.sched = SCHED_EXACT; /* the walk's name under an EXACT request, whatever the set */
            p.via_scratch = 1;
            p.down = r->dst_off > r->src_off;
            p.chunk_elems = e->scratch_chunk / r->es;
        } else if (!p.noop && !stream && !scan && servable (e, r) && fused_dtype (r->dtype) &&
                   r->n * r->es <= e->fused_max && ((r->dst_off | r->src_off) & 15) == 0) {
            p.servable = 1;
            p.oneshot = oneshot_fits (e, r);
        }
    } else if (stream) {
        if (order_sensitive (e, r->op, r->dtype, r->size) && !ordered_pair (e, r->op, r->dtype, r->size))
            plan_fail (&p, SCHED_E_STREAM_ORDER);
        else if (fused_eligible (e, r))
            plan_fused (e, r, &p);
        else
            plan_shards (e, r, &p);
    } else if (scan) {
        /* The kernels take an output that aliases the source of its own slot
         * only: in place that is inscan's shard fold and nothing else. */
        const int direct = scan_is_direct (e, r->size);
        if (!overlap || (same && !excl && !direct)) {
            if (direct)
                p.sched = SCHED_SCAN_DIRECT;
            else
                plan_shards (e, r, &p);
        } else {
            plan_scratch (e, r, &p);
        }
    } else {
        /* EXACT by request, or for an order-sensitive set too large for the
         * shard schedules' every-order fold (ordered_pair) */
        const int exact = e->algorithm == SHMEMX_REDUCE_EXACT ||
                          (order_sensitive (e, r->op, r->dtype, r->size) && !ordered_pair (e, r->op, r->dtype, r->size));
        if (exact && !overlap)
            p.sched = SCHED_EXACT;
        else if (!exact && (same || !overlap) && !r->chunk && fused_eligible (e, r))
            plan_fused (e, r, &p);
        else if (!exact && (same || !overlap))
            plan_shards (e, r, &p);
        else
            plan_scratch (e, r, &p);
    }
    return p;
}

#endif /* SHMEMI_SCHED_PLAN_H */
