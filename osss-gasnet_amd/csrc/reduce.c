/*
 * reduce.c -- the 44 shmem_<TYPE>_<OP>_to_all collectives on MI355X.
 *
 * Reference: src/reduce/reduce-op.c. There, every PE copies its source into
 * the target (:226-229), barriers (:230), then pulls every other PE's source
 * in 64-element chunks with shmem_getmem and folds them in with one indirect
 * call per element (:232-264), barriers again (:266) and copies back from a
 * temporary if target and source overlapped (:267-275).
 *
 * Here the combine runs on the PE's GPU (combine.hip, C ABI mi355_reduce.h)
 * and the cross-PE movement is xGMI peer access to the device symmetric heap:
 *
 *   P2P (default)  split the nreduce elements into PE_size contiguous shards
 *                  (256-byte aligned); PE i folds shard i of every member's
 *                  source into its own target shard; barrier; PE i gathers
 *                  the other shards from the members' targets. Result order
 *                  (shmemx.h): where the reference's members disagree
 *                  (floating point; see ordered_pair), PE i folds shard i in
 *                  EVERY member's reference order at once -- own source first,
 *                  then the others ascending (:226-264) -- keeps its own
 *                  version and leaves member q's in slot q of its version
 *                  area, from which q gathers it: every PE ends with the
 *                  reference's result for itself. Elsewhere (and with
 *                  SHMEM_REDUCE_ORDER=pe_start) every PE gets PE_start's
 *                  result, the fold in ascending active-set order.
 *   EXACT          every PE folds the full arrays in ITS reference order
 *                  (own source first, then the others ascending): bit-identical
 *                  to the reference on every PE, at PE_size x the xGMI reads.
 *   RCCL           ncclAllReduce for the op/type pairs RCCL has, when the
 *                  active set is the whole job; P2P otherwise.
 *
 * Buffers outside the device symmetric heap (host memory from shmem_malloc,
 * static arrays, other device memory) are staged through the heap's scratch
 * area in chunks: copy in, reduce device-resident, copy out.
 *
 * Which schedule a call on symmetric heap offsets runs is decided in
 * sched_plan.h (plan_schedule: host-only, enumerated on the CPU by
 * tests/test_sched_plan.py); this file fills its request and executes its
 * plan (run_blocking, reduce_on_stream).
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355_reduce.h"
#include "pshmem.h"
#include "shmem.h"
#include "shmemx.h"
#include "shmemi.h"
#include "loc_plan.h"
#include "prefix_plan.h"
#include "sched_plan.h"

enum { SHMEMI_CHAN_HOST = 0, SHMEMI_CHAN_STREAM = 1 }; /* signal-region channels */

struct aset {
    int start, stride, size, me; /* me = index of this PE in the set */
};

static int aset_pe (const struct aset *s, int i) { return s->start + i * s->stride; }

/* The active set of an entry point's arguments, checked: inside the job, and
 * this PE a member. */
static void aset_init (const char *fn, struct aset *s, int PE_start, int logPE_stride, int PE_size)
{
    if (logPE_stride < 0 || logPE_stride > 30 || PE_size < 1 || PE_start < 0 ||
        PE_start + (long) (PE_size - 1) * (1L << logPE_stride) >= shmemi.npes)
        shmemi_fatal ("%s: active set (PE_start %d, logPE_stride %d, PE_size %d) outside the %d PEs",
                      fn, PE_start, logPE_stride, PE_size, shmemi.npes);
    s->start = PE_start;
    s->stride = 1 << logPE_stride;
    s->size = PE_size;
    s->me = -1;
    for (int i = 0; i < PE_size; ++i)
        if (aset_pe (s, i) == shmemi.mype)
            s->me = i;
    if (s->me < 0)
        shmemi_fatal ("%s: PE %d is not in the active set (PE_start %d, logPE_stride %d, PE_size %d)",
                      fn, shmemi.mype, PE_start, logPE_stride, PE_size);
}

/* What the call ran (shmemx_last_call_info): called right after the
 * dominant kernel's launch, so the combine layer's last kernel is it.
 * sources/outputs buffers of `bytes` each; extra_alg / extra_peer: bytes
 * beyond those (the fused two-shot's gather). Rounds add launches. */
static const char *cur_schedule = "none";

static void note_call (int ordered, int sources, int outputs, int peer_sources, unsigned long long bytes,
                       unsigned long long extra_alg, unsigned long long extra_peer, const void *kernel)
{
    shmemi.last.valid = 1;
    shmemi.last.schedule = cur_schedule;
    shmemi.last.kernel = kernel;
    shmemi.last.ordered = ordered;
    shmemi.last.sources = sources;
    shmemi.last.outputs = outputs;
    shmemi.last.peer_sources = peer_sources;
    shmemi.last.bytes_per_buffer = bytes;
    shmemi.last.alg_bytes = (unsigned long long) (sources + outputs) * bytes + extra_alg;
    shmemi.last.peer_bytes = (unsigned long long) peer_sources * bytes + extra_peer;
    shmemi.last.launches++;
}

static void begin_call (const char *schedule)
{
    cur_schedule = schedule;
    shmemi.last.valid = 1;
    shmemi.last.schedule = schedule;
    shmemi.last.kernel = NULL;
    shmemi.last.launches = 0;
    shmemi.last.ordered = shmemi.last.sources = shmemi.last.outputs = shmemi.last.peer_sources = 0;
    shmemi.last.bytes_per_buffer = shmemi.last.alg_bytes = shmemi.last.peer_bytes = 0;
}

int shmemx_last_call_info (shmemx_call_info *info)
{
    if (info == NULL || !shmemi.last.valid)
        return -1;
    memset (info, 0, sizeof *info);
    snprintf (info->schedule, sizeof info->schedule, "%s", shmemi.last.schedule);
    if (shmemi.last.kernel != NULL && mi355_kernel_name (shmemi.last.kernel, info->kernel, sizeof info->kernel) != 0)
        info->kernel[0] = '\0';
    info->ordered = shmemi.last.ordered;
    info->sources = shmemi.last.sources;
    info->outputs = shmemi.last.outputs;
    info->peer_sources = shmemi.last.peer_sources;
    info->launches = shmemi.last.launches;
    info->bytes_per_buffer = shmemi.last.bytes_per_buffer;
    info->alg_bytes = shmemi.last.alg_bytes;
    info->peer_bytes = shmemi.last.peer_bytes;
    return 0;
}

/* Launch the fold and wait for its completion signal (the kernel's last
 * block writes a host-coherent word; ~4 us sooner than a stream sync). */
static void combine_wait (int op, int dtype, void *dst, const void *const *srcs, int nsrc, size_t n, int timed)
{
    if (timed)
        shmemi_timed_begin ();
    shmemi_arm_signal ();
    int rc = mi355_combine (op, dtype, dst, srcs, nsrc, n, shmemi.stream);
    if (timed)
        shmemi_timed_end ();
    if (rc != 0)
        shmemi_fatal ("combine kernel launch failed (op %d, dtype %d, %d sources, %zu elements): %d",
                      op, dtype, nsrc, n, rc);
    shmemi_wait_signal ();
}

/* Byte copies, 64 segments per launch; the last launch carries the signal
 * (and, when kernel timing is on, the event pair of timing phase `phase`;
 * phase < 0: not timed). */
static void copy_wait (void *const *dsts, const void *const *srcs, const size_t *nbytes, int nseg, int phase)
{
    const int timed = phase >= 0;
    if (nseg <= 0)
        return;
    for (int base = 0; base < nseg; base += 64) {
        const int k = nseg - base < 64 ? nseg - base : 64;
        const int last = base + k == nseg;
        if (last) {
            if (timed)
                shmemi_timed_begin_phase (phase);
            shmemi_arm_signal ();
        }
        int rc = mi355_copy_segments (dsts + base, srcs + base, nbytes + base, k, shmemi.stream);
        if (last && timed)
            shmemi_timed_end ();
        if (rc != 0)
            shmemi_fatal ("copy kernel launch failed: %d", rc);
    }
    shmemi_wait_signal ();
}

void mi355_shard_bounds (size_t n, size_t es, int size, int i, size_t *lo, size_t *hi)
{
    shard_bounds (n, es, size, i, lo, hi);
}

/* ---------------------------------------------------------------------- */
/* the planner's two sides (sched_plan.h)                                  */
/* ---------------------------------------------------------------------- */
static int scan_direct_forced (void)
{
    static int forced = -1;
    if (forced < 0) {
        const char *e = getenv ("SHMEM_SCAN_DIRECT");
        forced = e != NULL && atoi (e) != 0;
    }
    return forced;
}

/* The job's state as the planner sees it. */
static struct sched_env sched_env_now (void)
{
    const struct sched_env e = {shmemi.order, shmemi.algorithm, shmemi.fused_max, shmemi.oneshot_max,
                                shmemi.order_chunk, shmemi.scratch_chunk, shmemi.npes, shmemi.sigmem != NULL,
                                shmemi.sig_broken, shmemi.dev_wait_slow, shmemi.p2p_broken, shmemi.srv.enabled,
                                scan_direct_forced ()};
    return e;
}

/* A plan's error (fn: the stream entry point, for its messages). */
static void plan_fatal (const char *fn, enum sched_err err, int scan, int size)
{
    switch (err) {
    case SCHED_OK:
        return;
    case SCHED_E_ORDER_AREA:
        shmemi_fatal ("SHMEM_DEVICE_ORDER_SIZE (%zu bytes per channel) is too small for %d PEs", shmemi.order_chunk,
                      size);
    case SCHED_E_P2P_BROKEN:
        if (scan)
            shmemi_fatal ("peer GPU memory reads failed the init self-test; the scan collectives need them");
        shmemi_fatal ("peer GPU memory reads failed the init self-test; only the RCCL pairs "
                      "(sum/prod/min/max on short/int/long/float/double, complex sum) over all PEs can run");
    case SCHED_E_STREAM_MEMBERS:
        shmemi_fatal ("%s: stream-ordered collectives take at most %d PEs per active set (of at most %d)",
                      fn, MI355_FUSED_MAX_MEMBERS, MI355_SIG_RSDONE);
    case SCHED_E_STREAM_PEERS:
        shmemi_fatal ("%s: peer GPU memory failed the init self-test", fn);
    case SCHED_E_STREAM_OVERLAP:
        shmemi_fatal ("%s: target and source overlap without being equal", fn);
    case SCHED_E_STREAM_ORDER:
        shmemi_fatal ("%s: %d PEs: the stream-ordered schedules deliver each PE's reference order up to %d "
                      "PEs (set SHMEM_REDUCE_ORDER=pe_start)", fn, size, MI355_ORDERS_MAX_SOURCES);
    }
}

/* Where member q's version of the owner's shard lies in the owner's version
 * area on channel chan (sched_plan.h, ver_slot_bytes). */
static size_t ver_off (int chan, int owner, int q, size_t slot_bytes, size_t dst_off)
{
    return shmemi.order_off + (size_t) chan * shmemi.order_chunk + (size_t) (q < owner ? q : q - 1) * slot_bytes +
           (dst_off & 255);
}

/* ---------------------------------------------------------------------- */
/* device-resident schedules on symmetric heap offsets                     */
/* ---------------------------------------------------------------------- */

/* Member list of the active set for the device-flag kernels (fused.hip), on
 * one signal-region channel. */
static void member_args (MI355FusedArgs *a, const struct aset *s, int chan)
{
    memset (a, 0, sizeof *a);
    a->nmembers = s->size;
    a->me = s->me;
    for (int i = 0; i < s->size; ++i) {
        a->pe[i] = aset_pe (s, i);
        a->sig[i] = shmemi.peer_sig[a->pe[i]] + (size_t) chan * MI355_SIG_CHANNEL_WORDS;
    }
    a->err_flag = shmemi.stream_err;
    a->timeout_ticks = (unsigned long long) (shmemi.barrier_timeout * 1e8);
    a->share = shmemi.local_pes;
    a->no_acquire = shmemi.fused_no_acquire;
}

static void device_barrier (const MI355FusedArgs *a, hipStream_t st)
{
    shmemi_server_stop (); /* two spin-waiting grids need not fit beside each other */
    const int rc = mi355_device_barrier (a, st);
    if (rc != 0)
        shmemi_fatal ("device barrier launch failed: %d", rc);
}

/* For coll.c: the member list of an active set on the host channel. */
void shmemi_member_args (MI355FusedArgs *a, int PE_start, int stride, int PE_size, int me)
{
    struct aset s = {PE_start, stride, PE_size, me};
    member_args (a, &s, SHMEMI_CHAN_HOST);
}

/* For coll.c: a device barrier over an active set on the library stream
 * (host channel); `last` makes it carry the completion flag and waits. */
int shmemi_dev_barrier_ok (int PE_start, int stride, int PE_size)
{
    const struct sched_env e = sched_env_now ();
    return device_flags_ok (&e, PE_size);
}

void shmemi_dev_barrier (int PE_start, int stride, int PE_size, int me, int last)
{
    struct aset s = {PE_start, stride, PE_size, me};
    MI355FusedArgs a;
    member_args (&a, &s, SHMEMI_CHAN_HOST);
    if (last) {
        a.host_flag = shmemi.sig_flag;
        a.epoch = shmemi_next_epoch ();
    }
    device_barrier (&a, shmemi.stream);
    if (last && shmemi_wait_flag (a.epoch) != a.epoch)
        shmemi_fatal ("device barrier timed out waiting for the other PEs of the active set");
}

/* nan_pair's NaN word can carry the owner's "no NaN" to the other member:
 * the owner's signal region is mapped there and peers' stores into signal
 * regions were seen at init (without that, sig_broken: host barriers, and the
 * gather patches unconditionally). */
static int nan_word_ok (const struct aset *s)
{
    const int other_pe = aset_pe (s, 1 - s->me);
    return !shmemi.sig_broken && shmemi.sigmem != NULL && shmemi.peer_sig[other_pe] != NULL;
}

/* nan_pair: this call's number among the two-member calls with the other
 * member on channel chan -- the same on both members (every member makes the
 * same collective calls) -- whose parity picks the NaN word the owner's fold
 * sets (MI355_SIG_NANFLAG_AT; it clears the other parity's, which the previous
 * call's gather has finished reading) and the other member's gather reads. */
static long long pair_next (int chan, const struct aset *s)
{
    if (shmemi.pair_calls == NULL) {
        shmemi.pair_calls = (uint64_t *) calloc ((size_t) MI355_SIG_CHANNELS * (size_t) shmemi.npes, sizeof (uint64_t));
        if (shmemi.pair_calls == NULL)
            shmemi_fatal ("out of host memory");
    }
    return (long long) ++shmemi.pair_calls[(size_t) chan * (size_t) shmemi.npes + (size_t) aset_pe (s, 1 - s->me)];
}

/* The reduce-scatter leg: fold this PE's shard of every member's source
 * into its target shard -- in member order, or (ordered) in every member's
 * reference order with the other members' versions going to this PE's
 * version area on channel `chan`. Returns the launch's status (0: queued, or
 * nothing to do: empty shard). */
static int fold_shard (int op, int dtype, size_t es, size_t dst_off, size_t src_off, size_t n, const struct aset *s,
                       int ordered, long long pair_k, int chan, hipStream_t st)
{
    const int pair = pair_k >= 0;
    const void *sp[MI355_FUSED_MAX_MEMBERS > MI355_ORDERS_MAX_SOURCES ? MI355_FUSED_MAX_MEMBERS
                                                                       : MI355_ORDERS_MAX_SOURCES];
    size_t lo, hi;
    mi355_shard_bounds (n, es, s->size, s->me, &lo, &hi);
    if (hi <= lo) {
        /* no fold: clear the word the next call's fold would have (this
         * call's stays as the previous call of its parity left it, but the
         * other member's gather of an empty shard reads nothing) */
        if (pair && nan_word_ok (s)) {
            const int other = aset_pe (s, 1 - s->me);
            const hipError_t e = hipMemsetAsync (shmemi.sigmem + MI355_SIG_NANFLAG_AT (chan, (pair_k + 1) & 1, other),
                                                 0, sizeof (unsigned long long), st);
            if (e != hipSuccess)
                return (int) e;
        }
        return 0;
    }
    const void **spp = sp;
    if (s->size > (int) (sizeof sp / sizeof sp[0])) {
        spp = (const void **) malloc (sizeof (void *) * (size_t) s->size);
        if (spp == NULL)
            shmemi_fatal ("out of host memory");
    }
    for (int i = 0; i < s->size; ++i)
        spp[i] = shmemi_peer_ptr (aset_pe (s, i), src_off + lo * es);
    if (pair && s->me == 1) { /* nan_pair: this owner's order, its own source first */
        const void *t = spp[0];
        spp[0] = spp[1];
        spp[1] = t;
    }
    void *dst = shmemi_peer_ptr (shmemi.mype, dst_off + lo * es);
    int rc;
    if (pair && nan_word_ok (s)) {
        const int other = aset_pe (s, 1 - s->me);
        mi355_nan_flag_next_launch (shmemi.sigmem + MI355_SIG_NANFLAG_AT (chan, pair_k & 1, other),
                                    shmemi.sigmem + MI355_SIG_NANFLAG_AT (chan, (pair_k + 1) & 1, other));
    }
    if (!ordered) {
        rc = mi355_combine (op, dtype, dst, spp, s->size, hi - lo, st);
    } else {
        void *dsts[MI355_ORDERS_MAX_SOURCES];
        const size_t slot = ver_slot_bytes (n, es, s->size);
        for (int q = 0; q < s->size; ++q)
            dsts[q] = q == s->me ? dst : shmemi_peer_ptr (shmemi.mype, ver_off (chan, s->me, q, slot, dst_off));
        rc = mi355_combine_orders (op, dtype, dsts, spp, s->size, hi - lo, st);
    }
    if (rc == 0)
        note_call (ordered, s->size, ordered ? s->size : 1, s->size - 1, (unsigned long long) ((hi - lo) * es), 0, 0,
                   mi355_last_kernel ());
    if (spp != sp)
        free (spp);
    return rc;
}

/* The all-gather leg's segments: the other members' shards, from their
 * targets, or (ordered) this PE's version of them from their version areas.
 * Returns the number of segments (arrays of s->size entries). */
static int gather_segments (size_t es, size_t dst_off, size_t n, const struct aset *s, int ordered, int chan,
                            void **dsts, const void **sp, size_t *nb)
{
    const size_t slot = ver_slot_bytes (n, es, s->size);
    int k = 0;
    for (int i = 0; i < s->size; ++i) {
        size_t l, h;
        mi355_shard_bounds (n, es, s->size, i, &l, &h);
        if (i == s->me || h <= l)
            continue;
        dsts[k] = shmemi_peer_ptr (shmemi.mype, dst_off + l * es);
        sp[k] = ordered ? shmemi_peer_ptr (aset_pe (s, i), ver_off (chan, i, s->me, slot, dst_off))
                        : shmemi_peer_ptr (aset_pe (s, i), dst_off + l * es);
        nb[k] = (h - l) * es;
        ++k;
    }
    return k;
}

/* nan_pair's gather: the other member's shard from its target, where this
 * PE's own source is a NaN that NaN quieted instead. 0: queued, or nothing to
 * do (an empty shard: fires an armed signal). */
static int pair_gather (int dtype, size_t es, size_t dst_off, size_t src_off, size_t n, const struct aset *s,
                        long long pair_k, int chan, hipStream_t st)
{
    const int other = 1 - s->me, other_pe = aset_pe (s, other);
    size_t l, h;
    mi355_shard_bounds (n, es, 2, other, &l, &h);
    return mi355_nan_patch_copy (dtype, shmemi_peer_ptr (shmemi.mype, dst_off + l * es),
                                 shmemi_peer_ptr (other_pe, dst_off + l * es),
                                 shmemi_peer_ptr (shmemi.mype, src_off + l * es), h > l ? h - l : 0,
                                 nan_word_ok (s) ? shmemi.peer_sig[other_pe] +
                                                       MI355_SIG_NANFLAG_AT (chan, pair_k & 1, shmemi.mype)
                                                 : NULL, /* no word: always patch */
                                 st);
}

/* Before a host barrier lets peers read this PE's caller-written buffers,
 * the host must know the caller's queued work is done (one signal kernel,
 * shmemi_order_after_caller). Set per call by entry_prologue; the device-flag
 * schedules never need it. */
static int caller_order_pending;

static void host_order (void)
{
    if (caller_order_pending) {
        shmemi_order_after_caller (1);
        caller_order_pending = 0;
    }
}

static void stream_barrier (const char *fn, const struct aset *s, hipStream_t st)
{
    if (s->size < 2)
        return;
    MI355FusedArgs a;
    member_args (&a, s, SHMEMI_CHAN_STREAM);
    const int rc = mi355_device_barrier (&a, st);
    if (rc != 0)
        shmemi_fatal ("%s: device barrier launch failed: %d", fn, rc);
}

static void stream_copy (const char *fn, void *const *dsts, const void *const *srcs, const size_t *nb, int k,
                         hipStream_t st)
{
    for (int base = 0; base < k; base += 64) {
        const int m = k - base < 64 ? k - base : 64;
        const int rc = mi355_copy_segments (dsts + base, srcs + base, nb + base, m, st);
        if (rc != 0)
            shmemi_fatal ("%s: copy kernel launch failed: %d", fn, rc);
    }
}

/* ---------------------------------------------------------------------- */
/* the multi-launch P2P shard schedule               */
/* ---------------------------------------------------------------------- */
/* One round: barrier (every source is ready), the owner's leg on this PE's
 * shard, barrier (every shard is written), the gather leg, barrier (peers
 * are done reading this PE). A call picks how the members synchronise and
 * which two legs run; the two are independent.
 *
 *   sync         barrier                       a leg is              timed  channel
 *   SYNC_HOST    shmemi_barrier_set            signalled and waited  yes    host
 *   SYNC_DEV     one-block kernel on the       queued; the third     yes    host
 *                library stream                barrier's flag is the
 *                                              call's one host wait
 *   SYNC_STREAM  one-block kernel on the       queued; no host wait  no     stream
 *                caller's stream               at all (graph capture)
 *
 *   legs         owner's leg                              gather leg
 *   LEGS_FOLD    fold_shard, member order                 segments from the members' targets
 *   LEGS_ORDERS  fold_shard, every member's order         segments from their version areas
 *   LEGS_PAIR    fold_shard, this owner's order           pair_gather (NaN-patched)
 *   LEGS_INSCAN  scan_fold_shard                          segments from their version areas
 *   LEGS_EXSCAN  scan_fold_shard                          the same; member 0 gathers nothing */
struct shard_call {
    int op, dtype;
    size_t es;
    const struct aset *s;
    enum shard_legs legs;
    enum shard_sync sync;
    hipStream_t st; /* the library stream, or SYNC_STREAM's */
    const char *fn; /* SYNC_STREAM: the entry point, for its messages */
};

static int scan_fold_shard (int op, int dtype, size_t es, size_t dst_off, size_t src_off, size_t n,
                            const struct aset *s, int excl, int chan, hipStream_t st);

/* `last`: SYNC_DEV's barrier carries the completion flag and waits for it */
static void shard_barrier (const struct shard_call *c, int last)
{
    const struct aset *s = c->s;
    if (c->sync == SYNC_HOST)
        shmemi_barrier_set (s->start, s->stride, s->size);
    else if (c->sync == SYNC_DEV)
        shmemi_dev_barrier (s->start, s->stride, s->size, s->me, last);
    else
        stream_barrier (c->fn, s, c->st);
}

static void shard_round (const struct shard_call *c, size_t dst_off, size_t src_off, size_t n)
{
    const struct aset *s = c->s;
    const int host = c->sync == SYNC_HOST, dev = c->sync == SYNC_DEV;
    const int chan = c->sync == SYNC_STREAM ? SHMEMI_CHAN_STREAM : SHMEMI_CHAN_HOST;
    const int pair = c->legs == LEGS_PAIR, scan = c->legs >= LEGS_INSCAN, excl = c->legs == LEGS_EXSCAN;
    const size_t m = (size_t) s->size; /* sets above MI355_FUSED_MAX_MEMBERS reach SYNC_HOST */
    void **dsts = (void **) malloc (m * (2 * sizeof (void *) + sizeof (size_t)));
    if (dsts == NULL)
        shmemi_fatal ("out of host memory");
    const void **sp = (const void **) (dsts + m);
    size_t *nb = (size_t *) (sp + m);
    size_t lo, hi;
    mi355_shard_bounds (n, c->es, s->size, s->me, &lo, &hi);

    const long long pk = pair ? pair_next (chan, s) : -1;
    if (host)
        host_order ();
    shard_barrier (c, 0); /* every source is ready; on the device, stream-ordered after the caller's work */

    /* SYNC_HOST launches for a non-empty shard only -- but a pair's empty
     * shard still clears the next call's NaN word (fold_shard), unsignalled */
    const int queued = !host || hi > lo;
    if (queued || pair) {
        if (queued)
            shmemi_peer_acquire (c->st);
        if (queued && c->sync != SYNC_STREAM)
            shmemi_timed_begin ();
        if (queued && host)
            shmemi_arm_signal ();
        const int rc = scan ? scan_fold_shard (c->op, c->dtype, c->es, dst_off, src_off, n, s, excl, chan, c->st)
                            : fold_shard (c->op, c->dtype, c->es, dst_off, src_off, n, s, c->legs == LEGS_ORDERS, pk,
                                          chan, c->st);
        if (queued && c->sync != SYNC_STREAM)
            shmemi_timed_end ();
        if (rc != 0 && c->fn != NULL)
            shmemi_fatal ("%s: combine kernel launch failed: %d", c->fn, rc);
        if (rc != 0 && !queued)
            shmemi_fatal ("NaN word clear failed: %d", rc);
        if (rc != 0)
            shmemi_fatal (scan ? "prefix kernel launch failed (op %d, dtype %d, %d members, %zu elements): %d"
                               : "combine kernel launch failed (op %d, dtype %d, %d sources, %zu elements): %d",
                          c->op, c->dtype, s->size, n, rc);
        if (queued && host)
            shmemi_wait_signal ();
    }
    shard_barrier (c, 0); /* every shard is reduced */
    shmemi_peer_acquire (c->st);

    if (pair) {
        if (host)
            shmemi_arm_signal ();
        if (dev)
            shmemi_timed_begin_phase (1);
        const int rc = pair_gather (c->dtype, c->es, dst_off, src_off, n, s, pk, chan, c->st);
        if (dev)
            shmemi_timed_end ();
        if (rc != 0 && c->fn != NULL)
            shmemi_fatal ("%s: gather kernel launch failed", c->fn);
        if (rc != 0)
            shmemi_fatal ("gather kernel launch failed: %d", rc);
        if (host)
            shmemi_wait_signal ();
    } else {
        /* exscan's member 0 gathers nothing: its target stays as it was */
        const int k = excl && s->me == 0 ? 0
                                         : gather_segments (c->es, dst_off, n, s, c->legs != LEGS_FOLD, chan, dsts,
                                                            sp, nb);
        if (host) {
            copy_wait (dsts, sp, nb, k, 1);
        } else if (c->sync == SYNC_STREAM) {
            stream_copy (c->fn, dsts, sp, nb, k, c->st);
        } else if (k > 0) { /* at most MI355_FUSED_MAX_MEMBERS segments: one launch */
            shmemi_timed_begin_phase (1);
            const int rc = mi355_copy_segments (dsts, sp, nb, k, c->st);
            shmemi_timed_end ();
            if (rc != 0)
                shmemi_fatal ("copy kernel launch failed: %d", rc);
        }
    }
    shard_barrier (c, 1); /* peers are done reading this target and version area: the call is over */
    free (dsts);
}

/* [0, n) in rounds of at most `round` elements, each a complete schedule
 * (several when the versions outgrow the version area). */
static void shard_rounds (const struct shard_call *c, size_t dst_off, size_t src_off, size_t n, size_t round)
{
    size_t b = 0;
    do {
        const size_t cn = n - b < round ? n - b : round;
        shard_round (c, dst_off + b * c->es, src_off + b * c->es, cn);
        b += cn;
    } while (b < n);
}

/* A plan's shard schedule over [0, n), on the library stream or (SYNC_STREAM,
 * with the entry point's name) the caller's. */
static void run_shards (const struct sched_plan *p, const struct sched_req *r, const struct aset *s, hipStream_t st,
                        const char *fn)
{
    begin_call (sched_name (p->sched));
    const struct shard_call c = {r->op, r->dtype, r->es, s, p->legs, p->sync, st, fn};
    shard_rounds (&c, r->dst_off, r->src_off, r->n, p->round);
}

/* The fused kernel's arguments for n elements at the members' symmetric
 * offsets on channel `chan`. Ordered two-shot calls read and write the
 * members' version areas of that channel (mi355_reduce.h). */
static void fused_args (MI355FusedArgs *a, int op, int dtype, size_t es, size_t dst_off, size_t src_off, size_t n,
                        int ordered, int oneshot, const struct aset *s, int chan)
{
    member_args (a, s, chan);
    a->op = op;
    a->dtype = dtype;
    a->n = n;
    a->shard = shard_chunk (n, es, s->size);
    a->oneshot = oneshot;
    a->ordered = ordered;
    for (int i = 0; i < s->size; ++i) {
        a->src[i] = shmemi_peer_ptr (a->pe[i], src_off);
        a->dst[i] = shmemi_peer_ptr (a->pe[i], dst_off);
        if (ordered && !oneshot)
            a->ver[i] = shmemi_peer_ptr (a->pe[i], shmemi.order_off + (size_t) chan * shmemi.order_chunk);
    }
}

/* The fused kernel's bytes: one-shot = every member's whole source read
 * (N - 1 of them from peers), one output; two-shot = the shard of every
 * member folded into 1 (or, ordered, N) outputs, then the other N - 1 shards
 * gathered from peers and written here. A one-member "fused" call is the
 * persistent server's identity copy. */
static void note_fused (int size, int ordered, int oneshot, size_t n, size_t es, const void *kernel)
{
    if (size == 1) {
        note_call (0, 1, 1, 0, (unsigned long long) (n * es), 0, 0, kernel);
        return;
    }
    if (oneshot) {
        note_call (ordered, size, 1, size - 1, (unsigned long long) (n * es), 0, 0, kernel);
        return;
    }
    const unsigned long long shard = (unsigned long long) (shard_chunk (n, es, size) * es);
    note_call (ordered, size, ordered ? size : 1, size - 1, shard, 2ull * (unsigned long long) (size - 1) * shard,
               (unsigned long long) (size - 1) * shard, kernel);
}

/* ---------------------------------------------------------------------- */
/* persistent fused server (opt-in: SHMEM_PERSISTENT=1, shmemx_set_persistent) */
/* ---------------------------------------------------------------------- */
/* A blocking call pays a launch and its dispatch (~6 us, profiles/r02/
 * kernarg_probe.txt) before the first block runs. When fused calls of one
 * (op, dtype, active set) come back to back (the second within
 * SHMEM_PERSISTENT_IDLE_US of the first), the fused kernel is left resident
 * on a stream of its own (mi355_fused_server): a call then writes its
 * offsets, sizes and epoch into the mailbox and waits for the epoch as
 * usual. The server leaves after SHMEM_PERSISTENT_IDLE_US without a call, or
 * when any other GPU operation of the library needs the device (device
 * barriers, other fused or pull kernels, RCCL, stream-ordered calls,
 * shmemx_device_synchronize, host heap changes, finalize). Not ordered after
 * the caller's queued GPU work: the caller's writes to the source must be
 * complete (synchronized) before the call -- hence opt-in. */
static int server_matches (int op, int dtype, int ordered, const struct aset *s)
{
    return shmemi.srv.running && shmemi.srv.op == op && shmemi.srv.dtype == dtype && shmemi.srv.start == s->start &&
           shmemi.srv.stride == s->stride && shmemi.srv.size == s->size && shmemi.srv.ordered == ordered;
}

/* The server has left (EXITED): later servers start past its last seq. */
static void server_gone (void)
{
    const unsigned after = shmemi.srv.mb->state_seq + 1;
    if ((int) (after - shmemi.srv.seq) > 0)
        shmemi.srv.seq = after;
    shmemi.srv.running = 0;
    SHMEMI_HIP (hipStreamSynchronize (shmemi.srv.st)); /* the grid has drained */
}

static void server_wait_exited (void)
{
    const double t0 = shmemi_now ();
    unsigned spins = 0;
    while (__atomic_load_n (&shmemi.srv.mb->state, __ATOMIC_ACQUIRE) != MI355_SERVER_EXITED) {
        __builtin_ia32_pause ();
        if ((++spins & 1023u) == 0) {
            const hipError_t e = hipStreamQuery (shmemi.srv.st);
            if (e != hipSuccess && e != hipErrorNotReady)
                shmemi_fatal ("persistent fused server failed: %s", hipGetErrorString (e));
            if (shmemi_now () - t0 > shmemi.barrier_timeout)
                shmemi_fatal ("persistent fused server did not exit within %.0f s", shmemi.barrier_timeout);
        }
    }
}

void shmemi_server_stop (void)
{
    if (!shmemi.srv.running)
        return;
    MI355ServerMailbox *mb = shmemi.srv.mb;
    if (__atomic_load_n (&mb->state, __ATOMIC_ACQUIRE) != MI355_SERVER_EXITED) {
        mb->cmd = MI355_SERVER_QUIT;
        const unsigned seq = shmemi.srv.seq++;
        mb->check = mi355_mailbox_check (mb, seq);
        __atomic_store_n (&mb->seq_head, seq, __ATOMIC_RELEASE);
        __atomic_store_n (&mb->seq_tail, seq, __ATOMIC_RELEASE);
        server_wait_exited ();
    }
    server_gone ();
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "persistent fused server stopped");
}

/* Serve one call; 0 when the server had already left (the caller launches). */
static int server_call (size_t dst_off, size_t src_off, size_t n, size_t shard, int oneshot)
{
    MI355ServerMailbox *mb = shmemi.srv.mb;
    const unsigned epoch = shmemi_next_epoch ();
    mb->src_off = src_off;
    mb->dst_off = dst_off;
    mb->n = n;
    mb->shard = shard;
    mb->epoch = epoch;
    mb->oneshot = oneshot;
    mb->cmd = MI355_SERVER_RUN;
    const unsigned seq = shmemi.srv.seq++;
    mb->check = mi355_mailbox_check (mb, seq);
    __atomic_store_n (&mb->seq_head, seq, __ATOMIC_RELEASE);
    __atomic_store_n (&mb->seq_tail, seq, __ATOMIC_RELEASE);
    const double t0 = shmemi_now ();
    unsigned spins = 0;
    for (;;) {
        const unsigned v = __atomic_load_n (shmemi.sig_flag, __ATOMIC_ACQUIRE);
        if ((v & 0x7fffffffu) == epoch) {
            if (v & 0x80000000u)
                shmemi_fatal ("fused reduction timed out waiting for the other PEs of the active set");
            ++shmemi.srv.served;
            return 1;
        }
        if (__atomic_load_n (&mb->state, __ATOMIC_ACQUIRE) == MI355_SERVER_EXITED) {
            /* it left without taking this call (idle): the flag cannot come */
            if ((__atomic_load_n (shmemi.sig_flag, __ATOMIC_ACQUIRE) & 0x7fffffffu) == epoch)
                continue;
            server_gone ();
            return 0;
        }
        __builtin_ia32_pause ();
        if ((++spins & 1023u) == 0) {
            const hipError_t e = hipStreamQuery (shmemi.srv.st);
            if (e != hipSuccess && e != hipErrorNotReady)
                shmemi_fatal ("persistent fused server failed: %s", hipGetErrorString (e));
            if (shmemi_now () - t0 > shmemi.barrier_timeout)
                shmemi_fatal ("persistent fused server: call not completed within %.0f s", shmemi.barrier_timeout);
        }
    }
}

static void server_start (int op, int dtype, size_t es, size_t n, int ordered, int oneshot, const struct aset *s)
{
    /* the members' heaps and version areas; offsets, sizes and the one-shot flag come by mailbox */
    MI355FusedArgs a;
    fused_args (&a, op, dtype, es, 0, 0, 0, ordered, 0, s, SHMEMI_CHAN_HOST);
    a.host_flag = shmemi.sig_flag;
    MI355ServerMailbox *mb = shmemi.srv.mb;
    mb->state = MI355_SERVER_RUNNING;
    mb->state_seq = 0;
    /* the grid of this call's launch (mi355_fused_allreduce) */
    const unsigned long long vecs = oneshot || s->size == 1 ? (n * es + 15) / 16
                                                            : shard_chunk (n, es, s->size) * es / 16 * (s->size - 1);
    shmemi_lazy_stream (&shmemi.srv.st, hipStreamNonBlocking);
    const int rc = mi355_fused_server (&a, mb, shmemi.srv.seq, (unsigned long long) (shmemi.srv.idle_s * 1e8), vecs,
                                       shmemi.srv.st);
    if (rc != 0) {
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "persistent fused server not started: %d", rc);
        return;
    }
    shmemi.srv.running = 1;
    shmemi.srv.op = op;
    shmemi.srv.dtype = dtype;
    shmemi.srv.start = s->start;
    shmemi.srv.stride = s->stride;
    shmemi.srv.size = s->size;
    shmemi.srv.ordered = a.ordered;
    shmemi.srv.kernel = mi355_last_kernel ();
    shmemi.srv.grid_elems = n;
    ++shmemi.srv.launched;
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "persistent fused server started (%d members, sized for %zu elements)",
                  s->size, n);
}

static void copy_local (size_t dst_off, size_t src_off, size_t nbytes, int timed);

/* One launch of the fused kernel over the members' buffers, waited for. */
static void fused_launch (const struct sched_plan *p, const struct sched_req *r, const struct aset *s,
                          const void *host_src, void *host_dst)
{
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: fused one-launch P2P, %s, %s (%zu elements, %d members)%s",
                  p->oneshot ? "one-shot" : "reduce-scatter + all-gather",
                  p->ordered ? "every member's reference order" : "PE_start order", r->n, s->size,
                  host_src != NULL ? ", staging host buffers in-kernel" : "");
    MI355FusedArgs a;
    fused_args (&a, r->op, r->dtype, r->es, r->dst_off, r->src_off, r->n, p->ordered, p->oneshot, s, SHMEMI_CHAN_HOST);
    a.host_flag = shmemi.sig_flag;
    a.epoch = shmemi_next_epoch ();
    a.host_src = host_src;
    a.host_dst = host_dst;
    shmemi_timed_begin (); /* the call's one (dominant) kernel */
    const int rc = mi355_fused_allreduce (&a, shmemi.stream);
    shmemi_timed_end ();
    if (rc != 0)
        shmemi_fatal ("fused reduction launch failed (op %d, dtype %d, %d PEs, %zu elements): %d", r->op, r->dtype,
                      s->size, r->n, rc);
    begin_call (sched_name (p->sched));
    note_fused (s->size, a.ordered, a.oneshot, r->n, r->es, mi355_last_kernel ());
    if (shmemi_wait_flag (a.epoch) != a.epoch)
        shmemi_fatal ("fused reduction timed out waiting for the other PEs of the active set");
}

static void identity_copy (const struct sched_req *r)
{
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: 1-PE identity, one copy of %zu bytes", r->n * r->es);
    begin_call (sched_name (SCHED_IDENTITY));
    copy_local (r->dst_off, r->src_off, r->n * r->es, 1);
}

/* A fused plan, or the one-member copy of a servable one: by the persistent
 * server where the plan allows it and the server matches, else launched.
 * host_src/host_dst: device-accessible page-locked host buffers of this PE
 * staged in-kernel into src_off / out of dst_off (mi355_reduce.h), or NULL. */
static void fused_range (const struct sched_plan *p, const struct sched_req *r, const struct aset *s,
                         const void *host_src, void *host_dst)
{
    const size_t n = r->n;
    const double t_call = p->servable ? shmemi_now () : 0.0;
    if (p->servable && server_matches (r->op, r->dtype, p->ordered, s) && n <= 2 * shmemi.srv.grid_elems) {
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: persistent fused server (%zu elements, %d members)", n, s->size);
        if (server_call (r->dst_off, r->src_off, n, shard_chunk (n, r->es, s->size), p->oneshot)) {
            shmemi.srv.last_end = shmemi_now ();
            begin_call (sched_name (SCHED_PERSISTENT));
            note_fused (s->size, shmemi.srv.ordered, p->oneshot, n, r->es, shmemi.srv.kernel);
            return;
        }
    }
    shmemi_server_stop (); /* a different call: the launched grid must fit */
    if (s->size == 1)
        identity_copy (r);
    else
        fused_launch (p, r, s, host_src, host_dst);
    if (p->servable) {
        /* the second call of a burst leaves the kernel resident for the next */
        if (shmemi.srv.last_end >= 0.0 && t_call - shmemi.srv.last_end < shmemi.srv.idle_s)
            server_start (r->op, r->dtype, r->es, n, p->ordered, p->oneshot, s);
        shmemi.srv.last_end = shmemi_now ();
    }
}

/* EXACT: fold everything in this PE's reference order into dst; dst must
 * not overlap any source (callers route overlaps through scratch). */
static void exact_into (int op, int dtype, size_t dst_off, size_t src_off, size_t n, const struct aset *s)
{
    const void **sp = (const void **) malloc (sizeof (void *) * (size_t) s->size);
    if (sp == NULL)
        shmemi_fatal ("out of host memory");
    shmemi_peer_acquire (shmemi.stream);
    sp[0] = shmemi_peer_ptr (shmemi.mype, src_off);
    int k = 1;
    for (int i = 0; i < s->size; ++i)
        if (i != s->me)
            sp[k++] = shmemi_peer_ptr (aset_pe (s, i), src_off);
    combine_wait (op, dtype, shmemi_peer_ptr (shmemi.mype, dst_off), sp, s->size, n, 1);
    note_call (1, s->size, 1, s->size - 1, (unsigned long long) (n * mi355_dtype_size (dtype)), 0, 0,
               mi355_last_kernel ());
    free (sp);
}

/* timed: the copy is the call's dominant kernel (the PE_size == 1 identity) */
static void copy_local (size_t dst_off, size_t src_off, size_t nbytes, int timed)
{
    void *d = shmemi_peer_ptr (shmemi.mype, dst_off);
    const void *sv = shmemi_peer_ptr (shmemi.mype, src_off);
    size_t nb = nbytes;
    copy_wait (&d, &sv, &nb, 1, timed ? 0 : -1);
    if (timed)
        note_call (0, 1, 1, 0, (unsigned long long) nbytes, 0, 0, mi355_last_kernel ());
}

/* One blocking request at symmetric offsets: planned, traced, executed. */
static void run_blocking (const struct sched_req *r, const struct aset *s);

static struct sched_req blocking_req (enum sched_coll coll, int op, int dtype, size_t es, size_t dst_off,
                                      size_t src_off, size_t n, const struct aset *s)
{
    const struct sched_req r = {coll, ENTRY_BLOCKING, op, dtype, es, dst_off, src_off, n, s->size, s->me,
                                dst_off < SHMEMI_EXT_TARGET && src_off < SHMEMI_EXT_TARGET, 0};
    return r;
}

/* Reduce n elements at symmetric offsets. */
static void reduce_symmetric (int op, int dtype, size_t es, size_t dst_off, size_t src_off, size_t n,
                              const struct aset *s)
{
    const struct sched_req r = blocking_req (COLL_REDUCE, op, dtype, es, dst_off, src_off, n, s);
    run_blocking (&r, s);
}

/* ---------------------------------------------------------------------- */
/* RCCL                                                                    */
/* ---------------------------------------------------------------------- */
int shmemi_rccl_allreduce (int op, int dtype, const void *src, void *dst, size_t n);
int shmemi_rccl_supported (int op, int dtype);

/* ---------------------------------------------------------------------- */
/* entry                                                                   */
/* ---------------------------------------------------------------------- */
enum { PK_HOST = SHMEMI_PK_HOST, PK_DEV_SYM = SHMEMI_PK_DEV_SYM, PK_DEV_OTHER = SHMEMI_PK_DEV_OTHER };

static int ptr_kind (const void *p, size_t nbytes)
{
    if (shmemi_in_device_heap (p, nbytes))
        return PK_DEV_SYM;
    hipPointerAttribute_t a;
    memset (&a, 0, sizeof a);
    hipError_t e = hipPointerGetAttributes (&a, p);
    (void) hipGetLastError ();
    if (e == hipSuccess && (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged))
        return PK_DEV_OTHER;
    return PK_HOST;
}

/* Buffers outside the device heap: stream them through scratch in chunks,
 * double-buffered so the copy-in of chunk k+1 (stream in) and the copy-out of
 * chunk k-1 (stream out) run while chunk k is reduced: with host buffers the
 * two PCIe directions then work at the same time.
 *   A0/A1 = halves of scratch A (sources), B0/B1 = halves of scratch B (results)
 * PE_size == 1 is the identity: each chunk goes in to A and straight back out.
 * A target that overlaps the source from above is walked top down (memmove
 * order, like the reference's temporary target, reduce-op.c:174-215): the
 * copy-out of a chunk then only writes source bytes already copied in, while
 * the copy-in of the next chunk (below) runs beside it. */
static void staged (int op, int dtype, const char *fn, void *target, const void *source, size_t n,
                    const struct aset *s, int ks, int kt, int use_rccl)
{
    const size_t es = mi355_dtype_size (dtype);
    shmemi_lazy_stream (&shmemi.stream_in, hipStreamDefault);
    shmemi_lazy_stream (&shmemi.stream_out, hipStreamDefault);
    const size_t half = shmemi.scratch_chunk / 2 / SHMEMI_ALIGN * SHMEMI_ALIGN;
    const size_t per = half / es;
    const size_t nchunks = (n + per - 1) / per;
    const size_t a_off[2] = {shmemi.scratch_off, shmemi.scratch_off + half};
    const size_t b_off[2] = {shmemi.scratch_off + shmemi.scratch_chunk,
                             shmemi.scratch_off + shmemi.scratch_chunk + half};
    const hipMemcpyKind in_kind = ks == PK_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    const hipMemcpyKind out_kind = kt == PK_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const int identity = s->size == 1;
    const int down = (const char *) target > (const char *) source &&
                     (const char *) target < (const char *) source + n * es;

#define CHUNK_ID(k) (down ? nchunks - 1 - (k) : (k)) /* the k-th chunk processed */
#define CHUNK_N(c) (n - (c) * per < per ? n - (c) * per : per)
    for (size_t k = 0; k < nchunks + 1; ++k) {
        /* copy-in of the k-th chunk (issued one chunk ahead of its reduction) */
        if (k < nchunks) {
            const int j = (int) (k & 1);
            const size_t c = CHUNK_ID (k);
            if (k >= 2) /* A[j] was last read by the copy-out (identity) or reduction of the (k-2)-th chunk */
                SHMEMI_HIP (hipStreamWaitEvent (shmemi.stream_in, shmemi.ev_out[j], 0));
            SHMEMI_HIP (hipMemcpyAsync (shmemi.heap + a_off[j], (const char *) source + c * per * es,
                                        CHUNK_N (c) * es, in_kind, shmemi.stream_in));
            SHMEMI_HIP (hipEventRecord (shmemi.ev_in[j], shmemi.stream_in));
        }
        if (k == 0)
            continue;
        /* reduce and copy out the (k-1)-th chunk */
        const size_t q = k - 1, c = CHUNK_ID (q);
        const int j = (int) (q & 1);
        const size_t cn = CHUNK_N (c);
        size_t out_off = a_off[j];
        if (identity) {
            SHMEMI_HIP (hipStreamWaitEvent (shmemi.stream_out, shmemi.ev_in[j], 0));
        } else {
            SHMEMI_HIP (hipEventSynchronize (shmemi.ev_in[j])); /* peers read A[j] after the barrier */
            if (q >= 2) /* B[j] is still being copied out for the (q-2)-th chunk */
                SHMEMI_HIP (hipStreamWaitEvent (shmemi.stream, shmemi.ev_out[j], 0));
            out_off = b_off[j];
            if (use_rccl) {
                if (shmemi_rccl_allreduce (op, dtype, shmemi.heap + a_off[j], shmemi.heap + b_off[j], cn) != 0)
                    shmemi_fatal ("%s: ncclAllReduce failed", fn);
            } else {
                reduce_symmetric (op, dtype, es, b_off[j], a_off[j], cn, s);
            }
        }
        SHMEMI_HIP (hipMemcpyAsync ((char *) target + c * per * es, shmemi.heap + out_off, cn * es, out_kind,
                                    shmemi.stream_out));
        SHMEMI_HIP (hipEventRecord (shmemi.ev_out[j], shmemi.stream_out));
    }
#undef CHUNK_N
#undef CHUNK_ID
    SHMEMI_HIP (hipStreamSynchronize (shmemi.stream_out));
    SHMEMI_HIP (hipStreamSynchronize (shmemi.stream_in));
}

/* Buffers outside the device symmetric heap that this GPU can still reach:
 * plain device memory (hipMalloc, e.g. a framework's tensors) and page-locked
 * host arrays (shmem_malloc's default heap). Instead of separate H2D/D2D/D2H
 * copies around the reduction:
 *   1 PE          one copy kernel straight from source to target (device to
 *                 device at any size; with a host side up to 1 MiB -- above,
 *                 the DMA double buffering of staged() is faster);
 *   N PEs, small  the fused kernel stages this PE's source into its scratch A
 *                 and the result out of scratch B itself (one launch) -- the
 *                 same scratch offsets and the same single collective as
 *                 staged()'s one-chunk case, so PEs that take staged() (pageable
 *                 host arrays) still meet it.
 * Host arrays: ~30 -> ~11 us at 1 PE and ~58 -> ~19 us at 2 PEs for 8 B -
 * 8 KiB. Returns 0 when it does not apply. */
#define SHMEMI_SMALL_LOCAL_MAX ((size_t) 1 << 20)
static const void *reachable (const void *p, size_t nbytes, int kind)
{
    return kind == PK_HOST ? shmemi_host_dev_ptr (p, nbytes) : p;
}

static int local_direct (int op, int dtype, void *target, const void *source, size_t n, int overlap, int kt,
                         int ks, const struct aset *s)
{
    const size_t es = mi355_dtype_size (dtype), nbytes = n * es;
    if (overlap && target != source)
        return 0;
    void *ht = (void *) reachable (target, nbytes, kt);
    const void *hs = reachable (source, nbytes, ks);
    if (ht == NULL || hs == NULL)
        return 0;
    const int any_host = kt == PK_HOST || ks == PK_HOST;
    if (s->size == 1) {
        if (any_host && nbytes > SHMEMI_SMALL_LOCAL_MAX)
            return 0;
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: 1-PE identity, one copy kernel source -> target (%zu bytes)",
                      nbytes);
        begin_call ("identity");
        if (target != source) {
            void *d = ht;
            size_t nb = nbytes;
            copy_wait (&d, &hs, &nb, 1, -1);
            note_call (0, 1, 1, 0, (unsigned long long) nbytes, 0, 0, mi355_last_kernel ());
        }
        return 1;
    }
    const size_t half = shmemi.scratch_chunk / 2 / SHMEMI_ALIGN * SHMEMI_ALIGN;
    if (nbytes > SHMEMI_SMALL_LOCAL_MAX || nbytes > half)
        return 0;
    struct sched_req r = blocking_req (COLL_REDUCE, op, dtype, es, shmemi.scratch_off + shmemi.scratch_chunk,
                                       shmemi.scratch_off, n, s);
    r.in_heap = 0; /* this PE's two sides are its host buffers */
    const struct sched_env e = sched_env_now ();
    const struct sched_plan p = plan_schedule (&e, &r);
    if (p.sched != SCHED_FUSED_ONESHOT && p.sched != SCHED_FUSED_TWOSHOT)
        return 0;
    fused_range (&p, &r, s, hs, ht);
    return 1;
}

/* SHMEM_DEBUG=1: the members compare their arguments before anything else
 * of the call happens (runtime.c, shmemi_debug_exchange). */
static void debug_check (const char *fn, int op, int dtype, const void *target, const void *source, int nreduce,
                         int PE_start, int logPE_stride, int PE_size)
{
    if (PE_size < 2)
        return;
    struct shmemi_dbg_rec r;
    memset (&r, 0, sizeof r);
    r.op = op;
    r.dtype = dtype;
    r.nreduce = nreduce;
    r.pe_start = PE_start;
    r.log_stride = logPE_stride;
    r.pe_size = PE_size;
    r.tkind = r.skind = -1;
    if (nreduce > 0) {
        const size_t nbytes = (size_t) nreduce * mi355_dtype_size (dtype);
        r.tkind = ptr_kind (target, nbytes);
        r.skind = ptr_kind (source, nbytes);
        if (r.tkind == PK_DEV_SYM)
            r.toff = shmemi_heap_offset (target);
        if (r.skind == PK_DEV_SYM)
            r.soff = shmemi_heap_offset (source);
        /* the staging path walks its chunks in an order the members share */
        const char *t = (const char *) target, *sr = (const char *) source;
        r.overlap = t == sr ? 1 : t > sr && t < sr + nbytes ? 2 : sr > t && sr < t + nbytes ? 3 : 0;
    }
    r.algorithm = shmemi.algorithm;
    r.order = shmemi.order;
    r.fused_max = shmemi.fused_max;
    r.oneshot_max = shmemi.oneshot_max;
    snprintf (r.fn, sizeof r.fn, "%s", fn);
    shmemi_debug_exchange (&r, PE_start, 1 << logPE_stride, PE_size);
}

/* SHMEM_FUSED_MAX_BYTES and SHMEM_ONESHOT_MAX_BYTES from measurement, at
 * init, on this job's own layout (PE_size > 1, the variable not given): the
 * fused one-launch schedule saves the multi-launch schedule's barrier
 * launches (barrier-linear.c:57-85's two barriers and the gather's own) but
 * pays its device-side flag round trips in one grid; where it stops paying
 * depends on the links (round 5, two PEs on one GPU: 1 MiB, not the 2 MiB
 * default; bench.py threshold_sweep). Double sums over the whole job between
 * scratch buffers A and B: each size timed both ways (median of 9 blocking
 * calls after 2 warm-ups, entry to return), the medians max-reduced over the
 * PEs through the bootstrap segment, and the threshold set to the largest
 * size of the prefix of sizes where the fused (one-shot) call was no slower
 * -- the same decision on every PE. About 250 calls, a few ms. */
void shmemi_calibrate_thresholds (int fused, int oneshot)
{
    static const size_t fsz[SHMEMI_CALIB_NF] = {64 << 10, 256 << 10, 512 << 10, 1 << 20, 2 << 20, 4 << 20};
    static const size_t osz[SHMEMI_CALIB_NO] = {16 << 10, 32 << 10, 64 << 10, 128 << 10, 256 << 10};
    const int np = shmemi.npes, me = shmemi.mype, K = 9, W = 2;
    struct aset s = {0, 1, np, me};
    const size_t src_off = shmemi.scratch_off, dst_off = shmemi.scratch_off + shmemi.scratch_chunk;
    const size_t f0 = shmemi.fused_max, o0 = shmemi.oneshot_max;
    const unsigned mask0 = shmemi_trace_mask;
    shmemi_trace_mask &= ~(1u << SHMEMI_LOG_REDUCTION); /* no schedule lines for these calls */
    SHMEMI_HIP (hipMemset (shmemi.heap + src_off, 0, shmemi.scratch_chunk));
    SHMEMI_HIP (hipDeviceSynchronize ());
    shmemi_barrier_set (0, 1, np);
    uint64_t mine[SHMEMI_CALIB_SLOTS] = {0};
    /* slot of (kind, size): kind 0 fused / 1 multi-launch / 2 one-shot / 3 two-shot */
#define SLOT(kind, i) ((kind) < 2 ? (kind) * SHMEMI_CALIB_NF + (i) : 2 * SHMEMI_CALIB_NF + ((kind) - 2) * SHMEMI_CALIB_NO + (i))
    for (int kind = 0; kind < 4; ++kind) {
        if ((kind < 2 && !fused) || (kind >= 2 && !oneshot))
            continue;
        const int nsz = kind < 2 ? SHMEMI_CALIB_NF : SHMEMI_CALIB_NO;
        for (int i = 0; i < nsz; ++i) {
            const size_t bytes = kind < 2 ? fsz[i] : osz[i];
            if (bytes > shmemi.scratch_chunk)
                continue; /* 0 = not measured: ends the prefix below */
            shmemi.fused_max = kind == 1 ? 0 : (size_t) 1 << 30;
            shmemi.oneshot_max = kind == 2 ? (size_t) 1 << 30 : kind == 3 ? 0 : o0;
            double t[16];
            for (int r = 0; r < W + K; ++r) {
                caller_order_pending = 1;
                const double t0 = shmemi_now ();
                reduce_symmetric (MI355_OP_SUM, MI355_DOUBLE, 8, dst_off, src_off, bytes / 8, &s);
                if (r >= W)
                    t[r - W] = shmemi_now () - t0;
            }
            for (int a = 1; a < K; ++a) /* median: insertion sort of 9 */
                for (int b = a; b > 0 && t[b] < t[b - 1]; --b) {
                    const double x = t[b];
                    t[b] = t[b - 1];
                    t[b - 1] = x;
                }
            mine[SLOT (kind, i)] = (uint64_t) (t[K / 2] * 1e9) + 1;
        }
    }
    struct shmemi_pe_info *info = shmemi_seg_info (me);
    for (int k = 0; k < SHMEMI_CALIB_SLOTS; ++k)
        __atomic_store_n (&info->calib_ns[k], mine[k], __ATOMIC_RELEASE);
    shmemi_barrier_set (0, 1, np);
    for (int k = 0; k < SHMEMI_CALIB_SLOTS; ++k) {
        uint64_t w = 0;
        for (int q = 0; q < np; ++q) {
            const uint64_t v = __atomic_load_n (&shmemi_seg_info (q)->calib_ns[k], __ATOMIC_ACQUIRE);
            w = v == 0 || w == UINT64_MAX ? UINT64_MAX : v > w ? v : w; /* unmeasured anywhere: unmeasured */
        }
        shmemi.calib_us[k] = w == UINT64_MAX ? 0.0 : (double) w * 1e-3;
    }
    shmemi_barrier_set (0, 1, np); /* nobody reads the records any more */
    /* the largest size of the prefix where the fused / one-shot call was no slower */
    size_t fm = f0, om = o0;
    if (fused) {
        fm = 0;
        for (int i = 0; i < SHMEMI_CALIB_NF; ++i) {
            const double a = shmemi.calib_us[SLOT (0, i)], b = shmemi.calib_us[SLOT (1, i)];
            if (a <= 0.0 || b <= 0.0 || a > b)
                break;
            fm = fsz[i];
        }
    }
    if (oneshot) {
        om = 0;
        for (int i = 0; i < SHMEMI_CALIB_NO; ++i) {
            const double a = shmemi.calib_us[SLOT (2, i)], b = shmemi.calib_us[SLOT (3, i)];
            if (a <= 0.0 || b <= 0.0 || a > b)
                break;
            om = osz[i];
        }
    }
#undef SLOT
    shmemi.fused_max = fm;
    shmemi.oneshot_max = om;
    shmemi.calib_ran = 1;
    shmemi_trace_mask = mask0;
    SHMEMI_TRACE (SHMEMI_LOG_INIT, "thresholds from measurement: fused path up to %zu bytes, one-shot up to %zu bytes",
                  fm, om);
}

/* What reduce_impl and scan_impl do first: the argument checks, the n == 0
 * call, the buffers' kinds (*kt target, *ks source) and the library stream
 * ordered after the caller's work. 0: the call is over (n == 0). */
static int entry_prologue (int op, int dtype, const char *fn, void *target, const void *source, int nreduce,
                           int PE_start, int logPE_stride, int PE_size, long *pSync, struct aset *s, int *kt, int *ks)
{
    shmemi_init_check (fn);
    aset_init (fn, s, PE_start, logPE_stride, PE_size);
    if (nreduce < 0)
        shmemi_fatal ("%s: nreduce %d < 0", fn, nreduce);
    if (shmemi.debug && pSync != NULL && (pSync[0] != SHMEM_SYNC_VALUE || pSync[1] != SHMEM_SYNC_VALUE))
        shmemi_fatal ("%s: pSync not initialised to SHMEM_SYNC_VALUE", fn);
    if (shmemi.debug)
        debug_check (fn, op, dtype, target, source, nreduce, PE_start, logPE_stride, PE_size);
    if (nreduce == 0) {
        begin_call ("barrier-only");
        /* both barriers of reduce-op.c:230,266 still run (host only: no GPU work) */
        shmemi_barrier_set (s->start, s->stride, s->size);
        shmemi_barrier_set (s->start, s->stride, s->size);
        return 0;
    }
    if (shmemi.heap == NULL)
        shmemi_fatal ("%s: no GPU: this library reduces on the GPU only (SHMEM_BOOTSTRAP_ONLY set?)", fn);
    if (target == NULL || source == NULL)
        shmemi_fatal ("%s: NULL target or source", fn);
    const size_t nbytes = (size_t) nreduce * mi355_dtype_size (dtype);
    *kt = ptr_kind (target, nbytes);
    *ks = ptr_kind (source, nbytes);
    /* Device buffers: the library stream is ordered after the caller's
     * null-stream work. The device-flag schedules (fused kernel, device
     * barriers) then learn on the GPU that peers' sources are ready; a
     * schedule with host barriers first waits for that point on the host. */
    if (*kt != PK_HOST || *ks != PK_HOST)
        shmemi_order_after_caller (0); /* SHMEM_ENTRY_SYNC */
    caller_order_pending = s->size > 1 && *kt == PK_DEV_SYM && *ks == PK_DEV_SYM;
    if (shmemi_trace_mask & (1u << SHMEMI_LOG_REDUCTION)) {
        static const char *const kind[] = {"host", "device heap", "device, not symmetric"};
        const int overlap = target != source && ranges_overlap ((size_t) target, (size_t) source, nbytes);
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION,
                      "%s: nreduce %d, PE_start %d, logPE_stride %d, PE_size %d; target %p (%s), source %p (%s)", fn,
                      nreduce, PE_start, logPE_stride, PE_size, target, kind[*kt], source, kind[*ks]);
        /* the reference's overlap trace (reduce-op.c:210-223) */
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "target (%p) and source (%p, size %zu) %s", target, source, nbytes,
                      target == source ? "are the same buffer" : overlap ? "overlap, using temporary target"
                                                                          : "do not overlap");
    }
    return 1;
}

static void reduce_impl (int op, int dtype, const char *fn, void *target, const void *source,
                         int nreduce, int PE_start, int logPE_stride, int PE_size, long *pSync)
{
    struct aset s;
    int kt, ks;
    if (!entry_prologue (op, dtype, fn, target, source, nreduce, PE_start, logPE_stride, PE_size, pSync, &s, &kt, &ks))
        return;
    const size_t es = mi355_dtype_size (dtype), n = (size_t) nreduce, nbytes = n * es;
    const int overlap = target != source && ranges_overlap ((size_t) target, (size_t) source, nbytes);
    /* RCCL by request, or whenever the init self-test found peer heap reads
     * broken (whatever the selected algorithm): the pairs RCCL has still run */
    const int use_rccl = (shmemi.algorithm == SHMEMX_REDUCE_RCCL || shmemi.p2p_broken) && s.size == shmemi.npes &&
                         s.size > 1 && shmemi_rccl_supported (op, dtype);
    if (use_rccl && kt != PK_HOST && ks != PK_HOST && !overlap) {
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: RCCL allreduce");
        shmemi_server_stop ();
        if (shmemi_rccl_allreduce (op, dtype, source, target, n) != 0)
            shmemi_fatal ("%s: ncclAllReduce failed", fn);
        /* RCCL's own kernels: bytes as a full-mesh exchange would move them */
        begin_call ("rccl");
        note_call (0, 1, 1, 0, (unsigned long long) nbytes, 0,
                   2ull * (unsigned long long) (s.size - 1) * nbytes / (unsigned long long) s.size, NULL);
        return;
    }
    if (kt == PK_DEV_SYM && ks == PK_DEV_SYM) {
        reduce_symmetric (op, dtype, es, shmemi_heap_offset (target), shmemi_heap_offset (source), n, &s);
        return;
    }
    /* device buffers outside the heap (a framework's tensors): the members
     * map each other's allocations for this call and run the heap schedules
     * on them, or, when one of them cannot, all stage (extmap.c) */
    if (s.size > 1 && !use_rccl) {
        size_t toff, soff;
        if (shmemi_ext_begin (fn, target, source, nbytes, kt, ks, s.start, s.stride, s.size, &toff, &soff)) {
            SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "device buffers outside the heap mapped by the peers for this call");
            caller_order_pending = 1; /* peers read this PE's buffers directly */
            reduce_symmetric (op, dtype, es, toff, soff, n, &s);
            shmemi_ext_end ();
            static char name[80];
            snprintf (name, sizeof name, "mapped-%s", shmemi.last.schedule);
            shmemi.last.schedule = name;
            return;
        }
    }

    if (!use_rccl && local_direct (op, dtype, target, source, n, overlap, kt, ks, &s))
        return;
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "staged through the scratch buffers (%s)", use_rccl ? "RCCL" : "P2P");
    begin_call ("staged");
    staged (op, dtype, fn, target, source, n, &s, ks, kt, use_rccl);
    shmemi.last.schedule = "staged"; /* the kernel fields: the last chunk's reduction */
}

/* ---------------------------------------------------------------------- */
/* stream-ordered collectives (shmemx.h)                                   */
/* ---------------------------------------------------------------------- */
/* The same P2P schedule, enqueued on the caller's stream with no host wait:
 * cross-PE ordering is device-side (fused.hip's pair counts), so a caller can
 * overlap the reduction with its own kernels or capture it into a HIP graph.
 *   fused-eligible   one launch of the fused kernel
 *   otherwise        device barrier, fold of shard `me`, device barrier,
 *                    gather, device barrier -- the host schedule's three
 *                    barriers, each a one-block kernel instead of a host wait
 They use their own signal-region channel, so a host-launched fused call may
 * run while they are in flight; among themselves they must run one at a time
 * per PE (one stream, or streams the caller orders). Errors of device-side
 * waits (a peer never arrives within SHMEM_BARRIER_TIMEOUT) surface at the
 * next library call. */

void shmemi_check_stream_err (const char *fn)
{
    if (shmemi.stream_err != NULL && __atomic_load_n (shmemi.stream_err, __ATOMIC_ACQUIRE) != 0)
        shmemi_fatal ("%s: a stream-ordered collective timed out waiting for another PE", fn);
}

static void stream_begin (const char *fn)
{
    shmemi_init_check (fn);
    if (shmemi.heap == NULL)
        shmemi_fatal ("%s: no GPU (SHMEM_BOOTSTRAP_ONLY set?)", fn);
    shmemi_server_stop (); /* its grid and the stream-ordered ones need not fit together */
    shmemi_check_stream_err (fn);
}

static void stream_aset (const char *fn, struct aset *s, int PE_start, int logPE_stride, int PE_size)
{
    aset_init (fn, s, PE_start, logPE_stride, PE_size);
    const struct sched_env e = sched_env_now ();
    plan_fatal (fn, stream_set_error (&e, PE_size), 0, PE_size);
}

static void reduce_on_stream (int op, int dtype, const char *fn, void *target, const void *source, int nreduce,
                              int PE_start, int logPE_stride, int PE_size, void *stream)
{
    hipStream_t st = (hipStream_t) stream;
    stream_begin (fn);
    struct aset s;
    stream_aset (fn, &s, PE_start, logPE_stride, PE_size);
    if (nreduce < 0)
        shmemi_fatal ("%s: nreduce %d < 0", fn, nreduce);
    const size_t es = mi355_dtype_size (dtype);
    const size_t n = (size_t) nreduce;
    const size_t nbytes = n * es;
    if (n > 0 && (target == NULL || source == NULL || !shmemi_in_device_heap (target, nbytes) ||
                  !shmemi_in_device_heap (source, nbytes)))
        shmemi_fatal ("%s: target and source must lie in the device symmetric heap (shmemx_malloc_device)", fn);
    if (shmemi.debug)
        debug_check (fn, op, dtype, target, source, nreduce, PE_start, logPE_stride, PE_size);

    const struct sched_req r = {COLL_REDUCE, ENTRY_STREAM, op, dtype, es, n > 0 ? shmemi_heap_offset (target) : 0,
                                n > 0 ? shmemi_heap_offset (source) : 0, n, s.size, s.me, 1, 0};
    const struct sched_env e = sched_env_now ();
    const struct sched_plan p = plan_schedule (&e, &r);
    plan_fatal (fn, p.err, 0, s.size);
    switch (p.sched) {
    case SCHED_BARRIER_ONLY:
        begin_call (sched_name (p.sched));
        stream_barrier (fn, &s, st);
        break;
    case SCHED_STREAM_IDENTITY:
        begin_call (sched_name (p.sched));
        if (!p.noop) {
            void *d = target;
            const void *sv = source;
            stream_copy (fn, &d, &sv, &nbytes, 1, st);
            note_call (0, 1, 1, 0, (unsigned long long) nbytes, 0, 0, mi355_last_kernel ());
        }
        break;
    case SCHED_STREAM_FUSED_ONESHOT:
    case SCHED_STREAM_FUSED_TWOSHOT: {
        MI355FusedArgs a;
        fused_args (&a, op, dtype, es, r.dst_off, r.src_off, n, p.ordered, p.oneshot, &s, SHMEMI_CHAN_STREAM);
        const int rc = mi355_fused_allreduce (&a, st);
        if (rc != 0)
            shmemi_fatal ("%s: fused reduction launch failed: %d", fn, rc);
        begin_call (sched_name (p.sched));
        note_fused (s.size, a.ordered, a.oneshot, n, es, mi355_last_kernel ());
        break;
    }
    default: /* SCHED_STREAM_P2P, SCHED_STREAM_P2P_ROUNDS */
        run_shards (&p, &r, &s, st, fn);
    }
}

void shmemx_barrier_on_stream (int PE_start, int logPE_stride, int PE_size, void *stream)
{
    hipStream_t st = (hipStream_t) stream;
    stream_begin ("shmemx_barrier_on_stream");
    struct aset s;
    stream_aset ("shmemx_barrier_on_stream", &s, PE_start, logPE_stride, PE_size);
    stream_barrier ("shmemx_barrier_on_stream", &s, st);
}

/* ---------------------------------------------------------------------- */
/* the 44 entry points (reduce-op.c:388-448), pshmem_ strong, shmem_ weak  */
/* ---------------------------------------------------------------------- */
#define SHMEMI_REDUCE(Name, Op, Type, DT, OPC)                                                      \
    void pshmem_##Name##_##Op##_to_all (Type *target, Type *source, int nreduce, int PE_start,       \
                                        int logPE_stride, int PE_size, Type *pWrk, long *pSync)      \
    {                                                                                                \
        (void) pWrk; /* scratch lives in the device heap; pWrk is not touched */                   \
        reduce_impl (OPC, DT, "shmem_" #Name "_" #Op "_to_all", target, source, nreduce, PE_start,  \
                     logPE_stride, PE_size, pSync);                                                  \
    }                                                                                                \
    void shmemx_##Name##_##Op##_to_all_on_stream (Type *target, Type *source, int nreduce,           \
                                                  int PE_start, int logPE_stride, int PE_size,       \
                                                  Type *pWrk, long *pSync, void *stream)             \
    {                                                                                                \
        (void) pWrk;                                                                                 \
        (void) pSync;                                                                                \
        reduce_on_stream (OPC, DT, "shmemx_" #Name "_" #Op "_to_all_on_stream", target, source,     \
                          nreduce, PE_start, logPE_stride, PE_size, stream);                         \
    }                                                                                                \
    void shmem_##Name##_##Op##_to_all (Type *target, Type *source, int nreduce, int PE_start,        \
                                       int logPE_stride, int PE_size, Type *pWrk, long *pSync)       \
        __attribute__ ((weak, alias ("pshmem_" #Name "_" #Op "_to_all")));

#define SUMPROD(Name, Type, DT)                          \
    SHMEMI_REDUCE (Name, sum, Type, DT, MI355_OP_SUM)    \
    SHMEMI_REDUCE (Name, prod, Type, DT, MI355_OP_PROD)
#define LOGIC(Name, Type, DT)                            \
    SHMEMI_REDUCE (Name, and, Type, DT, MI355_OP_AND)    \
    SHMEMI_REDUCE (Name, or, Type, DT, MI355_OP_OR)      \
    SHMEMI_REDUCE (Name, xor, Type, DT, MI355_OP_XOR)
#define MINMAX(Name, Type, DT)                           \
    SHMEMI_REDUCE (Name, max, Type, DT, MI355_OP_MAX)    \
    SHMEMI_REDUCE (Name, min, Type, DT, MI355_OP_MIN)

SUMPROD (short, short, MI355_SHORT)
SUMPROD (int, int, MI355_INT)
SUMPROD (long, long, MI355_LONG)
SUMPROD (longlong, long long, MI355_LONGLONG)
SUMPROD (double, double, MI355_DOUBLE)
SUMPROD (float, float, MI355_FLOAT)
SUMPROD (longdouble, long double, MI355_LONGDOUBLE)
SUMPROD (complexd, double _Complex, MI355_COMPLEXD)
SUMPROD (complexf, float _Complex, MI355_COMPLEXF)
LOGIC (short, short, MI355_SHORT)
LOGIC (int, int, MI355_INT)
LOGIC (long, long, MI355_LONG)
LOGIC (longlong, long long, MI355_LONGLONG)
MINMAX (short, short, MI355_SHORT)
MINMAX (int, int, MI355_INT)
MINMAX (long, long, MI355_LONG)
MINMAX (longlong, long long, MI355_LONGLONG)
MINMAX (double, double, MI355_DOUBLE)
MINMAX (float, float, MI355_FLOAT)
MINMAX (longdouble, long double, MI355_LONGDOUBLE)

/* ---------------------------------------------------------------------- */
/* 16-bit floats (shmemx.h): not in the reference, so shmemx_ names only   */
/* ---------------------------------------------------------------------- */
#define SHMEMX_REDUCE(Name, Op, DT, OPC)                                                             \
    void shmemx_##Name##_##Op##_to_all (shmemx_##Name##_t *target, shmemx_##Name##_t *source,        \
                                        int nreduce, int PE_start, int logPE_stride, int PE_size,    \
                                        shmemx_##Name##_t *pWrk, long *pSync)                        \
    {                                                                                                \
        (void) pWrk;                                                                                 \
        reduce_impl (OPC, DT, "shmemx_" #Name "_" #Op "_to_all", target, source, nreduce, PE_start, \
                     logPE_stride, PE_size, pSync);                                                  \
    }                                                                                                \
    void shmemx_##Name##_##Op##_to_all_on_stream (shmemx_##Name##_t *target,                         \
                                                  shmemx_##Name##_t *source, int nreduce,            \
                                                  int PE_start, int logPE_stride, int PE_size,       \
                                                  shmemx_##Name##_t *pWrk, long *pSync, void *stream) \
    {                                                                                                \
        (void) pWrk;                                                                                 \
        (void) pSync;                                                                                \
        reduce_on_stream (OPC, DT, "shmemx_" #Name "_" #Op "_to_all_on_stream", target, source,     \
                          nreduce, PE_start, logPE_stride, PE_size, stream);                         \
    }
#define SHMEMX_REDUCE_TYPE(Name, DT)                 \
    SHMEMX_REDUCE (Name, sum, DT, MI355_OP_SUM)      \
    SHMEMX_REDUCE (Name, prod, DT, MI355_OP_PROD)    \
    SHMEMX_REDUCE (Name, max, DT, MI355_OP_MAX)      \
    SHMEMX_REDUCE (Name, min, DT, MI355_OP_MIN)

SHMEMX_REDUCE_TYPE (half, MI355_HALF)
SHMEMX_REDUCE_TYPE (bfloat16, MI355_BFLOAT16)

/* ---------------------------------------------------------------------- */
/* scan: shmemx_<T>_<op>_inscan / _exscan (shmemx.h)                       */
/* ---------------------------------------------------------------------- */
/* Member j of the active set receives the left fold of the sources of
 * members 0 .. j (inscan) or 0 .. j - 1 (exscan; member 0's target is left
 * untouched), in ascending member order with the accumulator on the left.
 * There is one order, so the result-order setting does not apply, and the
 * algorithm setting does not change the bits: every request runs one of
 *
 *   shard    (up to MI355_ORDERS_MAX_SOURCES members) the shard schedule
 *            (shard_round) with the LEGS_INSCAN / LEGS_EXSCAN legs: the owner
 *            of shard i reads every member's source shard once and writes
 *            EVERY prefix of it (mi355_combine_prefix) -- its own into its
 *            target shard, member q's into slot q of its version area, from
 *            which q gathers it.
 *   direct   (larger sets, or SHMEM_SCAN_DIRECT=1, a testing aid) between two
 *            host barriers member j folds the whole arrays of members 0 .. j
 *            with mi355_combine: j + 1 times the reads instead of one.
 *
 * The kernels take an output that aliases the source of its own slot only
 * (mi355_reduce.h). In place that is inscan's shard fold; exscan in place
 * (the owner's prefix me - 1 would land on source me), the direct schedule
 * in place (the target would be the fold's last source) and partially
 * overlapping buffers go through scratch buffer C, as a reduction's
 * overlapping calls do. */

/* The owner's leg: every prefix of this PE's shard. 0: queued, or nothing
 * to do (an empty shard). */
static int scan_fold_shard (int op, int dtype, size_t es, size_t dst_off, size_t src_off, size_t n,
                            const struct aset *s, int excl, int chan, hipStream_t st)
{
    const void *sp[MI355_ORDERS_MAX_SOURCES];
    void *dsts[MI355_ORDERS_MAX_SOURCES];
    size_t lo, hi;
    mi355_shard_bounds (n, es, s->size, s->me, &lo, &hi);
    if (hi <= lo)
        return 0;
    const int nsrc = mi355_scan_sources (excl, s->size);
    const size_t slot = ver_slot_bytes (n, es, s->size);
    for (int q = 0; q < nsrc; ++q) {
        sp[q] = shmemi_peer_ptr (aset_pe (s, q), src_off + lo * es);
        dsts[q] = NULL;
    }
    for (int q = 0; q < s->size; ++q) {
        const int j = mi355_scan_slot (excl, q);
        if (j < 0)
            continue; /* exscan's member 0 receives nothing */
        dsts[j] = q == s->me ? shmemi_peer_ptr (shmemi.mype, dst_off + lo * es)
                             : shmemi_peer_ptr (shmemi.mype, ver_off (chan, s->me, q, slot, dst_off));
    }
    const int rc = mi355_combine_prefix (op, dtype, dsts, sp, nsrc, hi - lo, st);
    if (rc == 0)
        note_call (1, nsrc, nsrc, nsrc - (s->me < nsrc ? 1 : 0), (unsigned long long) ((hi - lo) * es), 0, 0,
                   mi355_last_kernel ());
    return rc;
}

/* The direct schedule: this member's fold of the whole arrays; dst must not
 * overlap any source (scan_symmetric routes overlaps through scratch). */
static void scan_direct (int op, int dtype, size_t es, size_t dst_off, size_t src_off, size_t n, const struct aset *s,
                         int excl)
{
    const int k = mi355_scan_slot (excl, s->me) + 1; /* sources 0 .. k - 1 */
    host_order ();
    shmemi_barrier_set (s->start, s->stride, s->size); /* every source is ready */
    if (k > 0) {
        const void **sp = (const void **) malloc (sizeof (void *) * (size_t) k);
        if (sp == NULL)
            shmemi_fatal ("out of host memory");
        shmemi_peer_acquire (shmemi.stream);
        for (int i = 0; i < k; ++i)
            sp[i] = shmemi_peer_ptr (aset_pe (s, i), src_off);
        combine_wait (op, dtype, shmemi_peer_ptr (shmemi.mype, dst_off), sp, k, n, 1);
        note_call (1, k, 1, k - (s->me < k ? 1 : 0), (unsigned long long) (n * es), 0, 0, mi355_last_kernel ());
        free (sp);
    }
    shmemi_barrier_set (s->start, s->stride, s->size); /* peers are done reading us */
}

/* ---------------------------------------------------------------------- */
/* executing a blocking plan                                               */
/* ---------------------------------------------------------------------- */
/* An overlap no schedule takes (sched_plan.h, via_scratch): through scratch
 * buffer C chunk by chunk, each a request of its own into C and one copy
 * from there, walking down when the target lies above the source (memmove
 * order) -- like the reference's temporary target (reduce-op.c:174-215), but
 * safe for any overlap. */
static void through_scratch (const struct sched_plan *p, const struct sched_req *r, const struct aset *s)
{
    const size_t tmp_off = shmemi.scratch_off + 2 * shmemi.scratch_chunk, per = p->chunk_elems;
    const size_t nchunks = (r->n + per - 1) / per;
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: %s, %zu chunk(s) through scratch, %s",
                  r->coll == COLL_REDUCE ? "overlapping target" : "scan with overlapping target", nchunks,
                  p->down ? "top down" : "bottom up");
    for (size_t c = 0; c < nchunks; ++c) {
        const size_t b = (p->down ? nchunks - 1 - c : c) * per;
        struct sched_req cr = *r;
        cr.chunk = 1;
        cr.dst_off = tmp_off;
        cr.src_off = r->src_off + b * r->es;
        cr.n = r->n - b < per ? r->n - b : per;
        run_blocking (&cr, s);
        if (p->receives)
            copy_local (r->dst_off + b * r->es, tmp_off, cr.n * r->es, 0);
        /* nobody reads our target chunk; the next chunk's first barrier orders
         * our write before any peer reads the source bytes it may cover */
    }
    if (s->size > 1)
        shmemi_barrier_set (s->start, s->stride, s->size);
}

static void run_blocking (const struct sched_req *r, const struct aset *s)
{
    const struct sched_env e = sched_env_now ();
    const struct sched_plan p = plan_schedule (&e, r);
    const size_t n = r->n, nbytes = n * r->es;
    const int scan = r->coll != COLL_REDUCE, excl = r->coll == COLL_EXSCAN;
    const int dev = p.sync == SYNC_DEV;
    plan_fatal (NULL, p.err, scan, s->size);
    if (scan && !r->chunk && s->size > 1 &&
        (shmemi.algorithm == SHMEMX_REDUCE_EXACT || shmemi.algorithm == SHMEMX_REDUCE_RCCL))
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "scan: the %s request does not apply (a scan has one order and RCCL has "
                                            "no scan); running the scan schedule",
                      shmemi.algorithm == SHMEMX_REDUCE_EXACT ? "EXACT" : "RCCL");
    if (p.sched == SCHED_SCAN_LOCAL && !r->chunk)
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: scan of one member: %s",
                      excl ? "exscan, nothing to do" : r->dst_off == r->src_off ? "inscan in place, nothing to move"
                                                                                : "inscan, one copy");
    if (p.via_scratch) {
        /* one name for the whole walk where the chunks announce none */
        if (p.sched == SCHED_IDENTITY || p.sched == SCHED_EXACT || p.sched == SCHED_SCAN_LOCAL)
            begin_call (sched_name (p.sched));
        through_scratch (&p, r, s);
        return;
    }
    switch (p.sched) {
    case SCHED_IDENTITY:
    case SCHED_SCAN_LOCAL:
        if (r->chunk) {
            copy_local (r->dst_off, r->src_off, nbytes, 0);
        } else if (p.servable) {
            fused_range (&p, r, s, NULL, NULL);
        } else if (scan || p.noop) {
            if (!scan)
                SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: 1-PE identity in place, nothing to move");
            begin_call (sched_name (p.sched));
            if (!p.noop)
                copy_local (r->dst_off, r->src_off, nbytes, 1);
        } else {
            identity_copy (r);
        }
        break;
    case SCHED_FUSED_ONESHOT:
    case SCHED_FUSED_TWOSHOT:
        fused_range (&p, r, s, NULL, NULL);
        break;
    case SCHED_EXACT:
        if (!r->chunk) {
            SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: EXACT reference order, host barriers");
            begin_call (sched_name (p.sched));
        }
        host_order ();
        shmemi_barrier_set (s->start, s->stride, s->size);
        exact_into (r->op, r->dtype, r->dst_off, r->src_off, n, s);
        shmemi_barrier_set (s->start, s->stride, s->size);
        break;
    case SCHED_SCAN_DIRECT:
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: scan, direct: each member folds its prefix of the whole "
                                            "arrays, host barriers (%zu elements, %d members)", n, s->size);
        begin_call (sched_name (p.sched));
        scan_direct (r->op, r->dtype, r->es, r->dst_off, r->src_off, n, s, excl);
        break;
    default: /* the shard schedules */
        if (scan)
            SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: scan, P2P shards, %s barriers, every prefix from one pass "
                                                "(%zu elements, %d members%s)", dev ? "device" : "host", n, s->size,
                          n > p.round ? ", several rounds" : "");
        else
            SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: P2P shards, %s barriers, %s (%zu elements, %d members%s)",
                          dev ? "device" : "host",
                          p.legs == LEGS_PAIR ? "each member's reference order (own-order fold, NaN-patched gather)"
                          : p.ordered         ? "every member's reference order"
                                              : "PE_start order",
                          n, s->size, n > p.round ? ", several rounds" : "");
        run_shards (&p, r, s, shmemi.stream, NULL);
    }
}

static void scan_symmetric (int op, int dtype, size_t es, size_t dst_off, size_t src_off, size_t n,
                            const struct aset *s, int excl)
{
    const struct sched_req r = blocking_req (excl ? COLL_EXSCAN : COLL_INSCAN, op, dtype, es, dst_off, src_off, n, s);
    run_blocking (&r, s);
}

/* Host-heap (shmem_malloc) and other host arrays: each chunk goes into
 * scratch A, is scanned into scratch B and comes back out, in memmove order
 * when target and source overlap. Blocking copies: no double buffering. */
static void scan_staged (int op, int dtype, void *target, const void *source, size_t n, const struct aset *s,
                         int excl)
{
    const size_t es = mi355_dtype_size (dtype);
    const size_t per = shmemi.scratch_chunk / es;
    const size_t nchunks = (n + per - 1) / per;
    const size_t a_off = shmemi.scratch_off, b_off = shmemi.scratch_off + shmemi.scratch_chunk;
    const int receives = !(excl && s->me == 0);
    const int down = (const char *) target > (const char *) source &&
                     (const char *) target < (const char *) source + n * es;
    for (size_t c = 0; c < nchunks; ++c) {
        const size_t idx = down ? nchunks - 1 - c : c;
        const size_t b = idx * per;
        const size_t cn = n - b < per ? n - b : per;
        SHMEMI_HIP (hipMemcpy (shmemi.heap + a_off, (const char *) source + b * es, cn * es, hipMemcpyDefault));
        scan_symmetric (op, dtype, es, b_off, a_off, cn, s, excl);
        if (receives)
            SHMEMI_HIP (hipMemcpy ((char *) target + b * es, shmemi.heap + b_off, cn * es, hipMemcpyDefault));
    }
}

static void scan_impl (int op, int dtype, int excl, const char *fn, void *target, const void *source, int nreduce,
                       int PE_start, int logPE_stride, int PE_size, long *pSync)
{
    struct aset s;
    int kt, ks;
    if (!entry_prologue (op, dtype, fn, target, source, nreduce, PE_start, logPE_stride, PE_size, pSync, &s, &kt, &ks))
        return;
    if (kt == PK_DEV_OTHER || ks == PK_DEV_OTHER)
        shmemi_fatal ("%s: %s is device memory outside the symmetric heap; the scan collectives take device-heap "
                      "(shmemx_malloc_device) and host objects only", fn, kt == PK_DEV_OTHER ? "target" : "source");
    const size_t es = mi355_dtype_size (dtype), n = (size_t) nreduce;
    if (kt == PK_DEV_SYM && ks == PK_DEV_SYM) {
        scan_symmetric (op, dtype, es, shmemi_heap_offset (target), shmemi_heap_offset (source), n, &s, excl);
        return;
    }
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "scan staged through the scratch buffers");
    begin_call ("scan-staged");
    scan_staged (op, dtype, target, source, n, &s, excl);
    shmemi.last.schedule = "scan-staged"; /* the kernel fields: the last chunk's scan */
}

/* the 52 (type, op) pairs of *_to_all, each as inscan and exscan: shmemx_ names only */
#define SHMEMX_SCAN(Name, Op, Type, DT, OPC)                                                              \
    void shmemx_##Name##_##Op##_inscan (Type *target, Type *source, int nreduce, int PE_start,            \
                                        int logPE_stride, int PE_size, Type *pWrk, long *pSync)           \
    {                                                                                                     \
        (void) pWrk;                                                                                      \
        scan_impl (OPC, DT, 0, "shmemx_" #Name "_" #Op "_inscan", target, source, nreduce, PE_start,     \
                   logPE_stride, PE_size, pSync);                                                         \
    }                                                                                                     \
    void shmemx_##Name##_##Op##_exscan (Type *target, Type *source, int nreduce, int PE_start,            \
                                        int logPE_stride, int PE_size, Type *pWrk, long *pSync)           \
    {                                                                                                     \
        (void) pWrk;                                                                                      \
        scan_impl (OPC, DT, 1, "shmemx_" #Name "_" #Op "_exscan", target, source, nreduce, PE_start,     \
                   logPE_stride, PE_size, pSync);                                                         \
    }
#define SCAN_SUMPROD(Name, Type, DT)                   \
    SHMEMX_SCAN (Name, sum, Type, DT, MI355_OP_SUM)    \
    SHMEMX_SCAN (Name, prod, Type, DT, MI355_OP_PROD)
#define SCAN_LOGIC(Name, Type, DT)                     \
    SHMEMX_SCAN (Name, and, Type, DT, MI355_OP_AND)    \
    SHMEMX_SCAN (Name, or, Type, DT, MI355_OP_OR)      \
    SHMEMX_SCAN (Name, xor, Type, DT, MI355_OP_XOR)
#define SCAN_MINMAX(Name, Type, DT)                    \
    SHMEMX_SCAN (Name, max, Type, DT, MI355_OP_MAX)    \
    SHMEMX_SCAN (Name, min, Type, DT, MI355_OP_MIN)

SCAN_SUMPROD (short, short, MI355_SHORT)
SCAN_SUMPROD (int, int, MI355_INT)
SCAN_SUMPROD (long, long, MI355_LONG)
SCAN_SUMPROD (longlong, long long, MI355_LONGLONG)
SCAN_SUMPROD (double, double, MI355_DOUBLE)
SCAN_SUMPROD (float, float, MI355_FLOAT)
SCAN_SUMPROD (longdouble, long double, MI355_LONGDOUBLE)
SCAN_SUMPROD (complexd, double _Complex, MI355_COMPLEXD)
SCAN_SUMPROD (complexf, float _Complex, MI355_COMPLEXF)
SCAN_SUMPROD (half, shmemx_half_t, MI355_HALF)
SCAN_SUMPROD (bfloat16, shmemx_bfloat16_t, MI355_BFLOAT16)
SCAN_LOGIC (short, short, MI355_SHORT)
SCAN_LOGIC (int, int, MI355_INT)
SCAN_LOGIC (long, long, MI355_LONG)
SCAN_LOGIC (longlong, long long, MI355_LONGLONG)
SCAN_MINMAX (short, short, MI355_SHORT)
SCAN_MINMAX (int, int, MI355_INT)
SCAN_MINMAX (long, long, MI355_LONG)
SCAN_MINMAX (longlong, long long, MI355_LONGLONG)
SCAN_MINMAX (double, double, MI355_DOUBLE)
SCAN_MINMAX (float, float, MI355_FLOAT)
SCAN_MINMAX (longdouble, long double, MI355_LONGDOUBLE)
SCAN_MINMAX (half, shmemx_half_t, MI355_HALF)
SCAN_MINMAX (bfloat16, shmemx_bfloat16_t, MI355_BFLOAT16)

/* ---------------------------------------------------------------------- */
/* value and location: shmemx_<T>_maxloc_to_all / _minloc_to_all (shmemx.h) */
/* ---------------------------------------------------------------------- */
/* The host-synchronised row of the shard schedule with a pair of arrays on
 * each side: barrier (every source is ready), the owner folds its shard of
 * every member's values and locations into its own target and target_loc
 * (mi355_combine_loc; the same element range of both), barrier, one copy
 * launch pulls the other owners' two shards from their targets, barrier.
 * Nothing is rounded and the owner presents the members in ascending order,
 * so every member holds the same bits whatever the shard bounds are. In
 * place (target == source and target_loc == source_loc) the owner's output
 * aliases its own entry of the fold, which the kernel allows.
 *
 * Not built (shmemx.h says the same): long double and complex, a
 * stream-ordered or graph-captured form, the fused one-launch kernel, the
 * persistent server, RCCL, Fortran wrappers, the SHMEM_DEBUG argument
 * exchange, staging of host arrays. */

struct loc_call {
    int op, dtype;
    size_t es;
    size_t t_off, tl_off, s_off, sl_off; /* heap offsets; sl_off is unused when implicit */
    int implicit;                        /* source_loc == NULL: the location is the member index */
};

/* The owner's fold of elements [lo, hi) over every member, signalled and
 * waited. Up to 32 members: one launch into the target. Above: chained
 * launches (loc_plan.h), the running pair carried in scratch buffers A
 * (values) and B (locations) so that an in-place target still holds this
 * member's source when its turn comes; the range is walked in pieces whose
 * locations fit buffer B. */
static void loc_fold_range (const struct loc_call *c, const struct aset *s, size_t lo, size_t hi)
{
    const int chunks = mi355_loc_chunk_count (s->size);
    const size_t piece = chunks == 1 ? hi - lo : shmemi.scratch_chunk / sizeof (long);
    void *carry_val = shmemi.heap + shmemi.scratch_off;
    long *carry_loc = (long *) (shmemi.heap + shmemi.scratch_off + shmemi.scratch_chunk);
    if (piece == 0)
        shmemi_fatal ("SHMEM_DEVICE_SCRATCH_SIZE is too small for a value-and-location fold over %d members", s->size);
    for (size_t b = lo; b < hi; b += piece) {
        const size_t e = hi - b < piece ? hi : b + piece, len = e - b;
        for (int k = 0; k < chunks; ++k) {
            const mi355_loc_chunk ck = mi355_loc_chunk_at (s->size, k);
            const void *sv[MI355_LOC_MAX_SOURCES];
            const long *sl[MI355_LOC_MAX_SOURCES];
            if (ck.lead) {
                sv[0] = carry_val;
                sl[0] = carry_loc;
            }
            for (int i = 0; i < ck.take; ++i) {
                const int pe = aset_pe (s, ck.first + i);
                sv[ck.lead + i] = shmemi_peer_ptr (pe, c->s_off + b * c->es);
                sl[ck.lead + i] = c->implicit ? NULL : (const long *) shmemi_peer_ptr (pe, c->sl_off + b * sizeof (long));
            }
            void *dv = ck.final ? shmemi_peer_ptr (shmemi.mype, c->t_off + b * c->es) : carry_val;
            long *dl = ck.final ? (long *) shmemi_peer_ptr (shmemi.mype, c->tl_off + b * sizeof (long)) : carry_loc;
            const int last = ck.final && e == hi;
            if (last) {
                shmemi_timed_begin ();
                shmemi_arm_signal ();
            }
            const int rc = mi355_combine_loc (c->op, c->dtype, dv, dl, sv, sl, ck.loc_shift, ck.lead + ck.take, len,
                                              shmemi.stream);
            if (last)
                shmemi_timed_end ();
            if (rc != 0)
                shmemi_fatal ("value-and-location kernel launch failed (op %d, dtype %d, %d members, %zu elements): %d",
                              c->op, c->dtype, s->size, len, rc);
        }
    }
    note_call (0, s->size, 1, s->size - 1, (unsigned long long) ((hi - lo) * (c->es + sizeof (long))), 0, 0,
               mi355_last_kernel ());
    shmemi_wait_signal ();
}

static void loc_p2p (const struct loc_call *c, const struct aset *s, size_t n)
{
    size_t lo, hi;
    mi355_shard_bounds (n, c->es, s->size, s->me, &lo, &hi);
    host_order ();
    shmemi_barrier_set (s->start, s->stride, s->size); /* every source is ready */
    if (hi > lo) {
        shmemi_peer_acquire (shmemi.stream);
        loc_fold_range (c, s, lo, hi);
    }
    shmemi_barrier_set (s->start, s->stride, s->size); /* every shard is folded */
    shmemi_peer_acquire (shmemi.stream);

    /* the other owners' shards, values and locations: 2 (N - 1) segments */
    const size_t m = 2 * (size_t) s->size;
    void **dsts = (void **) malloc (m * (2 * sizeof (void *) + sizeof (size_t)));
    if (dsts == NULL)
        shmemi_fatal ("out of host memory");
    const void **sp = (const void **) (dsts + m);
    size_t *nb = (size_t *) (sp + m);
    int k = 0;
    for (int i = 0; i < s->size; ++i) {
        size_t l, h;
        mi355_shard_bounds (n, c->es, s->size, i, &l, &h);
        if (i == s->me || h <= l)
            continue;
        dsts[k] = shmemi_peer_ptr (shmemi.mype, c->t_off + l * c->es);
        sp[k] = shmemi_peer_ptr (aset_pe (s, i), c->t_off + l * c->es);
        nb[k++] = (h - l) * c->es;
        dsts[k] = shmemi_peer_ptr (shmemi.mype, c->tl_off + l * sizeof (long));
        sp[k] = shmemi_peer_ptr (aset_pe (s, i), c->tl_off + l * sizeof (long));
        nb[k++] = (h - l) * sizeof (long);
    }
    copy_wait (dsts, sp, nb, k, 1);
    free (dsts);
    shmemi_barrier_set (s->start, s->stride, s->size); /* peers are done reading this target */
}

static void loc_impl (int op, int dtype, const char *fn, void *target, long *target_loc, const void *source,
                      const long *source_loc, int nreduce, int PE_start, int logPE_stride, int PE_size)
{
    struct aset s;
    shmemi_init_check (fn);
    aset_init (fn, &s, PE_start, logPE_stride, PE_size);
    if (nreduce < 0)
        shmemi_fatal ("%s: nreduce %d < 0", fn, nreduce);
    if (nreduce == 0) {
        begin_call ("barrier-only");
        shmemi_barrier_set (s.start, s.stride, s.size);
        shmemi_barrier_set (s.start, s.stride, s.size);
        return;
    }
    if (shmemi.heap == NULL)
        shmemi_fatal ("%s: no GPU: this library reduces on the GPU only (SHMEM_BOOTSTRAP_ONLY set?)", fn);
    const size_t n = (size_t) nreduce, es = mi355_dtype_size (dtype);
    const struct {
        const char *name;
        const void *p;
        size_t nbytes;
        int optional;
    } args[4] = {{"target", target, n * es, 0},
                 {"target_loc", target_loc, n * sizeof (long), 0},
                 {"source", source, n * es, 0},
                 {"source_loc", source_loc, n * sizeof (long), 1}};
    for (int i = 0; i < 4; ++i) {
        if (args[i].p == NULL && args[i].optional)
            continue;
        if (args[i].p == NULL)
            shmemi_fatal ("%s: NULL %s", fn, args[i].name);
        if (ptr_kind (args[i].p, args[i].nbytes) != PK_DEV_SYM)
            shmemi_fatal ("%s: %s (%p, %zu bytes) is not in the device symmetric heap; the value-and-location "
                          "reductions take device-heap (shmemx_malloc_device) arrays only", fn, args[i].name,
                          args[i].p, args[i].nbytes);
    }
    if (s.size > 1 && shmemi.p2p_broken)
        shmemi_fatal ("%s: peer GPU memory reads failed the init self-test; the value-and-location reductions "
                      "need them", fn);
    shmemi_order_after_caller (0); /* SHMEM_ENTRY_SYNC */
    caller_order_pending = s.size > 1;
    const struct loc_call c = {op, dtype, es, shmemi_heap_offset (target), shmemi_heap_offset (target_loc),
                               shmemi_heap_offset (source), source_loc != NULL ? shmemi_heap_offset (source_loc) : 0,
                               source_loc == NULL};
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "%s: nreduce %d, PE_start %d, logPE_stride %d, PE_size %d; %s locations%s",
                  fn, nreduce, PE_start, logPE_stride, PE_size, c.implicit ? "member-index" : "explicit",
                  target == source && (c.implicit || (const long *) target_loc == source_loc) ? ", in place" : "");
    if (s.size == 1) {
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: value and location, one member: one local fold, no barrier");
        begin_call ("loc-local");
        loc_fold_range (&c, &s, 0, n);
        return;
    }
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: value and location, P2P shards, host barriers: fold of values "
                                        "and locations, one gather of both (%zu elements, %d members%s)", n, s.size,
                  mi355_loc_chunk_count (s.size) > 1 ? ", chained fold launches" : "");
    begin_call ("loc-p2p");
    loc_p2p (&c, &s, n);
}

#define SHMEMX_LOC(Name, Type, DT)                                                                              \
    void shmemx_##Name##_maxloc_to_all (Type *target, long *target_loc, const Type *source,                     \
                                        const long *source_loc, int nreduce, int PE_start, int logPE_stride,    \
                                        int PE_size)                                                            \
    {                                                                                                           \
        loc_impl (MI355_OP_MAX, DT, "shmemx_" #Name "_maxloc_to_all", target, target_loc, source, source_loc,   \
                  nreduce, PE_start, logPE_stride, PE_size);                                                    \
    }                                                                                                           \
    void shmemx_##Name##_minloc_to_all (Type *target, long *target_loc, const Type *source,                     \
                                        const long *source_loc, int nreduce, int PE_start, int logPE_stride,    \
                                        int PE_size)                                                            \
    {                                                                                                           \
        loc_impl (MI355_OP_MIN, DT, "shmemx_" #Name "_minloc_to_all", target, target_loc, source, source_loc,   \
                  nreduce, PE_start, logPE_stride, PE_size);                                                    \
    }

SHMEMX_LOC (short, short, MI355_SHORT)
SHMEMX_LOC (int, int, MI355_INT)
SHMEMX_LOC (long, long, MI355_LONG)
SHMEMX_LOC (longlong, long long, MI355_LONGLONG)
SHMEMX_LOC (float, float, MI355_FLOAT)
SHMEMX_LOC (double, double, MI355_DOUBLE)
SHMEMX_LOC (half, shmemx_half_t, MI355_HALF)
SHMEMX_LOC (bfloat16, shmemx_bfloat16_t, MI355_BFLOAT16)

/* ---------------------------------------------------------------------- */
/* wide sum: shmemx_<T>_wsum_to_all / _wsum_to_all_float (shmemx.h)         */
/* ---------------------------------------------------------------------- */
/* Half and bfloat16 sums accumulated in binary32 and rounded once, or not at
 * all (mi355_combine_wide). The host-synchronised row of the shard schedule,
 * as loc_p2p: barrier (every source is ready), the owner folds its shard of
 * every member's source into its own target, barrier, one copy launch pulls
 * the other owners' shards from their targets, barrier. The owner presents
 * the members in ascending order whatever SHMEM_REDUCE_ORDER says, so every
 * member holds the same bits, independent of the shard bounds; this
 * collective does not go through plan_schedule. The bounds are those of the
 * 2-byte source elements for both outputs, so a float shard starts on a
 * 512-byte boundary. In place (target == source, 16-bit result) the owner's
 * output aliases its own entry of the fold, which the kernel allows.
 *
 * Not built (shmemx.h says the same): stream-ordered, fused, persistent and
 * RCCL forms, Fortran wrappers, host-heap or external buffers, prod, min and
 * max, sets above 32 members. */

struct wide_call {
    int dtype, out_dtype;
    size_t oes;          /* bytes of one target element: 2 or 4 */
    size_t t_off, s_off; /* heap offsets */
};

/* The owner's fold of elements [lo, hi) over every member, signalled and waited. */
static void wide_fold_range (const struct wide_call *c, const struct aset *s, size_t lo, size_t hi)
{
    const void *sv[MI355_ORDERS_MAX_SOURCES];
    for (int i = 0; i < s->size; ++i)
        sv[i] = shmemi_peer_ptr (aset_pe (s, i), c->s_off + lo * 2);
    shmemi_timed_begin ();
    shmemi_arm_signal ();
    const int rc = mi355_combine_wide (c->dtype, c->out_dtype, shmemi_peer_ptr (shmemi.mype, c->t_off + lo * c->oes), sv,
                                       s->size, hi - lo, shmemi.stream);
    shmemi_timed_end ();
    if (rc != 0)
        shmemi_fatal ("wide sum kernel launch failed (dtype %d, out %d, %d members, %zu elements): %d", c->dtype,
                      c->out_dtype, s->size, hi - lo, rc);
    /* the sources and the output as 2-byte buffers; a float output's other half beyond them */
    note_call (0, s->size, 1, s->size - 1, (unsigned long long) ((hi - lo) * 2),
               (unsigned long long) ((hi - lo) * (c->oes - 2)), 0, mi355_last_kernel ());
    shmemi_wait_signal ();
}

static void wide_p2p (const struct wide_call *c, const struct aset *s, size_t n)
{
    size_t lo, hi;
    mi355_shard_bounds (n, 2, s->size, s->me, &lo, &hi);
    host_order ();
    shmemi_barrier_set (s->start, s->stride, s->size); /* every source is ready */
    if (hi > lo) {
        shmemi_peer_acquire (shmemi.stream);
        wide_fold_range (c, s, lo, hi);
    }
    shmemi_barrier_set (s->start, s->stride, s->size); /* every shard is folded */
    shmemi_peer_acquire (shmemi.stream);

    /* the other owners' shards of the target: at most N - 1 segments */
    void *dsts[MI355_ORDERS_MAX_SOURCES];
    const void *sp[MI355_ORDERS_MAX_SOURCES];
    size_t nb[MI355_ORDERS_MAX_SOURCES];
    int k = 0;
    for (int i = 0; i < s->size; ++i) {
        size_t l, h;
        mi355_shard_bounds (n, 2, s->size, i, &l, &h);
        if (i == s->me || h <= l)
            continue;
        dsts[k] = shmemi_peer_ptr (shmemi.mype, c->t_off + l * c->oes);
        sp[k] = shmemi_peer_ptr (aset_pe (s, i), c->t_off + l * c->oes);
        nb[k++] = (h - l) * c->oes;
    }
    copy_wait (dsts, sp, nb, k, 1);
    shmemi_barrier_set (s->start, s->stride, s->size); /* peers are done reading this target */
}

static void wide_impl (int dtype, int float_out, const char *fn, void *target, const void *source, int nreduce,
                       int PE_start, int logPE_stride, int PE_size)
{
    struct aset s;
    shmemi_init_check (fn);
    aset_init (fn, &s, PE_start, logPE_stride, PE_size);
    if (PE_size > MI355_ORDERS_MAX_SOURCES)
        shmemi_fatal ("%s: PE_size %d: the wide sums take active sets of at most %d members", fn, PE_size,
                      MI355_ORDERS_MAX_SOURCES);
    if (nreduce < 0)
        shmemi_fatal ("%s: nreduce %d < 0", fn, nreduce);
    if (nreduce == 0) {
        begin_call ("barrier-only");
        shmemi_barrier_set (s.start, s.stride, s.size);
        shmemi_barrier_set (s.start, s.stride, s.size);
        return;
    }
    if (shmemi.heap == NULL)
        shmemi_fatal ("%s: no GPU: this library reduces on the GPU only (SHMEM_BOOTSTRAP_ONLY set?)", fn);
    const size_t n = (size_t) nreduce, oes = float_out ? sizeof (float) : 2;
    const struct {
        const char *name;
        const void *p;
        size_t nbytes;
    } args[2] = {{"target", target, n * oes}, {"source", source, n * 2}};
    for (int i = 0; i < 2; ++i) {
        if (args[i].p == NULL)
            shmemi_fatal ("%s: NULL %s", fn, args[i].name);
        if (ptr_kind (args[i].p, args[i].nbytes) != PK_DEV_SYM)
            shmemi_fatal ("%s: %s (%p, %zu bytes) is not in the device symmetric heap; the wide sums take "
                          "device-heap (shmemx_malloc_device) arrays only", fn, args[i].name, args[i].p,
                          args[i].nbytes);
    }
    const size_t t = (size_t) target, sr = (size_t) source;
    if (t < sr + n * 2 && sr < t + n * oes && (float_out || t != sr))
        shmemi_fatal (float_out ? "%s: the float target (%p, %zu bytes) overlaps source (%p, %zu bytes)"
                                : "%s: target (%p, %zu bytes) and source (%p, %zu bytes) overlap without being equal",
                      fn, target, n * oes, source, n * 2);
    if (s.size > 1 && shmemi.p2p_broken)
        shmemi_fatal ("%s: peer GPU memory reads failed the init self-test; the wide sums need them", fn);
    shmemi_order_after_caller (0); /* SHMEM_ENTRY_SYNC */
    caller_order_pending = s.size > 1;
    const struct wide_call c = {dtype, float_out ? MI355_FLOAT : dtype, oes, shmemi_heap_offset (target),
                                shmemi_heap_offset (source)};
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "%s: nreduce %d, PE_start %d, logPE_stride %d, PE_size %d; %s result%s", fn,
                  nreduce, PE_start, logPE_stride, PE_size, float_out ? "float" : "16-bit",
                  target == source ? ", in place" : "");
    if (s.size == 1) {
        SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: wide sum, one member: one local fold, no barrier");
        begin_call ("wide-local");
        wide_fold_range (&c, &s, 0, n);
        return;
    }
    SHMEMI_TRACE (SHMEMI_LOG_REDUCTION, "schedule: wide sum, P2P shards, host barriers: binary32 fold in ascending "
                                        "member order, one gather (%zu elements, %d members)", n, s.size);
    begin_call ("wide-p2p");
    wide_p2p (&c, &s, n);
}

#define SHMEMX_WSUM(Name, Type, DT)                                                                               \
    void shmemx_##Name##_wsum_to_all (Type *target, const Type *source, int nreduce, int PE_start,                \
                                      int logPE_stride, int PE_size)                                              \
    {                                                                                                             \
        wide_impl (DT, 0, "shmemx_" #Name "_wsum_to_all", target, source, nreduce, PE_start, logPE_stride,        \
                   PE_size);                                                                                      \
    }                                                                                                             \
    void shmemx_##Name##_wsum_to_all_float (float *target, const Type *source, int nreduce, int PE_start,         \
                                            int logPE_stride, int PE_size)                                        \
    {                                                                                                             \
        wide_impl (DT, 1, "shmemx_" #Name "_wsum_to_all_float", target, source, nreduce, PE_start, logPE_stride,  \
                   PE_size);                                                                                      \
    }

SHMEMX_WSUM (half, shmemx_half_t, MI355_HALF)
SHMEMX_WSUM (bfloat16, shmemx_bfloat16_t, MI355_BFLOAT16)
