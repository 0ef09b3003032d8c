/*
 * coll.c -- the data-movement neighbours of the reduction path (SURVEY.md
 * section 8f rows 3-4): one-sided put/get and the broadcast / collect /
 * fcollect collectives, over the same device symmetric heap and peer
 * mappings as the reductions.
 *
 * Reference semantics followed:
 *   shmem_putmem/getmem, put/get32/64/128, shmem_<T>_put/get
 *       src/ptp/putget.c:116-256 -> shmemi_comms_put_bulk / get_bulk: blocking
 *       byte copies to/from a symmetric address on another PE
 *   shmem_broadcast32/64   src/broadcast/broadcast.c:69-110,
 *       linear form broadcast-linear.c:61-82: barrier, then every PE but the
 *       root copies the root's source into its target; the root's target is
 *       untouched (the reference's default tree form, broadcast-tree.c, also
 *       overwrites the non-root PEs' SOURCE with the data as it forwards it;
 *       that side effect is not part of the API and is not reproduced)
 *   shmem_fcollect32/64    src/fcollect/fcollect-linear.c:60-93: PE i's
 *       nelems elements land at offset i*nelems of every member's target
 *   shmem_collect32/64     src/collect/collect-linear.c:60-156: like fcollect
 *       with per-PE counts; offsets are the running sum in active-set order
 *   shmem_alltoall32/64, shmem_alltoalls32/64   src/alltoall/alltoall-linear.c:
 *       member i's block m lands as block i of member m's target, the strided
 *       form dst / sst elements apart (see alltoall_bytes for the one
 *       deliberate deviation: blocks are numbered by the index in the active
 *       set, not by the global PE number)
 *   shmem_<T>_iput/iget, shmem_iput/iget32/64/128   src/ptp/strided.c:110-238:
 *       target[k*tst] = source[k*sst], one element per network call there,
 *       one strided kernel launch here (see iput_bytes / iget_bytes)
 *   shmem_<T>_p / _g   src/ptp/putget.c: a put or get of one element
 *
 * The remote side of put/get, and every collective's source, is symmetric:
 * in the device symmetric heap (shmemx_malloc_device), which peers read over
 * xGMI, or in shmem_malloc's symmetric host heap (hostheap.c), whose every
 * PE's segment is mapped in every PE, as the reference's segment exchange
 * makes them reachable (comms-inline.h:766-845). Host-heap objects move with
 * plain memory copies when the other side is host memory too (the
 * reference's transport does the same over GASNet), and with hipMemcpy when
 * it is device memory; everything else below is the device path. Local sides
 * may be any host or device memory. A put into
 * another GPU's memory goes through hipMemcpy on the peer-mapped pointer (the
 * HIP runtime's P2P copy contract makes the bytes visible to the peer's later
 * kernels; this library's kernels only ever write their own GPU's memory, so
 * no coherence question about a peer GPU's L2 arises); a put whose target is
 * on this GPU (a PE sharing it, or this PE) runs the copy kernel (a strided put:
 * the strided kernel; into another GPU's memory the kernel only packs the
 * elements and the runtime's 2-D copy places them). A get into device
 * memory, and every collective, PULLS with the streaming copy kernel: every
 * PE reads the members' sources over xGMI into its own target, between two
 * barriers -- the same producer/consumer pattern as the reduction's
 * all-gather leg. Host-memory local sides use hipMemcpy. Broadcast and
 * fcollect queue barrier, copies and barrier on the library stream (device
 * barriers, one host wait); collect exchanges its counts through the host
 * bootstrap segment and keeps host barriers.
 *
 * tests/test_datamove_cpu.py (host heap, no GPU) and tests/test_gpu_datamove.py
 * hold put / get, broadcast, fcollect and collect to the byte-exact model of
 * tests/_datamove_ref.py at every byte phase and size edge, and assert the
 * route or schedule each call takes.
 */
#define _GNU_SOURCE
#include <complex.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355_reduce.h"
#include "pshmem.h"
#include "shmem.h"
#include "shmemx.h"
#include "shmemi.h"

/* ---------------------------------------------------------------------- */
/* helpers                                                                 */
/* ---------------------------------------------------------------------- */
static void check_pe (const char *fn, int pe)
{
    if (pe < 0 || pe >= shmemi.npes)
        shmemi_fatal ("%s: PE %d outside 0..%d", fn, pe, shmemi.npes - 1);
}

/* Address of symmetric object `sym` (nbytes long) on PE `pe`: in the peer's
 * device heap, or in its host heap segment as mapped here. */
static void *remote_addr (const char *fn, const void *sym, size_t nbytes, int pe)
{
    if (pe == shmemi.mype)
        return (void *) sym;
    if (shmemi_in_device_heap (sym, nbytes))
        return shmemi_peer_ptr (pe, shmemi_heap_offset (sym));
    if (shmemi_in_host_heap (sym, nbytes))
        return shmemi_host_peer_ptr (pe, sym);
    shmemi_fatal ("%s: remote address %p is not symmetric (allocate it with shmem_malloc or "
                  "shmemx_malloc_device)", fn, sym);
}

static int is_device_ptr (const void *p);

/* p is host memory (no GPU at all: everything is) */
static int host_side (const void *p)
{
    return shmemi.heap == NULL || !is_device_ptr (p);
}

static void need_gpu (const char *fn)
{
    if (shmemi.heap == NULL)
        shmemi_fatal ("%s: no GPU (SHMEM_BOOTSTRAP_ONLY): only host-memory copies run without one", fn);
}

static void blocking_copy (void *dst, const void *src, size_t nbytes)
{
    if (nbytes == 0 || dst == src)
        return;
    SHMEMI_HIP (hipMemcpyAsync (dst, src, nbytes, hipMemcpyDefault, shmemi.stream));
    SHMEMI_HIP (hipStreamSynchronize (shmemi.stream));
}

static void pull (void **dsts, const void **srcs, size_t *nbytes, int nseg);

static void put_bytes (const char *fn, void *dest, const void *src, size_t nbytes, int pe)
{
    shmemi_init_check (fn);
    if (nbytes > 0 && (dest == NULL || src == NULL))
        shmemi_fatal ("%s: NULL %s (%zu bytes, PE %d)", fn, dest == NULL ? "dest" : "source", nbytes, pe);
    if (shmemi.heap != NULL)
        shmemi_server_stop ();
    check_pe (fn, pe);
    if (nbytes == 0)
        return;
    void *to = remote_addr (fn, dest, nbytes, pe);
    const int to_host = shmemi_in_host_heap (dest, nbytes) || (pe == shmemi.mype && host_side (dest));
    if (to_host && host_side (src)) {
        /* host memory both sides (a peer's host heap segment is mapped
         * here): the bytes are in place when memmove returns, and the
         * barriers' release/acquire make them visible to the peer */
        memmove (to, src, nbytes);
        return;
    }
    need_gpu (fn);
    const void *from = is_device_ptr (src) ? src : shmemi_host_dev_ptr (src, nbytes);
    if (!to_host && from != NULL && from != to && shmemi_pe_same_device (pe)) {
        /* target memory on this GPU (this PE's own heap, or a PE sharing the
         * GPU) <- device or page-locked host: the streaming copy kernel; the
         * call returns once every store has drained (local completion), and
         * shmem_quiet / the barriers wait for the kernel's end. A target on
         * ANOTHER GPU keeps the runtime's P2P copy below: this library's
         * kernels never write another GPU's memory (see the file header). */
        shmemi_order_after_caller (0);
        size_t nb = nbytes;
        shmemi_arm_signal ();
        const int rc = mi355_copy_segments (&to, &from, &nb, 1, shmemi.stream);
        if (rc != 0)
            shmemi_fatal ("%s: copy kernel launch failed: %d", fn, rc);
        shmemi_wait_signal ();
        return;
    }
    blocking_copy (to, src, nbytes);
}

static void get_bytes (const char *fn, void *dest, const void *src, size_t nbytes, int pe)
{
    shmemi_init_check (fn);
    if (nbytes > 0 && (dest == NULL || src == NULL))
        shmemi_fatal ("%s: NULL %s (%zu bytes, PE %d)", fn, dest == NULL ? "dest" : "source", nbytes, pe);
    if (shmemi.heap != NULL)
        shmemi_server_stop ();
    check_pe (fn, pe);
    if (nbytes == 0)
        return;
    const void *from = remote_addr (fn, src, nbytes, pe);
    const int from_host = shmemi_in_host_heap (src, nbytes) || (pe == shmemi.mype && host_side (src));
    if (from_host && host_side (dest)) {
        memmove (dest, from, nbytes);
        return;
    }
    need_gpu (fn);
    if (!from_host && is_device_ptr (dest) && dest != from) {
        /* device <- (peer) device: the streaming copy kernel pulls over xGMI
         * (2-3x the rate of hipMemcpy's D2D path, profiles/r01/coll_bench) */
        shmemi_order_after_caller (0);
        pull (&dest, &from, &nbytes, 1);
    } else {
        blocking_copy (dest, from, nbytes);
    }
}

/* ---------------------------------------------------------------------- */
/* put / get                                                               */
/* ---------------------------------------------------------------------- */
void pshmem_putmem (void *dest, const void *src, size_t nelems, int pe)
{
    put_bytes ("shmem_putmem", dest, src, nelems, pe);
}
void pshmem_getmem (void *dest, const void *src, size_t nelems, int pe)
{
    get_bytes ("shmem_getmem", dest, src, nelems, pe);
}
void pshmem_put32 (void *dest, const void *src, size_t nelems, int pe)
{
    put_bytes ("shmem_put32", dest, src, 4 * nelems, pe);
}
void pshmem_put64 (void *dest, const void *src, size_t nelems, int pe)
{
    put_bytes ("shmem_put64", dest, src, 8 * nelems, pe);
}
void pshmem_put128 (void *dest, const void *src, size_t nelems, int pe)
{
    put_bytes ("shmem_put128", dest, src, 16 * nelems, pe);
}
void pshmem_get32 (void *dest, const void *src, size_t nelems, int pe)
{
    get_bytes ("shmem_get32", dest, src, 4 * nelems, pe);
}
void pshmem_get64 (void *dest, const void *src, size_t nelems, int pe)
{
    get_bytes ("shmem_get64", dest, src, 8 * nelems, pe);
}
void pshmem_get128 (void *dest, const void *src, size_t nelems, int pe)
{
    get_bytes ("shmem_get128", dest, src, 16 * nelems, pe);
}

#define TYPED_PUTGET(Name, Type)                                                                    \
    void pshmem_##Name##_put (Type *dest, const Type *src, size_t nelems, int pe)                   \
    {                                                                                               \
        put_bytes ("shmem_" #Name "_put", dest, src, sizeof (Type) * nelems, pe);                  \
    }                                                                                               \
    void pshmem_##Name##_get (Type *dest, const Type *src, size_t nelems, int pe)                   \
    {                                                                                               \
        get_bytes ("shmem_" #Name "_get", dest, src, sizeof (Type) * nelems, pe);                  \
    }                                                                                               \
    void shmem_##Name##_put (Type *dest, const Type *src, size_t nelems, int pe)                    \
        __attribute__ ((weak, alias ("pshmem_" #Name "_put")));                                     \
    void shmem_##Name##_get (Type *dest, const Type *src, size_t nelems, int pe)                    \
        __attribute__ ((weak, alias ("pshmem_" #Name "_get")));

TYPED_PUTGET (char, char)
TYPED_PUTGET (short, short)
TYPED_PUTGET (int, int)
TYPED_PUTGET (long, long)
TYPED_PUTGET (longlong, long long)
TYPED_PUTGET (longdouble, long double)
TYPED_PUTGET (double, double)
TYPED_PUTGET (float, float)

/* ---------------------------------------------------------------------- */
/* collectives                                                             */
/* ---------------------------------------------------------------------- */
struct cset {
    int start, stride, size, me;
};

static struct cset make_set (const char *fn, int PE_start, int logPE_stride, int PE_size)
{
    shmemi_init_check (fn);
    if (shmemi.heap != NULL)
        shmemi_server_stop ();
    if (logPE_stride < 0 || logPE_stride > 30 || PE_size < 1 || PE_start < 0 ||
        PE_start + (long) (PE_size - 1) * (1L << logPE_stride) >= shmemi.npes)
        shmemi_fatal ("%s: active set (PE_start %d, logPE_stride %d, PE_size %d) outside the %d PEs", fn,
                      PE_start, logPE_stride, PE_size, shmemi.npes);
    struct cset s = {PE_start, 1 << logPE_stride, PE_size, -1};
    for (int i = 0; i < PE_size; ++i)
        if (PE_start + i * s.stride == shmemi.mype)
            s.me = i;
    if (s.me < 0)
        shmemi_fatal ("%s: PE %d is not in the active set (PE_start %d, logPE_stride %d, PE_size %d)", fn,
                      shmemi.mype, PE_start, logPE_stride, PE_size);
    return s;
}

static int is_device_ptr (const void *p)
{
    if (shmemi.heap == NULL)
        return 0;
    if (shmemi_in_device_heap (p, 0))
        return 1;
    hipPointerAttribute_t a;
    memset (&a, 0, sizeof a);
    hipError_t e = hipPointerGetAttributes (&a, p);
    (void) hipGetLastError ();
    return e == hipSuccess && (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged);
}

/* Pull nseg byte ranges of peers' symmetric HOST heap segments (mapped here)
 * into local memory: plain copies into host memory, hipMemcpy into device
 * memory (the GPU does not read the peers' segments: they are not
 * registered with this process's HIP). */
static void pull_host (const char *fn, void **dsts, const void **srcs, size_t *nbytes, int nseg)
{
    for (int i = 0; i < nseg; ++i) {
        if (nbytes[i] == 0)
            continue;
        if (host_side (dsts[i])) {
            memmove (dsts[i], srcs[i], nbytes[i]);
        } else {
            need_gpu (fn);
            SHMEMI_HIP (hipMemcpyAsync (dsts[i], srcs[i], nbytes[i], hipMemcpyDefault, shmemi.stream));
            SHMEMI_HIP (hipStreamSynchronize (shmemi.stream));
        }
    }
}

/* Pull nseg byte ranges from peers into local memory: one copy kernel when
 * the destination is device memory, DMA copies otherwise. wait: block until
 * done (the copy kernel's completion signal, or a stream synchronize);
 * otherwise only queue them on the library stream. */
static void pull_impl (void **dsts, const void **srcs, size_t *nbytes, int nseg, int wait)
{
    int dev = 1;
    for (int i = 0; i < nseg; ++i)
        dev &= is_device_ptr (dsts[i]);
    if (dev) {
        shmemi_peer_acquire (shmemi.stream); /* the sources are other PEs' memory */
        for (int base = 0; base < nseg; base += 64) {
            const int k = nseg - base < 64 ? nseg - base : 64;
            const int last = base + k == nseg;
            if (last && wait)
                shmemi_arm_signal ();
            int rc = mi355_copy_segments (dsts + base, srcs + base, nbytes + base, k, shmemi.stream);
            if (rc != 0)
                shmemi_fatal ("copy kernel launch failed: %d", rc);
        }
        if (wait)
            shmemi_wait_signal ();
    } else {
        for (int i = 0; i < nseg; ++i)
            if (nbytes[i] != 0)
                SHMEMI_HIP (hipMemcpyAsync (dsts[i], srcs[i], nbytes[i], hipMemcpyDefault, shmemi.stream));
        if (wait)
            SHMEMI_HIP (hipStreamSynchronize (shmemi.stream));
    }
}

static void pull (void **dsts, const void **srcs, size_t *nbytes, int nseg)
{
    pull_impl (dsts, srcs, nbytes, nseg, 1);
}

/* Opening barrier: every source is ready. With device barriers the rest of
 * the collective is queued behind it (dev = 1); else a host barrier after the
 * host has seen the caller's work done. */
/* 1: source in the symmetric host heap; 0: in the device heap (or nothing to
 * read); fatal otherwise */
static int source_kind (const char *fn, const void *source, size_t nbytes)
{
    if (nbytes == 0 || shmemi_in_device_heap (source, nbytes))
        return 0;
    if (shmemi_in_host_heap (source, nbytes))
        return 1;
    shmemi_fatal ("%s: source %p is not symmetric (allocate it with shmem_malloc or shmemx_malloc_device)", fn,
                  source);
}

/* PE pe's copy of a symmetric source (device or host heap) */
static const void *source_on (int pe, const void *source, int host)
{
    return host ? shmemi_host_peer_ptr (pe, source) : shmemi_peer_ptr (pe, shmemi_heap_offset (source));
}

static int collective_entry (const char *fn, const void *source, size_t nbytes, const struct cset *s,
                             int allow_dev)
{
    if (source_kind (fn, source, nbytes) != 0 || shmemi.heap == NULL)
        allow_dev = 0; /* the host heap: host barriers, the copies below run on the host */
    if (shmemi.heap == NULL) {
        shmemi_barrier_set (s->start, s->stride, s->size);
        return 0;
    }
    if (allow_dev && shmemi_dev_barrier_ok (s->start, s->stride, s->size)) {
        shmemi_order_after_caller (0); /* SHMEM_ENTRY_SYNC */
        shmemi_dev_barrier (s->start, s->stride, s->size, s->me, 0);
        return 1;
    }
    shmemi_order_after_caller (1);
    shmemi_barrier_set (s->start, s->stride, s->size);
    return 0;
}

/* Closing barrier: nobody reads this PE's source any more. */
static void collective_exit (const struct cset *s, int dev)
{
    if (dev)
        shmemi_dev_barrier (s->start, s->stride, s->size, s->me, 1);
    else
        shmemi_barrier_set (s->start, s->stride, s->size);
}

/* Small broadcast / fcollect in ONE launch (mi355_fused_pull): arrive, pull
 * this PE's segments, "done reading" -- instead of device barrier, copy
 * kernel and device barrier. The choice depends on the call's arguments only
 * (every member must make it alike); a member whose target the kernel cannot
 * write (pageable host memory) pulls into its scratch C and copies out. */
static int fused_pull_ok (const struct cset *s, size_t total)
{
    return shmemi.heap != NULL && s->size >= 2 && shmemi.fused_max != 0 && total <= shmemi.fused_max &&
           total <= shmemi.scratch_chunk && shmemi_dev_barrier_ok (s->start, s->stride, s->size);
}

/* segments: byte offsets into this PE's target of `total` bytes */
static void fused_pull (const char *fn, const struct cset *s, void *target, size_t total, const size_t *toff,
                        const void *const *srcs, const size_t *nb, int k)
{
    char *t = NULL;
    int copy_out = 0;
    if (total != 0) {
        t = is_device_ptr (target) ? (char *) target : (char *) shmemi_host_dev_ptr (target, total);
        if (t == NULL) {
            t = shmemi.heap + shmemi.scratch_off + 2 * shmemi.scratch_chunk; /* scratch C */
            copy_out = 1;
        }
    }
    MI355PullArgs p;
    memset (&p, 0, sizeof p);
    shmemi_member_args (&p.m, s->start, s->stride, s->size, s->me);
    p.nseg = k;
    for (int i = 0; i < k; ++i) {
        p.dst[i] = t + toff[i];
        p.src[i] = srcs[i];
        p.nbytes[i] = nb[i];
    }
    p.m.host_flag = shmemi.sig_flag;
    p.m.epoch = shmemi_next_epoch ();
    shmemi_order_after_caller (0); /* SHMEM_ENTRY_SYNC */
    const int rc = mi355_fused_pull (&p, shmemi.stream);
    if (rc != 0)
        shmemi_fatal ("%s: fused pull launch failed: %d", fn, rc);
    if (shmemi_wait_flag (p.m.epoch) != p.m.epoch)
        shmemi_fatal ("%s: timed out waiting for the other PEs of the active set", fn);
    if (copy_out)
        for (int i = 0; i < k; ++i)
            blocking_copy ((char *) target + toff[i], t + toff[i], nb[i]);
}

static void broadcast_bytes (const char *fn, void *target, const void *source, size_t nbytes, int PE_root,
                             int PE_start, int logPE_stride, int PE_size)
{
    struct cset s = make_set (fn, PE_start, logPE_stride, PE_size);
    if (PE_root < 0 || PE_root >= PE_size)
        shmemi_fatal ("%s: PE_root %d outside the active set of %d PEs", fn, PE_root, PE_size);
    const int root = PE_start + PE_root * s.stride;
    const int host = source_kind (fn, source, nbytes);
    if (s.size == 1)
        return; /* the root does not write its own target, and there is nobody to wait for */
    if (!host && fused_pull_ok (&s, nbytes)) {
        SHMEMI_TRACE (SHMEMI_LOG_BROADCAST, "%s: %zu bytes from PE %d, one fused launch", fn, nbytes, root);
        const void *src = nbytes != 0 ? shmemi_peer_ptr (root, shmemi_heap_offset (source)) : NULL;
        const size_t toff = 0;
        fused_pull (fn, &s, target, nbytes, &toff, &src, &nbytes, shmemi.mype != root && nbytes != 0 ? 1 : 0);
        return;
    }
    const int dev = collective_entry (fn, source, nbytes, &s, 1);
    if (shmemi.mype != root && nbytes != 0) {
        void *d = target;
        const void *src = source_on (root, source, host);
        if (host)
            pull_host (fn, &d, &src, &nbytes, 1);
        else
            pull_impl (&d, &src, &nbytes, 1, !dev);
    }
    collective_exit (&s, dev); /* nobody reads the root's source any more */
}

void pshmem_broadcast32 (void *target, const void *source, size_t nelems, int PE_root, int PE_start,
                         int logPE_stride, int PE_size, long *pSync)
{
    (void) pSync;
    broadcast_bytes ("shmem_broadcast32", target, source, 4 * nelems, PE_root, PE_start, logPE_stride, PE_size);
}

void pshmem_broadcast64 (void *target, const void *source, size_t nelems, int PE_root, int PE_start,
                         int logPE_stride, int PE_size, long *pSync)
{
    (void) pSync;
    broadcast_bytes ("shmem_broadcast64", target, source, 8 * nelems, PE_root, PE_start, logPE_stride, PE_size);
}

/* counts[i] bytes from member i land at the running offset in target */
static void gather_bytes (const char *fn, void *target, const void *source, const size_t *counts,
                          const struct cset *s, int wait, int host)
{
    void **dsts = (void **) malloc (sizeof (void *) * (size_t) s->size);
    const void **srcs = (const void **) malloc (sizeof (void *) * (size_t) s->size);
    size_t *nb = (size_t *) malloc (sizeof (size_t) * (size_t) s->size);
    if (dsts == NULL || srcs == NULL || nb == NULL)
        shmemi_fatal ("out of host memory");
    size_t off = 0;
    int k = 0;
    for (int i = 0; i < s->size; ++i) {
        const int pe = s->start + i * s->stride;
        if (counts[i] != 0) {
            dsts[k] = (char *) target + off;
            srcs[k] = source_on (pe, source, host);
            nb[k] = counts[i];
            ++k;
        }
        off += counts[i];
    }
    if (k > 0 && host)
        pull_host (fn, dsts, srcs, nb, k);
    else if (k > 0)
        pull_impl (dsts, srcs, nb, k, wait);
    free (nb);
    free (srcs);
    free (dsts);
}

static void fcollect_bytes (const char *fn, void *target, const void *source, size_t nbytes, int PE_start,
                            int logPE_stride, int PE_size)
{
    struct cset s = make_set (fn, PE_start, logPE_stride, PE_size);
    const int host = source_kind (fn, source, nbytes);
    if (s.size == 1) { /* one member: target = source, nobody to wait for */
        if (nbytes != 0 && target != source) {
            void *d = target;
            const void *src = source;
            if (host) {
                pull_host (fn, &d, &src, &nbytes, 1);
            } else {
                shmemi_order_after_caller (0);
                pull (&d, &src, &nbytes, 1);
            }
        }
        return;
    }
    if (!host && s.size <= MI355_PULL_MAX_SEGS && nbytes != 0 && fused_pull_ok (&s, nbytes * (size_t) s.size)) {
        size_t toff[MI355_PULL_MAX_SEGS], nb[MI355_PULL_MAX_SEGS];
        const void *srcs[MI355_PULL_MAX_SEGS];
        for (int i = 0; i < s.size; ++i) {
            toff[i] = (size_t) i * nbytes;
            srcs[i] = shmemi_peer_ptr (s.start + i * s.stride, shmemi_heap_offset (source));
            nb[i] = nbytes;
        }
        SHMEMI_TRACE (SHMEMI_LOG_COLLECT, "%s: %d x %zu bytes, one fused launch", fn, s.size, nbytes);
        fused_pull (fn, &s, target, nbytes * (size_t) s.size, toff, srcs, nb, s.size);
        return;
    }
    const int dev = collective_entry (fn, source, nbytes, &s, 1);
    size_t *counts = (size_t *) malloc (sizeof (size_t) * (size_t) s.size);
    if (counts == NULL)
        shmemi_fatal ("out of host memory");
    for (int i = 0; i < s.size; ++i)
        counts[i] = nbytes;
    gather_bytes (fn, target, source, counts, &s, !dev, host);
    free (counts);
    collective_exit (&s, dev); /* nobody reads our source any more */
}

void pshmem_fcollect32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                        int PE_size, long *pSync)
{
    (void) pSync;
    fcollect_bytes ("shmem_fcollect32", target, source, 4 * nelems, PE_start, logPE_stride, PE_size);
}

void pshmem_fcollect64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                        int PE_size, long *pSync)
{
    (void) pSync;
    fcollect_bytes ("shmem_fcollect64", target, source, 8 * nelems, PE_start, logPE_stride, PE_size);
}

/* collect: the per-PE byte counts travel through the bootstrap segment; the
 * closing barrier keeps a count alive until every member has read it */
static void collect_bytes (const char *fn, void *target, const void *source, size_t nbytes, int PE_start,
                           int logPE_stride, int PE_size)
{
    struct cset s = make_set (fn, PE_start, logPE_stride, PE_size);
    /* a member that contributes nothing still reads the others' sources: the
     * heap they are in is the heap of its own source pointer, whatever its
     * count (source_kind alone calls a source of 0 bytes device memory) */
    const int host = nbytes != 0 ? source_kind (fn, source, nbytes) : shmemi_in_host_heap (source, 0);
    shmemi_publish_count (nbytes);
    (void) collective_entry (fn, source, nbytes, &s, 0);
    size_t *counts = (size_t *) malloc (sizeof (size_t) * (size_t) s.size);
    if (counts == NULL)
        shmemi_fatal ("out of host memory");
    for (int i = 0; i < s.size; ++i)
        counts[i] = shmemi_peer_count (s.start + i * s.stride);
    if (nbytes == 0 && !host && !shmemi_in_device_heap (source, 0))
        for (int i = 0; i < s.size; ++i)
            if (counts[i] != 0)
                shmemi_fatal ("%s: source %p is not symmetric (allocate it with shmem_malloc or "
                              "shmemx_malloc_device)", fn, source);
    gather_bytes (fn, target, source, counts, &s, 1, host);
    free (counts);
    shmemi_barrier_set (s.start, s.stride, s.size);
}

void pshmem_collect32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync)
{
    (void) pSync;
    collect_bytes ("shmem_collect32", target, source, 4 * nelems, PE_start, logPE_stride, PE_size);
}

void pshmem_collect64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync)
{
    (void) pSync;
    collect_bytes ("shmem_collect64", target, source, 8 * nelems, PE_start, logPE_stride, PE_size);
}

/* ---------------------------------------------------------------------- */
/* all-to-all                                                              */
/* ---------------------------------------------------------------------- */
/* d[k * dst] = s[k * sst], k < n, in host memory (elements of es = 1, 2, 4, 8
 * or 16 bytes; a 16-byte element moves as bytes: shmem_iput128's pointers
 * promise no more than the caller's type does) */
static void host_strided_copy (void *d, const void *s, size_t es, ptrdiff_t dst, ptrdiff_t sst, size_t n)
{
    if (dst == 1 && sst == 1) {
        memmove (d, s, n * es);
        return;
    }
#define HOST_STRIDED(Type)                                                                          \
    for (size_t k = 0; k < n; ++k)                                                                  \
        ((Type *) d)[(ptrdiff_t) k * dst] = ((const Type *) s)[(ptrdiff_t) k * sst];
    switch (es) {
    case 1:
        HOST_STRIDED (uint8_t)
        break;
    case 2:
        HOST_STRIDED (uint16_t)
        break;
    case 4:
        HOST_STRIDED (uint32_t)
        break;
    case 8:
        HOST_STRIDED (uint64_t)
        break;
    default:
        for (size_t k = 0; k < n; ++k)
            memcpy ((char *) d + (ptrdiff_t) k * dst * 16, (const char *) s + (ptrdiff_t) k * sst * 16, 16);
        break;
    }
#undef HOST_STRIDED
}

/* k blocks of nelems elements into device memory: the copy kernel when both
 * strides are 1 (mi355_strided_copy hands those on), the strided kernel
 * otherwise, 64 blocks per launch. wait as in pull_impl. */
static void a2a_launch (const char *fn, int es, void **dsts, const void **srcs, ptrdiff_t dst, ptrdiff_t sst,
                        size_t nelems, int k, int wait)
{
    shmemi_peer_acquire (shmemi.stream); /* the sources are other PEs' memory */
    for (int base = 0; base < k; base += 64) {
        const int g = k - base < 64 ? k - base : 64;
        if (base + g == k && wait)
            shmemi_arm_signal ();
        shmemi_timed_begin ();
        const int rc = mi355_strided_copy (es, dsts + base, srcs + base, dst, sst, nelems, g, shmemi.stream);
        shmemi_timed_end ();
        if (rc != 0)
            shmemi_fatal ("%s: %s kernel launch failed: %d", fn, dst == 1 && sst == 1 ? "copy" : "strided", rc);
    }
    if (wait)
        shmemi_wait_signal ();
}

/* Strided blocks from device sources into HOST memory (the host heap or
 * pageable memory): the strided kernel packs as many blocks as fit into
 * scratch C, one copy brings them to the host, and host loops place the
 * elements dst apart -- the gap elements of the target are never written.
 * Returns with everything in place. */
static void a2a_staged (const char *fn, int es, void **dsts, const void **srcs, ptrdiff_t dst, ptrdiff_t sst,
                        size_t nelems, int k)
{
    char *scratch = shmemi.heap + shmemi.scratch_off + 2 * shmemi.scratch_chunk; /* scratch C */
    const size_t cap = shmemi.scratch_chunk / (size_t) es;                        /* elements per pass */
    if (cap == 0)
        shmemi_fatal ("%s: no device scratch to stage a host target through", fn);
    const size_t piece = nelems < cap ? nelems : cap; /* elements of one block per pass */
    size_t per = cap / piece;                         /* blocks per pass */
    if (per > 64)
        per = 64;
    char *tmp = (char *) malloc (per * piece * (size_t) es);
    if (tmp == NULL)
        shmemi_fatal ("out of host memory");
    shmemi_peer_acquire (shmemi.stream);
    for (size_t k0 = 0; k0 < nelems; k0 += piece) {
        const size_t cnt = nelems - k0 < piece ? nelems - k0 : piece;
        for (int base = 0; base < k; base += (int) per) {
            const int g = k - base < (int) per ? k - base : (int) per;
            void *pd[64];
            const void *ps[64];
            for (int j = 0; j < g; ++j) {
                pd[j] = scratch + (size_t) j * cnt * (size_t) es;
                ps[j] = (const char *) srcs[base + j] + (ptrdiff_t) k0 * sst * es;
            }
            const int rc = mi355_strided_copy (es, pd, ps, 1, sst, cnt, g, shmemi.stream);
            if (rc != 0)
                shmemi_fatal ("%s: strided kernel launch failed: %d", fn, rc);
            SHMEMI_HIP (hipMemcpyAsync (tmp, scratch, (size_t) g * cnt * (size_t) es, hipMemcpyDeviceToHost,
                                        shmemi.stream));
            SHMEMI_HIP (hipStreamSynchronize (shmemi.stream));
            for (int j = 0; j < g; ++j)
                host_strided_copy ((char *) dsts[base + j] + (ptrdiff_t) k0 * dst * es, tmp + (size_t) j * cnt * es,
                                   (size_t) es, dst, 1, cnt);
        }
    }
    free (tmp);
}

/* Blocks out of peers' symmetric HOST heap segments (the pull_host pattern):
 * host loops into host memory; into device memory a copy per block when both
 * sides are contiguous, else the elements packed on the host, copied to
 * scratch C and spread by the strided kernel. */
static void a2a_from_host (const char *fn, int es, void **dsts, const void **srcs, ptrdiff_t dst, ptrdiff_t sst,
                           size_t nelems, int k)
{
    if (host_side (dsts[0])) {
        for (int i = 0; i < k; ++i)
            host_strided_copy (dsts[i], srcs[i], (size_t) es, dst, sst, nelems);
        return;
    }
    need_gpu (fn);
    if (dst == 1 && sst == 1) {
        for (int i = 0; i < k; ++i)
            SHMEMI_HIP (hipMemcpyAsync (dsts[i], srcs[i], nelems * (size_t) es, hipMemcpyDefault, shmemi.stream));
        SHMEMI_HIP (hipStreamSynchronize (shmemi.stream));
        return;
    }
    char *scratch = shmemi.heap + shmemi.scratch_off + 2 * shmemi.scratch_chunk; /* scratch C */
    const size_t cap = shmemi.scratch_chunk / (size_t) es;
    if (cap == 0)
        shmemi_fatal ("%s: no device scratch to stage a host source through", fn);
    const size_t piece = nelems < cap ? nelems : cap;
    char *tmp = (char *) malloc (piece * (size_t) es);
    if (tmp == NULL)
        shmemi_fatal ("out of host memory");
    for (int i = 0; i < k; ++i)
        for (size_t k0 = 0; k0 < nelems; k0 += piece) {
            const size_t cnt = nelems - k0 < piece ? nelems - k0 : piece;
            host_strided_copy (tmp, (const char *) srcs[i] + (ptrdiff_t) k0 * sst * es, (size_t) es, 1, sst, cnt);
            void *d = (char *) dsts[i] + (ptrdiff_t) k0 * dst * es;
            if (dst == 1) {
                SHMEMI_HIP (hipMemcpyAsync (d, tmp, cnt * (size_t) es, hipMemcpyHostToDevice, shmemi.stream));
            } else {
                const void *sc = scratch;
                SHMEMI_HIP (hipMemcpyAsync (scratch, tmp, cnt * (size_t) es, hipMemcpyHostToDevice, shmemi.stream));
                const int rc = mi355_strided_copy (es, &d, &sc, dst, 1, cnt, 1, shmemi.stream);
                if (rc != 0)
                    shmemi_fatal ("%s: strided kernel launch failed: %d", fn, rc);
            }
            SHMEMI_HIP (hipStreamSynchronize (shmemi.stream)); /* tmp and scratch are reused */
        }
    free (tmp);
}

/* target_on_m[(i*nelems + k) * dst] = source_on_i[(m*nelems + k) * sst] for
 * member i < N, k < nelems, m this PE's index IN THE ACTIVE SET.
 *
 * Reference: src/alltoall/alltoall.c, alltoall-linear.c:60-84 (one
 * shmem_iget or shmem_getmem per member, then shmem_quiet). One deliberate
 * deviation: alltoall-linear.c:74,78 offsets the source by the GLOBAL PE
 * number (GET_STATE (mype)); that equals the index in the set only for the
 * set (0, 0, N), and for any other set reads outside the block layout
 * OpenSHMEM 1.3 defines. This build implements the specification's meaning;
 * on (0, 0, N) the result is the reference's bit for bit.
 *
 * Every member pulls, so the call is bracketed like fcollect_bytes: an
 * opening barrier (every source is ready) and a closing one (nobody still
 * reads my source) -- the reference needs neither more than its quiet, its
 * gets being blocking and its callers synchronising around the call. Small
 * contiguous calls run as one mi355_fused_pull launch under fcollect's
 * conditions. */
static void alltoall_bytes (const char *fn, int es, void *target, const void *source, ptrdiff_t dst, ptrdiff_t sst,
                            size_t nelems, int PE_start, int logPE_stride, int PE_size)
{
    struct cset s = make_set (fn, PE_start, logPE_stride, PE_size);
    if (dst < 1 || sst < 1)
        shmemi_fatal ("%s: strides dst %td, sst %td: both must be at least 1", fn, dst, sst);
    const size_t N = (size_t) s.size, ue = (size_t) es;
    const size_t sspan = nelems == 0 ? 0 : ((N * nelems - 1) * (size_t) sst + 1) * ue; /* bytes of source read */
    const int host = source_kind (fn, source, sspan);
    if (nelems != 0 && target == NULL)
        shmemi_fatal ("%s: NULL target (%zu elements)", fn, nelems);
    const int contig = dst == 1 && sst == 1;
    const size_t nb = nelems * ue;
    if (!host && contig && s.size >= 2 && s.size <= MI355_PULL_MAX_SEGS && nb != 0 && fused_pull_ok (&s, nb * N)) {
        size_t toff[MI355_PULL_MAX_SEGS], nbs[MI355_PULL_MAX_SEGS];
        const void *srcs[MI355_PULL_MAX_SEGS];
        for (int i = 0; i < s.size; ++i) {
            toff[i] = (size_t) i * nb;
            srcs[i] = (const char *) shmemi_peer_ptr (s.start + i * s.stride, shmemi_heap_offset (source)) +
                      (size_t) s.me * nb;
            nbs[i] = nb;
        }
        SHMEMI_TRACE (SHMEMI_LOG_ALLTOALL, "%s: %d x %zu bytes, one fused launch", fn, s.size, nb);
        fused_pull (fn, &s, target, nb * N, toff, srcs, nbs, s.size);
        return;
    }
    int dev = 0;
    if (s.size > 1)
        dev = collective_entry (fn, source, sspan, &s, 1);
    else if (!host && nelems != 0)
        shmemi_order_after_caller (0); /* one member: a local copy, nobody to wait for */
    if (nelems != 0) {
        void **dsts = (void **) malloc (sizeof (void *) * N);
        const void **srcs = (const void **) malloc (sizeof (void *) * N);
        if (dsts == NULL || srcs == NULL)
            shmemi_fatal ("out of host memory");
        for (int i = 0; i < s.size; ++i) {
            const int pe = s.start + i * s.stride;
            dsts[i] = (char *) target + (ptrdiff_t) ((size_t) i * nelems) * dst * es;
            srcs[i] = (const char *) source_on (pe, source, host) + (ptrdiff_t) ((size_t) s.me * nelems) * sst * es;
        }
        if (host) {
            SHMEMI_TRACE (SHMEMI_LOG_ALLTOALL, "%s: %d x %zu elements of %d bytes, strides %td/%td, host", fn, s.size,
                          nelems, es, dst, sst);
            a2a_from_host (fn, es, dsts, srcs, dst, sst, nelems, s.size);
        } else if (is_device_ptr (target)) {
            SHMEMI_TRACE (SHMEMI_LOG_ALLTOALL, "%s: %d x %zu elements of %d bytes, strides %td/%td, %s kernel", fn,
                          s.size, nelems, es, dst, sst, contig ? "copy" : "strided");
            a2a_launch (fn, es, dsts, srcs, dst, sst, nelems, s.size, !dev);
        } else if (contig) {
            SHMEMI_TRACE (SHMEMI_LOG_ALLTOALL, "%s: %d x %zu bytes into host memory, copies", fn, s.size, nb);
            size_t *nbs = (size_t *) malloc (sizeof (size_t) * N);
            if (nbs == NULL)
                shmemi_fatal ("out of host memory");
            for (int i = 0; i < s.size; ++i)
                nbs[i] = nb;
            pull_impl (dsts, srcs, nbs, s.size, !dev);
            free (nbs);
        } else {
            SHMEMI_TRACE (SHMEMI_LOG_ALLTOALL,
                          "%s: %d x %zu elements of %d bytes, strides %td/%td, strided kernel staged into host memory",
                          fn, s.size, nelems, es, dst, sst);
            a2a_staged (fn, es, dsts, srcs, dst, sst, nelems, s.size);
        }
        free (srcs);
        free (dsts);
    }
    if (s.size > 1)
        collective_exit (&s, dev); /* nobody reads our source any more */
}

void pshmem_alltoall32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                        int PE_size, long *pSync)
{
    (void) pSync;
    alltoall_bytes ("shmem_alltoall32", 4, target, source, 1, 1, nelems, PE_start, logPE_stride, PE_size);
}

void pshmem_alltoall64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                        int PE_size, long *pSync)
{
    (void) pSync;
    alltoall_bytes ("shmem_alltoall64", 8, target, source, 1, 1, nelems, PE_start, logPE_stride, PE_size);
}

void pshmem_alltoalls32 (void *target, const void *source, ptrdiff_t dst, ptrdiff_t sst, size_t nelems,
                         int PE_start, int logPE_stride, int PE_size, long *pSync)
{
    (void) pSync;
    alltoall_bytes ("shmem_alltoalls32", 4, target, source, dst, sst, nelems, PE_start, logPE_stride, PE_size);
}

void pshmem_alltoalls64 (void *target, const void *source, ptrdiff_t dst, ptrdiff_t sst, size_t nelems,
                         int PE_start, int logPE_stride, int PE_size, long *pSync)
{
    (void) pSync;
    alltoall_bytes ("shmem_alltoalls64", 8, target, source, dst, sst, nelems, PE_start, logPE_stride, PE_size);
}

/* ---------------------------------------------------------------------- */
/* strided put / get                                                       */
/* ---------------------------------------------------------------------- */
/* target[k * tst] = source[k * sst] for k < nelems, elements of es = 1, 2, 4,
 * 8 or 16 bytes, one side symmetric on PE pe (device heap or host heap).
 *
 * Reference: src/ptp/strided.c:110-238, one shmem_<T>_p / _g network call per
 * element in a host loop. Here a call is one launch of the strided kernel
 * (mi355_strided_copy) wherever the GPU reaches both sides, host loops where
 * both are host memory, and the all-to-all's single-block paths (a2a_launch,
 * a2a_staged, a2a_from_host) in between. Both calls block like put_bytes /
 * get_bytes: on return a get's data is in place, a put's source may be reused
 * and its target is written. Elements between and after the strided ones are
 * never written. */
static void strided_entry (const char *fn, const void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst,
                           size_t nelems, int pe)
{
    shmemi_init_check (fn);
    if (tst < 1 || sst < 1)
        shmemi_fatal ("%s: strides tst %td, sst %td: both must be at least 1", fn, tst, sst);
    if (nelems > 0 && (target == NULL || source == NULL))
        shmemi_fatal ("%s: NULL %s (%zu elements, PE %d)", fn, target == NULL ? "target" : "source", nelems, pe);
    if (shmemi.heap != NULL)
        shmemi_server_stop ();
    check_pe (fn, pe);
}

/* bytes from the first to the last element touched */
static size_t strided_span (size_t nelems, ptrdiff_t stride, int es)
{
    return ((nelems - 1) * (size_t) stride + 1) * (size_t) es;
}

/* one block through the strided kernel (the copy kernel for strides 1, 1),
 * returning when its stores have drained */
static void strided_kernel (const char *fn, int es, void *d, const void *s, ptrdiff_t tst, ptrdiff_t sst, size_t n)
{
    if (d == s && tst == sst)
        return;
    shmemi_arm_signal ();
    const int rc = mi355_strided_copy (es, &d, &s, tst, sst, n, 1, shmemi.stream);
    if (rc != 0)
        shmemi_fatal ("%s: %s kernel launch failed: %d", fn, tst == 1 && sst == 1 ? "copy" : "strided", rc);
    shmemi_wait_signal ();
}

static void iget_bytes (const char *fn, int es, void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst,
                        size_t nelems, int pe)
{
    strided_entry (fn, target, source, tst, sst, nelems, pe);
    if (nelems == 0)
        return;
    const size_t sspan = strided_span (nelems, sst, es);
    const void *from = remote_addr (fn, source, sspan, pe);
    const int from_host = shmemi_in_host_heap (source, sspan) || (pe == shmemi.mype && host_side (source));
    void *d = target;
    if (from_host) {
        /* a host heap segment (mapped here) or this PE's own host memory:
         * host loops into host memory; into device memory packed on the host
         * and spread by the kernel */
        a2a_from_host (fn, es, &d, &from, tst, sst, nelems, 1);
        return;
    }
    need_gpu (fn);
    shmemi_order_after_caller (0);
    if (is_device_ptr (target)) {
        if (target != from || tst != sst)
            a2a_launch (fn, es, &d, &from, tst, sst, nelems, 1, 1);
    } else if (tst == 1 && sst == 1) {
        blocking_copy (target, from, nelems * (size_t) es);
    } else {
        a2a_staged (fn, es, &d, &from, tst, sst, nelems, 1);
    }
}

/* A strided put into ANOTHER GPU's memory. This library's kernels never write
 * another GPU's memory (the file header), so the kernel only packs: pieces of
 * at most one scratch chunk are gathered contiguously into scratch C
 * (dst_stride 1; a pageable source is packed on the host and copied in), and
 * the runtime's copy places each piece on the peer-mapped pointer -- a 2-D
 * copy of `cnt` rows of one element, tst elements apart, or a plain copy when
 * tst is 1. SHMEM_TEST_IPUT_REMOTE_GPU=1 sends same-GPU targets here (tests). */
static void iput_remote_gpu (const char *fn, int es, char *to, const void *source, ptrdiff_t tst, ptrdiff_t sst,
                             size_t nelems)
{
    const size_t ue = (size_t) es;
    char *scratch = shmemi.heap + shmemi.scratch_off + 2 * shmemi.scratch_chunk; /* scratch C */
    const size_t cap = shmemi.scratch_chunk / ue;                                 /* elements per piece */
    if (cap == 0)
        shmemi_fatal ("%s: no device scratch to pack a put to another GPU in", fn);
    const size_t piece = nelems < cap ? nelems : cap;
    const char *from = is_device_ptr (source)
                           ? (const char *) source
                           : (const char *) shmemi_host_dev_ptr (source, strided_span (nelems, sst, es));
    char *tmp = NULL;
    if (from == NULL && sst != 1 && (tmp = (char *) malloc (piece * ue)) == NULL)
        shmemi_fatal ("out of host memory");
    for (size_t k0 = 0; k0 < nelems; k0 += piece) {
        const size_t cnt = nelems - k0 < piece ? nelems - k0 : piece;
        const ptrdiff_t soff = (ptrdiff_t) k0 * sst * es;
        const void *packed = scratch;
        if (sst == 1) {
            packed = (const char *) source + soff; /* contiguous already */
        } else if (from != NULL) {
            void *pd = scratch;
            const void *ps = from + soff;
            const int rc = mi355_strided_copy (es, &pd, &ps, 1, sst, cnt, 1, shmemi.stream);
            if (rc != 0)
                shmemi_fatal ("%s: strided kernel launch failed: %d", fn, rc);
        } else {
            host_strided_copy (tmp, (const char *) source + soff, ue, 1, sst, cnt);
            SHMEMI_HIP (hipMemcpyAsync (scratch, tmp, cnt * ue, hipMemcpyHostToDevice, shmemi.stream));
        }
        char *d = to + (ptrdiff_t) k0 * tst * es;
        if (tst == 1)
            SHMEMI_HIP (hipMemcpyAsync (d, packed, cnt * ue, hipMemcpyDefault, shmemi.stream));
        else
            SHMEMI_HIP (hipMemcpy2DAsync (d, (size_t) tst * ue, packed, ue, ue, cnt, hipMemcpyDefault, shmemi.stream));
        SHMEMI_HIP (hipStreamSynchronize (shmemi.stream)); /* tmp and scratch are reused */
    }
    free (tmp);
}

static int iput_test_remote_gpu (void)
{
    static int v = -1;
    if (v < 0) {
        const char *e = getenv ("SHMEM_TEST_IPUT_REMOTE_GPU");
        v = e != NULL && e[0] == '1';
    }
    return v;
}

static void iput_bytes (const char *fn, int es, void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst,
                        size_t nelems, int pe)
{
    strided_entry (fn, target, source, tst, sst, nelems, pe);
    if (nelems == 0)
        return;
    const size_t tspan = strided_span (nelems, tst, es), sspan = strided_span (nelems, sst, es);
    void *to = remote_addr (fn, target, tspan, pe);
    const int to_host = shmemi_in_host_heap (target, tspan) || (pe == shmemi.mype && host_side (target));
    if (to_host && host_side (source)) {
        /* host memory both sides (a peer's host heap segment is mapped here):
         * in place on return, visible to the peer after the next barrier */
        host_strided_copy (to, source, (size_t) es, tst, sst, nelems);
        return;
    }
    need_gpu (fn);
    shmemi_order_after_caller (0);
    if (to_host) {
        /* device source into host memory: packed by the kernel, copied out, spread on the host */
        if (tst == 1 && sst == 1)
            blocking_copy (to, source, nelems * (size_t) es);
        else
            a2a_staged (fn, es, &to, &source, tst, sst, nelems, 1);
        return;
    }
    if (!shmemi_pe_same_device (pe) || iput_test_remote_gpu ()) {
        iput_remote_gpu (fn, es, (char *) to, source, tst, sst, nelems);
        return;
    }
    /* target on this GPU (this PE's heap, or a PE sharing the GPU): the kernel
     * writes the peer mapping; page-locked host sources go in through their
     * device address, pageable ones are packed on the host and staged */
    const void *from = is_device_ptr (source) ? source : shmemi_host_dev_ptr (source, sspan);
    if (from != NULL)
        strided_kernel (fn, es, to, from, tst, sst, nelems);
    else
        a2a_from_host (fn, es, &to, &source, tst, sst, nelems, 1);
}

#define STRIDED_PUTGET(Name, Type, Size)                                                            \
    void pshmem_##Name##_iput (Type *target, const Type *source, ptrdiff_t tst, ptrdiff_t sst,      \
                               size_t nelems, int pe)                                               \
    {                                                                                               \
        iput_bytes ("shmem_" #Name "_iput", Size, target, source, tst, sst, nelems, pe);           \
    }                                                                                               \
    void pshmem_##Name##_iget (Type *target, const Type *source, ptrdiff_t tst, ptrdiff_t sst,      \
                               size_t nelems, int pe)                                               \
    {                                                                                               \
        iget_bytes ("shmem_" #Name "_iget", Size, target, source, tst, sst, nelems, pe);           \
    }                                                                                               \
    void shmem_##Name##_iput (Type *target, const Type *source, ptrdiff_t tst, ptrdiff_t sst,       \
                              size_t nelems, int pe)                                                \
        __attribute__ ((weak, alias ("pshmem_" #Name "_iput")));                                    \
    void shmem_##Name##_iget (Type *target, const Type *source, ptrdiff_t tst, ptrdiff_t sst,       \
                              size_t nelems, int pe)                                                \
        __attribute__ ((weak, alias ("pshmem_" #Name "_iget")));

STRIDED_PUTGET (char, char, 1)
STRIDED_PUTGET (short, short, (int) sizeof (short))
STRIDED_PUTGET (int, int, (int) sizeof (int))
STRIDED_PUTGET (long, long, (int) sizeof (long))
STRIDED_PUTGET (longlong, long long, (int) sizeof (long long))
STRIDED_PUTGET (float, float, (int) sizeof (float))
STRIDED_PUTGET (double, double, (int) sizeof (double))
STRIDED_PUTGET (longdouble, long double, (int) sizeof (long double))

#define SIZED_IPUTGET(Bits)                                                                         \
    void pshmem_iput##Bits (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst,         \
                            size_t nelems, int pe)                                                  \
    {                                                                                               \
        iput_bytes ("shmem_iput" #Bits, Bits / 8, target, source, tst, sst, nelems, pe);           \
    }                                                                                               \
    void pshmem_iget##Bits (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst,         \
                            size_t nelems, int pe)                                                  \
    {                                                                                               \
        iget_bytes ("shmem_iget" #Bits, Bits / 8, target, source, tst, sst, nelems, pe);           \
    }                                                                                               \
    void shmem_iput##Bits (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst,          \
                           size_t nelems, int pe)                                                   \
        __attribute__ ((weak, alias ("pshmem_iput" #Bits)));                                        \
    void shmem_iget##Bits (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst,          \
                           size_t nelems, int pe)                                                   \
        __attribute__ ((weak, alias ("pshmem_iget" #Bits)));

SIZED_IPUTGET (32)
SIZED_IPUTGET (64)
SIZED_IPUTGET (128)

/* single elements (reference src/ptp/putget.c shmem_<T>_p / _g): a put or
 * get of one element; the strided calls above are NOT built from them */
#define SINGLE_PG(Name, Type)                                                                       \
    void pshmem_##Name##_p (Type *addr, Type value, int pe)                                         \
    {                                                                                               \
        put_bytes ("shmem_" #Name "_p", addr, &value, sizeof (Type), pe);                          \
    }                                                                                               \
    Type pshmem_##Name##_g (Type *addr, int pe)                                                     \
    {                                                                                               \
        Type value;                                                                                 \
        memset (&value, 0, sizeof value);                                                           \
        get_bytes ("shmem_" #Name "_g", &value, addr, sizeof (Type), pe);                          \
        return value;                                                                               \
    }                                                                                               \
    void shmem_##Name##_p (Type *addr, Type value, int pe)                                          \
        __attribute__ ((weak, alias ("pshmem_" #Name "_p")));                                       \
    Type shmem_##Name##_g (Type *addr, int pe) __attribute__ ((weak, alias ("pshmem_" #Name "_g")));

SINGLE_PG (char, char)
SINGLE_PG (short, short)
SINGLE_PG (int, int)
SINGLE_PG (long, long)
SINGLE_PG (longlong, long long)
SINGLE_PG (float, float)
SINGLE_PG (double, double)
SINGLE_PG (longdouble, long double)

#define WEAK(name) __attribute__ ((weak, alias ("p" #name)))
void shmem_putmem (void *dest, const void *src, size_t nelems, int pe) WEAK (shmem_putmem);
void shmem_getmem (void *dest, const void *src, size_t nelems, int pe) WEAK (shmem_getmem);
void shmem_put32 (void *dest, const void *src, size_t nelems, int pe) WEAK (shmem_put32);
void shmem_put64 (void *dest, const void *src, size_t nelems, int pe) WEAK (shmem_put64);
void shmem_put128 (void *dest, const void *src, size_t nelems, int pe) WEAK (shmem_put128);
void shmem_get32 (void *dest, const void *src, size_t nelems, int pe) WEAK (shmem_get32);
void shmem_get64 (void *dest, const void *src, size_t nelems, int pe) WEAK (shmem_get64);
void shmem_get128 (void *dest, const void *src, size_t nelems, int pe) WEAK (shmem_get128);
void shmem_broadcast32 (void *target, const void *source, size_t nelems, int PE_root, int PE_start,
                        int logPE_stride, int PE_size, long *pSync) WEAK (shmem_broadcast32);
void shmem_broadcast64 (void *target, const void *source, size_t nelems, int PE_root, int PE_start,
                        int logPE_stride, int PE_size, long *pSync) WEAK (shmem_broadcast64);
void shmem_fcollect32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync) WEAK (shmem_fcollect32);
void shmem_fcollect64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync) WEAK (shmem_fcollect64);
void shmem_collect32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                      int PE_size, long *pSync) WEAK (shmem_collect32);
void shmem_collect64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                      int PE_size, long *pSync) WEAK (shmem_collect64);
void shmem_alltoall32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync) WEAK (shmem_alltoall32);
void shmem_alltoall64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync) WEAK (shmem_alltoall64);
void shmem_alltoalls32 (void *target, const void *source, ptrdiff_t dst, ptrdiff_t sst, size_t nelems,
                        int PE_start, int logPE_stride, int PE_size, long *pSync) WEAK (shmem_alltoalls32);
void shmem_alltoalls64 (void *target, const void *source, ptrdiff_t dst, ptrdiff_t sst, size_t nelems,
                        int PE_start, int logPE_stride, int PE_size, long *pSync) WEAK (shmem_alltoalls64);
