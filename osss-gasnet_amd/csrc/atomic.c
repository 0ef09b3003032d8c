/*
 * atomic.c -- remote atomics, point-to-point waits and locks (the reference's
 * src/atomic/atomic.c, waituntil.c and lock.c), and the atomic accumulate
 * extension shmemx_<T>_atomic_add_v.
 *
 * A symmetric object lives in exactly one heap, so all its atomics take one
 * path and are mutually atomic:
 *   device heap   one mi355_amo launch (amo.hip: a system-scope atomic by one
 *                 lane on the target PE's heap as mapped here) on the library
 *                 stream, behind the caller's earlier work; the call waits for
 *                 the launch and reads the old value from a host-coherent slot
 *   host heap     an __atomic_* builtin with __ATOMIC_SEQ_CST on the target
 *                 PE's segment as mapped here (hostheap.c); no GPU involved,
 *                 so this path also runs under SHMEM_BOOTSTRAP_ONLY
 * pe == this PE takes the same paths. Every atomic, fetching or not, is
 * complete at the target when the call returns (OpenSHMEM allows an
 * implementation to complete them early), which leaves shmem_fence and
 * shmem_quiet nothing to do beyond a synchronise of the library stream.
 *
 * The reference sends each atomic as an active message whose handler runs on
 * the target PE under a lock (atomic.c, comms); here the target PE takes no
 * part. Arithmetic is on unsigned integers of the width (wrap-around, no
 * signed overflow in the library); the float and double forms of swap, fetch
 * and set move bit patterns.
 *
 * Waits are host loops: no kernel polls (a kernel waiting on another process
 * would hold its CU while the process that must release it may need the same
 * GPU; DESIGN.md section 5, "Atomics, waits, locks"). A host-heap variable is
 * polled with atomic loads of its own width; a device-heap one is fetched
 * with mi355_amo's FETCH (a 16-bit one with a 2-byte copy into the
 * host-coherent slot), compared on the host, and the loop backs off. Both are
 * bounded by SHMEM_WAIT_TIMEOUT.
 *
 * Locks: a ticket lock in the two 32-bit halves of the lock's `long`, acting
 * on the copy at the lock's home PE ((offset in its heap / 8) mod PEs, so
 * that a program's locks spread over the PEs): the low half is the next
 * ticket, the high half the ticket being served; both start at 0 and wrap.
 *   set_lock     ticket = fadd (next, 1); fetch serving until it is ticket
 *   clear_lock   quiet (the holder's puts are visible first); add (serving, 1)
 *   test_lock    s = fetch (serving); taken iff cswap (next, s, s + 1) == s
 *                (serving <= next and serving only grows, so next == s proves
 *                nobody holds or waits); never blocks
 * Only 32-bit operations touch the word, so no two widths meet on it. The
 * reference's MCS-style queue (lock.c) also splits the long; a ticket lock
 * needs no per-PE node and is fair.
 */
#define _GNU_SOURCE
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mi355_reduce.h"
#include "pshmem.h"
#include "shmem.h"
#include "shmemx.h"
#include "shmemi.h"

enum { AT_HOST = 0, AT_DEV = 1 };

static void check_pe (const char *fn, int pe)
{
    if (pe < 0 || pe >= shmemi.npes)
        shmemi_fatal ("%s: PE %d outside 0..%d", fn, pe, shmemi.npes - 1);
}

/* Which heap holds the symmetric object `sym` (nbytes long, aligned to
 * `align`), and its address on PE `pe`. Anything else aborts by name. */
static int locate (const char *fn, const void *sym, size_t nbytes, size_t align, int pe, void **addr)
{
    shmemi_init_check (fn);
    check_pe (fn, pe);
    if (sym == NULL)
        shmemi_fatal ("%s: NULL symmetric address (PE %d)", fn, pe);
    if (((uintptr_t) sym & (align - 1)) != 0)
        shmemi_fatal ("%s: address %p is not aligned to its %zu-byte type", fn, sym, align);
    if (shmemi_in_device_heap (sym, nbytes)) {
        *addr = pe == shmemi.mype ? (void *) sym : shmemi_peer_ptr (pe, shmemi_heap_offset (sym));
        return AT_DEV;
    }
    if (shmemi_in_host_heap (sym, nbytes)) {
        *addr = shmemi_host_peer_ptr (pe, sym);
        return AT_HOST;
    }
    shmemi_fatal ("%s: address %p is in neither symmetric heap (allocate it with shmem_malloc or "
                  "shmemx_malloc_device)", fn, sym);
}

static const char *const op_names[MI355_NUM_AMO_OPS] = {"swap", "cswap", "fadd", "fetch", "set"};

static uint64_t host_amo (int op, int width, void *addr, uint64_t value, uint64_t cond)
{
    if (width == 4) {
        uint32_t *p = (uint32_t *) addr, c = (uint32_t) cond;
        switch (op) {
        case MI355_AMO_SWAP: return __atomic_exchange_n (p, (uint32_t) value, __ATOMIC_SEQ_CST);
        case MI355_AMO_CSWAP:
            (void) __atomic_compare_exchange_n (p, &c, (uint32_t) value, 0, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
            return c;
        case MI355_AMO_FADD: return __atomic_fetch_add (p, (uint32_t) value, __ATOMIC_SEQ_CST);
        case MI355_AMO_FETCH: return __atomic_load_n (p, __ATOMIC_SEQ_CST);
        default: __atomic_store_n (p, (uint32_t) value, __ATOMIC_SEQ_CST); return 0;
        }
    }
    uint64_t *p = (uint64_t *) addr, c = cond;
    switch (op) {
    case MI355_AMO_SWAP: return __atomic_exchange_n (p, value, __ATOMIC_SEQ_CST);
    case MI355_AMO_CSWAP:
        (void) __atomic_compare_exchange_n (p, &c, value, 0, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
        return c;
    case MI355_AMO_FADD: return __atomic_fetch_add (p, value, __ATOMIC_SEQ_CST);
    case MI355_AMO_FETCH: return __atomic_load_n (p, __ATOMIC_SEQ_CST);
    default: __atomic_store_n (p, value, __ATOMIC_SEQ_CST); return 0;
    }
}

/* One launch on the library stream, ordered after the caller's work like the
 * other point-to-point calls; returns once the operation is done at the
 * target and its old value is in the slot. */
static uint64_t dev_amo (const char *fn, int op, int width, void *addr, uint64_t value, uint64_t cond)
{
    shmemi_server_stop ();
    shmemi_order_after_caller (0);
    shmemi_arm_signal ();
    shmemi_timed_begin ();
    const int rc = mi355_amo (op, width, addr, value, cond, shmemi.amo_slot, shmemi.stream);
    shmemi_timed_end ();
    if (rc != 0)
        shmemi_fatal ("%s: atomic kernel launch failed: %d", fn, rc);
    shmemi_wait_signal ();
    return __atomic_load_n (shmemi.amo_slot, __ATOMIC_ACQUIRE);
}

static uint64_t amo (const char *fn, int op, int width, const void *target, uint64_t value, uint64_t cond, int pe)
{
    void *addr = NULL;
    const int where = locate (fn, target, (size_t) width, (size_t) width, pe, &addr);
    const uint64_t old = where == AT_HOST ? host_amo (op, width, addr, value, cond)
                                          : dev_amo (fn, op, width, addr, value, cond);
    SHMEMI_TRACE (SHMEMI_LOG_ATOMIC, "%s(%p, PE %d): %s of %d bytes in the %s heap, value %#llx, old %#llx", fn, target,
                  pe, op_names[op], width, where == AT_HOST ? "host" : "device", (unsigned long long) value,
                  (unsigned long long) old);
    return old;
}

/* ---------------------------------------------------------------------- */
/* the typed entry points                                                  */
/* ---------------------------------------------------------------------- */
/* bit patterns in and out: memcpy, never a conversion */
#define TO_BITS(Type, v) __extension__({ uint64_t b_ = 0; Type v_ = (v); memcpy (&b_, &v_, sizeof v_); b_; })
#define FROM_BITS(Type, b) __extension__({ uint64_t b_ = (b); Type v_; memcpy (&v_, &b_, sizeof v_); v_; })
#define ALIAS(Ret, Name, Args) Ret shmem_##Name Args __attribute__ ((weak, alias ("pshmem_" #Name)));

#define AMO_SWAP_FETCH_SET(Name, Type)                                                              \
    Type pshmem_##Name##_swap (Type *target, Type value, int pe)                                    \
    {                                                                                               \
        return FROM_BITS (Type, amo ("shmem_" #Name "_swap", MI355_AMO_SWAP, (int) sizeof (Type), target,    \
                                     TO_BITS (Type, value), 0, pe));                                \
    }                                                                                               \
    Type pshmem_##Name##_fetch (const Type *dest, int pe)                                           \
    {                                                                                               \
        return FROM_BITS (Type, amo ("shmem_" #Name "_fetch", MI355_AMO_FETCH, (int) sizeof (Type), dest, 0, \
                                     0, pe));                                                       \
    }                                                                                               \
    void pshmem_##Name##_set (Type *dest, Type value, int pe)                                       \
    {                                                                                               \
        (void) amo ("shmem_" #Name "_set", MI355_AMO_SET, (int) sizeof (Type), dest, TO_BITS (Type, value),  \
                    0, pe);                                                                         \
    }                                                                                               \
    ALIAS (Type, Name##_swap, (Type * target, Type value, int pe))                                  \
    ALIAS (Type, Name##_fetch, (const Type *dest, int pe))                                          \
    ALIAS (void, Name##_set, (Type * dest, Type value, int pe))

#define AMO_INTEGER(Name, Type)                                                                     \
    Type pshmem_##Name##_cswap (Type *target, Type cond, Type value, int pe)                        \
    {                                                                                               \
        return FROM_BITS (Type, amo ("shmem_" #Name "_cswap", MI355_AMO_CSWAP, (int) sizeof (Type), target,  \
                                     TO_BITS (Type, value), TO_BITS (Type, cond), pe));             \
    }                                                                                               \
    Type pshmem_##Name##_fadd (Type *target, Type value, int pe)                                    \
    {                                                                                               \
        return FROM_BITS (Type, amo ("shmem_" #Name "_fadd", MI355_AMO_FADD, (int) sizeof (Type), target,    \
                                     TO_BITS (Type, value), 0, pe));                                \
    }                                                                                               \
    Type pshmem_##Name##_finc (Type *target, int pe)                                                \
    {                                                                                               \
        return FROM_BITS (Type, amo ("shmem_" #Name "_finc", MI355_AMO_FADD, (int) sizeof (Type), target, 1, \
                                     0, pe));                                                       \
    }                                                                                               \
    void pshmem_##Name##_add (Type *target, Type value, int pe)                                     \
    {                                                                                               \
        (void) amo ("shmem_" #Name "_add", MI355_AMO_FADD, (int) sizeof (Type), target,             \
                    TO_BITS (Type, value), 0, pe);                                                  \
    }                                                                                               \
    void pshmem_##Name##_inc (Type *target, int pe)                                                 \
    {                                                                                               \
        (void) amo ("shmem_" #Name "_inc", MI355_AMO_FADD, (int) sizeof (Type), target, 1, 0, pe);  \
    }                                                                                               \
    ALIAS (Type, Name##_cswap, (Type * target, Type cond, Type value, int pe))                      \
    ALIAS (Type, Name##_fadd, (Type * target, Type value, int pe))                                  \
    ALIAS (Type, Name##_finc, (Type * target, int pe))                                              \
    ALIAS (void, Name##_add, (Type * target, Type value, int pe))                                   \
    ALIAS (void, Name##_inc, (Type * target, int pe))

AMO_SWAP_FETCH_SET (int, int)
AMO_SWAP_FETCH_SET (long, long)
AMO_SWAP_FETCH_SET (longlong, long long)
AMO_SWAP_FETCH_SET (float, float)
AMO_SWAP_FETCH_SET (double, double)
AMO_INTEGER (int, int)
AMO_INTEGER (long, long)
AMO_INTEGER (longlong, long long)

/* ---------------------------------------------------------------------- */
/* fence                                                                   */
/* ---------------------------------------------------------------------- */
/* Every put and atomic of this library is complete at its target when the
 * call returns or, for the copy kernel's local completion, when the library
 * stream has drained: ordering them is the quiet. */
void pshmem_fence (void) { pshmem_quiet (); }
void shmem_fence (void) __attribute__ ((weak, alias ("pshmem_fence")));

/* ---------------------------------------------------------------------- */
/* wait / wait_until                                                       */
/* ---------------------------------------------------------------------- */
static const char *const cmp_names[6] = {"==", "!=", ">", "<=", "<", ">="};

static int satisfied (int cmp, long long v, long long want)
{
    switch (cmp) {
    case SHMEM_CMP_EQ: return v == want;
    case SHMEM_CMP_NE: return v != want;
    case SHMEM_CMP_GT: return v > want;
    case SHMEM_CMP_LE: return v <= want;
    case SHMEM_CMP_LT: return v < want;
    default: return v >= want;
    }
}

/* the bounded back-off of every waiting loop here: spin, then yield, then
 * sleep up to 50 us between polls; the abort flag and the limit are looked
 * at as the loop slows down */
struct backoff {
    double t0;
    unsigned polls;
};

static int backoff_expired (struct backoff *b, int dev)
{
    ++b->polls;
    if (!dev && b->polls < 2000) {
        __builtin_ia32_pause ();
        return 0;
    }
    if (b->polls < (dev ? 64u : 20000u)) {
        sched_yield ();
    } else {
        const struct timespec ts = {0, dev ? 20000 : 50000};
        nanosleep (&ts, NULL);
    }
    if ((b->polls & 63u) != 0)
        return 0;
    shmemi_check_abort ();
    const double t = shmemi_now ();
    if (b->t0 == 0.0)
        b->t0 = t;
    return t - b->t0 > shmemi.wait_timeout;
}

/* the value of the 2-, 4- or 8-byte variable at ivar (this PE's copy), sign-extended */
static long long read_ivar (const char *fn, int where, const volatile void *ivar, int width)
{
    if (where == AT_HOST) {
        switch (width) {
        case 2: return (int16_t) __atomic_load_n ((const volatile uint16_t *) ivar, __ATOMIC_SEQ_CST);
        case 4: return (int32_t) __atomic_load_n ((const volatile uint32_t *) ivar, __ATOMIC_SEQ_CST);
        default: return (int64_t) __atomic_load_n ((const volatile uint64_t *) ivar, __ATOMIC_SEQ_CST);
        }
    }
    if (width == 2) {
        /* 16 bits are read as 16 bits: a 2-byte copy into the host-coherent slot */
        shmemi_server_stop ();
        shmemi_order_after_caller (0);
        SHMEMI_HIP (hipMemcpyAsync (shmemi.amo_slot, (const void *) ivar, 2, hipMemcpyDeviceToHost, shmemi.stream));
        SHMEMI_HIP (hipStreamSynchronize (shmemi.stream));
        return (int16_t) __atomic_load_n ((uint16_t *) shmemi.amo_slot, __ATOMIC_ACQUIRE);
    }
    const uint64_t v = dev_amo (fn, MI355_AMO_FETCH, width, (void *) ivar, 0, 0);
    return width == 4 ? (long long) (int32_t) v : (long long) (int64_t) v;
}

static void wait_until (const char *fn, const volatile void *ivar, int width, int cmp, long long want)
{
    void *addr = NULL;
    if (cmp < SHMEM_CMP_EQ || cmp > SHMEM_CMP_GE) {
        shmemi_init_check (fn);
        shmemi_fatal ("%s: unknown comparison %d (SHMEM_CMP_EQ .. SHMEM_CMP_GE)", fn, cmp);
    }
    const int where = locate (fn, (const void *) ivar, (size_t) width, (size_t) width, shmemi.mype, &addr);
    struct backoff b = {0.0, 0};
    long long v;
    while (!satisfied (cmp, v = read_ivar (fn, where, ivar, width), want))
        if (backoff_expired (&b, where == AT_DEV))
            shmemi_fatal ("%s: the variable at %p still holds %lld after %.0f s (SHMEM_WAIT_TIMEOUT), waiting for "
                          "a value %s %lld", fn, (const void *) ivar, v, shmemi.wait_timeout, cmp_names[cmp], want);
    SHMEMI_TRACE (SHMEMI_LOG_ATOMIC, "%s(%p): %lld %s %lld after %u polls of the %s heap", fn, (const void *) ivar, v,
                  cmp_names[cmp], want, b.polls + 1, where == AT_HOST ? "host" : "device");
}

#define WAITS(Name, Type)                                                                           \
    void pshmem_##Name##_wait_until (volatile Type *ivar, int cmp, Type cmp_value)                  \
    {                                                                                               \
        wait_until ("shmem_" #Name "_wait_until", ivar, (int) sizeof (Type), cmp, cmp_value);       \
    }                                                                                               \
    void pshmem_##Name##_wait (volatile Type *ivar, Type cmp_value)                                 \
    {                                                                                               \
        wait_until ("shmem_" #Name "_wait", ivar, (int) sizeof (Type), SHMEM_CMP_NE, cmp_value);    \
    }                                                                                               \
    ALIAS (void, Name##_wait_until, (volatile Type * ivar, int cmp, Type cmp_value))                \
    ALIAS (void, Name##_wait, (volatile Type * ivar, Type cmp_value))

WAITS (short, short)
WAITS (int, int)
WAITS (long, long)
WAITS (longlong, long long)

/* the untyped names wait on a long (reference waituntil.c) */
void pshmem_wait_until (volatile long *ivar, int cmp, long cmp_value)
{
    wait_until ("shmem_wait_until", ivar, (int) sizeof (long), cmp, cmp_value);
}
void pshmem_wait (volatile long *ivar, long cmp_value)
{
    wait_until ("shmem_wait", ivar, (int) sizeof (long), SHMEM_CMP_NE, cmp_value);
}
void (shmem_wait_until) (volatile long *ivar, int cmp, long cmp_value) __attribute__ ((weak, alias ("pshmem_wait_until")));
void (shmem_wait) (volatile long *ivar, long cmp_value) __attribute__ ((weak, alias ("pshmem_wait")));

/* ---------------------------------------------------------------------- */
/* locks                                                                   */
/* ---------------------------------------------------------------------- */
struct lock_at {
    uint32_t *next, *serving; /* this PE's addresses of the two halves */
    int home;
};

static struct lock_at lock_of (const char *fn, volatile long *lock)
{
    void *addr = NULL;
    const int where = locate (fn, (const void *) lock, sizeof (long), sizeof (long), shmemi.mype, &addr);
    const size_t off = where == AT_DEV ? shmemi_heap_offset ((const void *) lock)
                                       : (size_t) ((const char *) lock - shmemi.hheap);
    struct lock_at l = {(uint32_t *) lock, (uint32_t *) lock + 1, (int) ((off / sizeof (long)) % (size_t) shmemi.npes)};
    return l;
}

void pshmem_set_lock (volatile long *lock)
{
    static const char fn[] = "shmem_set_lock";
    const struct lock_at l = lock_of (fn, lock);
    const uint32_t ticket = (uint32_t) amo (fn, MI355_AMO_FADD, 4, l.next, 1, 0, l.home);
    struct backoff b = {0.0, 0};
    uint32_t s;
    while ((s = (uint32_t) amo (fn, MI355_AMO_FETCH, 4, l.serving, 0, 0, l.home)) != ticket)
        if (backoff_expired (&b, shmemi_in_device_heap ((const void *) lock, sizeof (long))))
            shmemi_fatal ("%s: the lock at %p (home PE %d) serves ticket %u after %.0f s (SHMEM_WAIT_TIMEOUT); this "
                          "PE holds ticket %u", fn, (const void *) lock, l.home, s, shmemi.wait_timeout, ticket);
    SHMEMI_TRACE (SHMEMI_LOG_LOCK, "%s(%p): ticket %u at home PE %d after %u polls", fn, (const void *) lock, ticket,
                  l.home, b.polls + 1);
}

void pshmem_clear_lock (volatile long *lock)
{
    static const char fn[] = "shmem_clear_lock";
    const struct lock_at l = lock_of (fn, lock);
    pshmem_quiet (); /* the holder's puts are visible before the next holder runs */
    const uint32_t s = (uint32_t) amo (fn, MI355_AMO_FADD, 4, l.serving, 1, 0, l.home);
    SHMEMI_TRACE (SHMEMI_LOG_LOCK, "%s(%p): ticket %u done at home PE %d", fn, (const void *) lock, s, l.home);
}

int pshmem_test_lock (volatile long *lock)
{
    static const char fn[] = "shmem_test_lock";
    const struct lock_at l = lock_of (fn, lock);
    const uint32_t s = (uint32_t) amo (fn, MI355_AMO_FETCH, 4, l.serving, 0, 0, l.home);
    const uint32_t seen = (uint32_t) amo (fn, MI355_AMO_CSWAP, 4, l.next, s + 1u, s, l.home);
    SHMEMI_TRACE (SHMEMI_LOG_LOCK, "%s(%p): serving %u, next %u at home PE %d: %s", fn, (const void *) lock, s, seen,
                  l.home, seen == s ? "taken" : "busy");
    return seen == s ? 0 : 1;
}

void shmem_set_lock (volatile long *lock) __attribute__ ((weak, alias ("pshmem_set_lock")));
void shmem_clear_lock (volatile long *lock) __attribute__ ((weak, alias ("pshmem_clear_lock")));
int shmem_test_lock (volatile long *lock) __attribute__ ((weak, alias ("pshmem_test_lock")));

/* ---------------------------------------------------------------------- */
/* shmemx_<T>_atomic_add_v                                                  */
/* ---------------------------------------------------------------------- */
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

static void host_add_v (int dtype, void *to, const void *from, size_t n)
{
    if (dtype == MI355_INT) {
        for (size_t i = 0; i < n; ++i)
            (void) __atomic_fetch_add ((uint32_t *) to + i, ((const uint32_t *) from)[i], __ATOMIC_SEQ_CST);
    } else if (dtype == MI355_LONG || dtype == MI355_LONGLONG) {
        for (size_t i = 0; i < n; ++i)
            (void) __atomic_fetch_add ((uint64_t *) to + i, ((const uint64_t *) from)[i], __ATOMIC_SEQ_CST);
    } else if (dtype == MI355_FLOAT) {
        /* a CAS loop on the bit pattern */
        for (size_t i = 0; i < n; ++i) {
            uint32_t *p = (uint32_t *) to + i, old = __atomic_load_n (p, __ATOMIC_RELAXED), new_;
            do {
                const float s = FROM_BITS (float, old) + ((const float *) from)[i];
                new_ = (uint32_t) TO_BITS (float, s);
            } while (!__atomic_compare_exchange_n (p, &old, new_, 1, __ATOMIC_SEQ_CST, __ATOMIC_RELAXED));
        }
    } else {
        for (size_t i = 0; i < n; ++i) {
            uint64_t *p = (uint64_t *) to + i, old = __atomic_load_n (p, __ATOMIC_RELAXED), new_;
            do {
                const double s = FROM_BITS (double, old) + ((const double *) from)[i];
                new_ = TO_BITS (double, s);
            } while (!__atomic_compare_exchange_n (p, &old, new_, 1, __ATOMIC_SEQ_CST, __ATOMIC_RELAXED));
        }
    }
}

static void dev_add_v (const char *fn, int dtype, void *to, const void *from, size_t n, int wait)
{
    if (wait)
        shmemi_arm_signal ();
    shmemi_timed_begin ();
    const int rc = mi355_atomic_add_v (dtype, to, from, n, shmemi.stream);
    shmemi_timed_end ();
    if (rc != 0)
        shmemi_fatal ("%s: accumulate kernel launch failed: %d", fn, rc);
    if (wait)
        shmemi_wait_signal ();
}

static void atomic_add_v (const char *fn, int dtype, size_t es, void *target, const void *source, size_t n, int pe)
{
    shmemi_init_check (fn);
    check_pe (fn, pe);
    if (n == 0)
        return;
    if (source == NULL)
        shmemi_fatal ("%s: NULL source (%zu elements, PE %d)", fn, n, pe);
    if (((uintptr_t) source & (es - 1)) != 0)
        shmemi_fatal ("%s: source %p is not aligned to its %zu-byte type", fn, source, es);
    if (n > (size_t) -1 / es)
        shmemi_fatal ("%s: %zu elements of %zu bytes overflow size_t", fn, n, es);
    void *to = NULL;
    const int where = locate (fn, target, n * es, es, pe, &to);
    SHMEMI_TRACE (SHMEMI_LOG_ATOMIC, "%s(%p, %p, %zu, PE %d): target in the %s heap", fn, target, source, n, pe,
                  where == AT_HOST ? "host" : "device");
    if (shmemi.heap != NULL)
        shmemi_server_stop ();
    const int src_dev = is_device_ptr (source);
    if (where == AT_HOST) {
        if (!src_dev) {
            host_add_v (dtype, to, source, n);
            return;
        }
        /* a device source into a host-heap target: bring it to the host first */
        void *tmp = malloc (n * es);
        if (tmp == NULL)
            shmemi_fatal ("out of host memory");
        shmemi_order_after_caller (0);
        SHMEMI_HIP (hipMemcpyAsync (tmp, source, n * es, hipMemcpyDeviceToHost, shmemi.stream));
        SHMEMI_HIP (hipStreamSynchronize (shmemi.stream));
        host_add_v (dtype, to, tmp, n);
        free (tmp);
        return;
    }
    shmemi_order_after_caller (0);
    if (src_dev) {
        dev_add_v (fn, dtype, to, source, n, 1);
        return;
    }
    /* a host source (the host heap or plain host memory): staged through
     * scratch C in pieces, as a2a_from_host stages its blocks (coll.c) */
    char *scratch = shmemi.heap + shmemi.scratch_off + 2 * shmemi.scratch_chunk;
    const size_t cap = shmemi.scratch_chunk / es;
    if (cap == 0)
        shmemi_fatal ("%s: no device scratch to stage a host source through", fn);
    for (size_t k0 = 0; k0 < n; k0 += cap) {
        const size_t cnt = n - k0 < cap ? n - k0 : cap;
        SHMEMI_HIP (hipMemcpyAsync (scratch, (const char *) source + k0 * es, cnt * es, hipMemcpyHostToDevice,
                                    shmemi.stream));
        dev_add_v (fn, dtype, (char *) to + k0 * es, scratch, cnt, 1); /* scratch is reused */
    }
}

#define ATOMIC_ADD_V(Name, Type, Dtype)                                                             \
    void shmemx_##Name##_atomic_add_v (Type *target, const Type *source, size_t nelems, int pe)     \
    {                                                                                               \
        atomic_add_v ("shmemx_" #Name "_atomic_add_v", Dtype, sizeof (Type), target, source, nelems, pe);   \
    }

ATOMIC_ADD_V (int, int, MI355_INT)
ATOMIC_ADD_V (long, long, MI355_LONG)
ATOMIC_ADD_V (longlong, long long, MI355_LONGLONG)
ATOMIC_ADD_V (float, float, MI355_FLOAT)
ATOMIC_ADD_V (double, double, MI355_DOUBLE)
