/*
 * shmemx.h -- MI355X extensions around the reduction path.
 *
 * Not part of the reference API (its experimental header src/shmemx.h holds
 * nb put/get and wtime, none of which this build provides except wtime).
 * These entry points let a caller keep reduction buffers device-resident in
 * the GPU symmetric heap and let the bench observe
 * kernel time on the library's own stream.
 */
#ifndef _SHMEMX_H
#define _SHMEMX_H 1

#include <stddef.h>
#include <shmem.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Device symmetric heap: memory in this PE's HBM, at the same offset from
 * the heap base on every PE, mapped into every peer GPU over xGMI.
 * Collective (all PEs call with the same size, like shmem_malloc). */
void *shmemx_malloc_device (size_t size);
void shmemx_free_device (void *ptr);
/* 1 if ptr lies in this PE's device symmetric heap. */
int shmemx_is_device_symmetric (const void *ptr);
/* PE pe's copy of the device-heap object at ptr as an address kernels on this
 * PE's GPU can load from and store to (an IPC mapping of pe's heap; xGMI
 * traffic when pe is on another GPU); NULL if ptr is not in the device heap or
 * pe's heap is not mapped. Not dereferenceable by the host. */
void *shmemx_peer_device_ptr (const void *ptr, int pe);

/* Device buffers outside the heap (hipMalloc, a framework's tensors) as
 * *_to_all target/source with PE_size > 1: the members export the
 * allocations holding them (IPC), map each other's for the call and reduce
 * in place of staging them through scratch -- one host barrier per call for
 * the exchange, no copies. Applies when every member passes device memory
 * of the same kinds (heap / not heap) for target and for source, 16-byte
 * aligned, target == source or disjoint, and every allocation can be
 * exported (hipMalloc yes, virtual-memory hipMemCreate no); otherwise every
 * member stages, as with SHMEM_EXTERNAL_MAP=0. Mapped allocations stay open
 * for later calls (at most SHMEM_EXTERNAL_MAP_CACHE, default 64; they keep
 * the peer's memory alive after it frees it): flush closes them all on this
 * PE; stats = allocations mapped now, opened and closed since init. */
void shmemx_external_map_flush (void);
void shmemx_external_map_stats (long *mapped, long *opened, long *closed);
/* Calls on mapped buffers that staged instead because a member could not open
 * a peer's buffer (its export is re-made for the next call). */
long shmemx_external_map_fallbacks (void);

/* Cross-PE schedule for *_to_all (env SHMEM_REDUCE_ALGORITHM sets the
 * default at init):
 *   SHMEMX_REDUCE_AUTO  = P2P shard schedule (below)
 *   SHMEMX_REDUCE_P2P   = each PE reduces 1/N of the elements from every
 *                         PE's source over xGMI, then gathers the other
 *                         shards; every PE receives the reference's result
 *                         for itself (or PE_start's, see the result order)
 *   SHMEMX_REDUCE_EXACT = each PE folds all N sources in the reference order
 *                         (own first, then ascending); bit-identical to the
 *                         reference on every PE
 *   SHMEMX_REDUCE_RCCL  = ncclAllReduce where RCCL has the op/type, P2P
 *                         otherwise (FP results within the stated tolerance)
 */
enum shmemx_reduce_algorithm {
    SHMEMX_REDUCE_AUTO = 0,
    SHMEMX_REDUCE_P2P = 1,
    SHMEMX_REDUCE_EXACT = 2,
    SHMEMX_REDUCE_RCCL = 3
};
int shmemx_set_reduce_algorithm (int algorithm); /* returns the previous one */
int shmemx_get_reduce_algorithm (void);
/* The schedule thresholds at run time (defaults: SHMEM_FUSED_MAX_BYTES = 2 MiB,
 * SHMEM_ONESHOT_MAX_BYTES = 64 KiB): messages up to fused_max bytes per PE
 * take the one-launch fused kernel (capped at 1 GiB; 0 = never), those up to
 * oneshot_max of them its one-shot fold. Collective settings like the
 * algorithm: every PE sets the same value between calls (SHMEM_DEBUG=1
 * checks both per call). Return the previous value. A fused path that the
 * init self-test turned off stays off. */
size_t shmemx_set_fused_max_bytes (size_t bytes);
size_t shmemx_set_oneshot_max_bytes (size_t bytes);
size_t shmemx_get_fused_max_bytes (void);
size_t shmemx_get_oneshot_max_bytes (void);
/* Whether init set the two thresholds above from measurement (PE_size > 1,
 * SHMEM_FUSED_MAX_BYTES / SHMEM_ONESHOT_MAX_BYTES not given,
 * SHMEM_THRESHOLD_CALIBRATE not 0): 1 if it did. us[0..21] (n entries
 * filled): the job-wide median call times in microseconds of the measured
 * double sums -- fused then multi-launch at 64K, 256K, 512K, 1M, 2M, 4M
 * bytes, one-shot then two-shot at 16K, 32K, 64K, 128K, 256K (0: size not
 * measured, larger than the scratch buffers). Each threshold is the largest
 * size of the prefix of sizes where the fused (one-shot) call was no slower. */
int shmemx_threshold_calibration (double *us, int n);

/* Whose result the P2P schedules (and the stream-ordered calls) deliver
 * (env SHMEM_REDUCE_ORDER=reference|pe_start sets the default at init):
 *   SHMEMX_ORDER_REFERENCE (default) = every PE receives the result the
 *       reference computes on THAT PE: its own source first, then the others
 *       in ascending active-set order (reduce-op.c:226-264). Where the order
 *       matters (floating-point sum/prod from 3 PEs, floating-point min/max
 *       from 2: rounding, NaN and +-0 selects) the owner of each shard folds it
 *       in every member's order in one pass over the sources and each PE
 *       gathers its own version: the same xGMI traffic as the shard schedule,
 *       plus (N-1)/N of the message written to local HBM.
 *   SHMEMX_ORDER_PE_START = every PE receives PE_start's result (identical bits
 *       on all PEs, the plain shard schedule).
 * Integer and bitwise reductions are order-independent: both give the same. */
enum shmemx_reduce_order {
    SHMEMX_ORDER_REFERENCE = 0,
    SHMEMX_ORDER_PE_START = 1
};
int shmemx_set_reduce_order (int order); /* returns the previous one */
int shmemx_get_reduce_order (void);
/* The schedule and the result order are per-PE settings, but they decide
 * what the members do together: every member of an active set must use the
 * same algorithm, order and SHMEM_DEVICE_ORDER_SIZE when it calls, or one PE
 * may take the fused path while another takes the multi-launch one (a hang),
 * or gather version areas its peers never wrote. Init aborts when the PEs'
 * environment settings differ; SHMEM_DEBUG=1 also checks every call (below).
 * With 2 PEs, floating-point sum and product are computed once (a + b is
 * b + a) and both PEs get the same bits; for float and double (and their
 * complex types), where both operands are NaNs with different payloads, the
 * reference's PE 1 would keep its own operand's payload (x86 SSE returns the
 * first operand's), so the payload -- not the NaN-ness -- may differ from the
 * reference's there (tests/_compare.py compares those NaNs whatever the
 * payload). Long double is exact, payloads included: the x87 picks between
 * two NaNs by their kind and significand, not by operand position.
 *
 * SHMEM_DEBUG=1: every *_to_all call (host API and stream-ordered) first
 * exchanges its arguments with the other members of its active set -- op,
 * type, nreduce, PE_start, logPE_stride, PE_size, the target/source memory
 * kinds and their symmetric-heap offsets, the algorithm and order settings --
 * and aborts every PE with a message naming the first field that differs
 * (the reference's debug build checks init and symmetry,
 * src/reduce/reduce-op.c:395-398, src/utils/utils.h:74-129). Costs two host
 * barriers per call. The exchange runs on the host when the call is issued,
 * so a stream-ordered call captured into a HIP graph is checked once, at
 * capture time: its replays repeat the captured arguments and are not
 * checked again. */

/* Persistent fused server (opt-in; env SHMEM_PERSISTENT=1 sets it at init,
 * SHMEM_PERSISTENT_IDLE_US = how long it stays without a call, default 1000):
 * back-to-back blocking reductions of one (type, op, active set) that take
 * the one-launch fused schedule (up to SHMEM_FUSED_MAX_BYTES, device-resident
 * symmetric buffers) are served by a fused kernel left resident between
 * calls, fed through a host-coherent mailbox: no launch per call. Results are
 * those of the launched kernel. Caveats, hence opt-in: a served call is not
 * ordered after GPU work the caller queued -- complete it first (the caller's
 * writes to the source must be done); and while the server is resident, HIP
 * calls that wait on the null stream or the whole device (hipDeviceSynchronize,
 * hipStreamSynchronize(0), hipMemcpy) return only once it idles out -- on this
 * HIP the null stream waits for the server's non-blocking stream too.
 * shmemx_device_synchronize and every other GPU operation of this library
 * stop it first. */
int shmemx_set_persistent (int enable); /* returns the previous setting */
/* since init: calls served by a resident server, servers launched */
void shmemx_persistent_stats (long *served, long *launched);

/* Device and timing helpers (used by bench.py and the tests). */
int shmemx_device_id (void);                 /* HIP ordinal of this PE's GPU */
/* Link from this PE's GPU to PE pe's: type (hsa_amd_link_info_type_t: 4 =
 * xGMI, 2 = PCIe) and hop count; -1 if pe shares this GPU or is not visible. */
int shmemx_peer_link (int pe, int *link_type, int *hops);
/* 1 if PE pe's GPU is this PE's GPU (same PCI bus id), else 0. */
int shmemx_pe_same_device (int pe);
void shmemx_device_synchronize (void);        /* hipDeviceSynchronize, checked */
/* hipMemcpy (kind inferred from the pointers), checked; blocking. */
void shmemx_memcpy (void *dst, const void *src, size_t nbytes);
double shmemx_wtime (void);                   /* seconds, monotonic */

/* Kernel timing: while enabled, every dominant kernel the reduction path
 * launches is bracketed by HIP events on the library's stream. */
void shmemx_kernel_timing (int enable);        /* enable resets the counters */
/* Number of timed launches, total and per-launch average duration (ms) of the
 * launches timed since the last enable. Synchronizes the stream. */
void shmemx_kernel_timing_stats (long *launches, double *total_ms, double *avg_ms);
/* the same for one phase: 0 = each call's dominant kernel (the fold, or a 1-PE call's copy; what
 * shmemx_kernel_timing_stats reports), 1 = the all-gather copy of the P2P schedule */
void shmemx_kernel_timing_phase_stats (int phase, long *launches, double *total_ms, double *avg_ms);

/* What this PE's last *_to_all call ran (host API and stream-ordered calls):
 * the schedule, the dominant kernel -- the reduce-scatter fold of the P2P
 * schedules, the copy of a 1-PE call, the fused kernel -- and the bytes that
 * kernel streams, computed from the schedule the library chose, not assumed
 * by the caller. Returns 0, or -1 before the first call. */
typedef struct shmemx_call_info {
    char schedule[64];      /* "p2p", "p2p-rounds", "fused-oneshot", "fused-twoshot", "persistent",
                             * "identity", "exact", "rccl", "staged", "barrier-only"; the scan
                             * collectives' "scan-*" names are listed with them below */
    char kernel[256];       /* demangled dominant kernel, as rocprofv3 names it ("" for rccl) */
    int ordered;            /* 1: every member's reference order (version areas written) */
    int sources, outputs;   /* buffers the dominant kernel reads / writes */
    int peer_sources;       /* of its sources, how many lie in other PEs' heaps */
    int launches;           /* dominant-kernel launches in the call (rounds) */
    unsigned long long bytes_per_buffer;  /* bytes of each source and output, per launch */
    unsigned long long alg_bytes;         /* (sources + outputs) x bytes_per_buffer, + the fused
                                           * two-shot's gather (2 (N-1) shards) */
    unsigned long long peer_bytes;        /* of alg_bytes, read from other PEs' heaps */
} shmemx_call_info;
int shmemx_last_call_info (shmemx_call_info *info);

/* The init-time coherence self-test of peer-heap reads (PE_size > 1 jobs):
 * every PE reads every peer's marker through its L2 (a cached load), each
 * peer rewrites its marker with a write-through store, and after a barrier
 * the reader re-reads it once without and once after mi355_acquire_system.
 * ran: the test ran (peer heaps mapped); passed: the re-read after the
 * acquire saw every new value on every PE (else the job runs the RCCL
 * schedule, like a failed mapping); stale_without_acquire: some PE's re-read
 * WITHOUT the acquire returned an old value (evidence that the acquire the
 * P2P schedules queue before reading peers' buffers is needed). All three
 * are the job's (OR / AND over the PEs). */
void shmemx_coherence_selftest (int *ran, int *passed, int *stale_without_acquire);
/* The same test's check of system-coherent loads (sc0 sc1, the fused kernel's
 * reads of the members' buffers), made before any acquire: sysload_fresh =
 * every block of every PE saw every peer's new value; acquires_skipped = the
 * fused kernel therefore runs without its per-block system-scope acquires
 * (SHMEM_FUSED_ACQUIRE=1 keeps them). */
void shmemx_coherence_sysload (int *sysload_fresh, int *acquires_skipped);
/* The init test of the CALLER's producer path (round 4): every PE wrote 32
 * words with plain stores from a kernel on the null stream, as a caller
 * writes its source, and every peer re-read them (after caching the old
 * values) in the fused kernel's ordering (same-stream flag, device wait) and
 * in the multi-launch schedules' (signal kernel, host wait, host barrier).
 * fresh[6] (1 = every block of every PE saw every new word), in order:
 * fused ordering plain loads / 16-byte system-coherent loads / plain loads
 * after a system-scope acquire, then the same three after the host-wait
 * ordering. The fused kernel skips its acquires only when fresh[1] (and
 * sysload_fresh) hold; it is not used when neither fresh[1] nor fresh[2];
 * the job runs RCCL when fresh[5] fails. ran = 0 above 64 PEs. */
void shmemx_coherence_producer (int *ran, int *fresh);
/* The init timing of device-side waits (PE_size > 1 jobs with signal regions):
 * us = the job's slowest PE's time per device barrier over all PEs; slow = 1
 * when that passed 1 ms (the hardware time-slices the PEs' queues: more PEs
 * on one GPU than it schedules together), and then the job runs host barriers
 * and no fused kernel. */
void shmemx_device_wait_report (int *slow, double *us);

/* Bring up the RCCL communicator of the whole job (what SHMEM_REDUCE_ALGORITHM=rccl uses) without
 * aborting when RCCL cannot come up within timeout_s seconds: 0 = ready on this PE, -1 = not. Every PE
 * must call it; agree on the outcome (e.g. a min reduction) before selecting the RCCL schedule. */
int shmemx_rccl_init (double timeout_s);

/* Stream-ordered collectives. Enqueued on `stream` (a hipStream_t; NULL =
 * the null stream) and return at once: the reduction runs after the work
 * queued on that stream before it, and the work queued after it sees the
 * result. Cross-PE ordering is device-side (a one-launch fused kernel for
 * messages up to SHMEM_FUSED_MAX_BYTES, else fold and gather kernels between
 * one-block device barriers), so a call can be captured into a HIP graph and
 * replayed; every replay is one more collective for all members.
 *   - target and source lie in the device symmetric heap, equal or disjoint
 *   - PE_size <= 32; P2P schedule whatever the reduce algorithm setting,
 *     delivering the result order set by shmemx_set_reduce_order
 *   - every member issues the same sequence of collectives, host-side and
 *     stream-ordered interleaved in the same order; one PE's stream-ordered
 *     calls run one at a time: one stream, or streams the caller orders
 *     (host-side calls use separate device flags and may overlap them)
 *   - a device-side wait that times out (SHMEM_BARRIER_TIMEOUT) is reported
 *     by the next shmem_barrier_all / shmem_quiet / stream-ordered call
 * pWrk and pSync are accepted for symmetry with shmem_*_to_all and unused. */
void shmemx_barrier_on_stream (int PE_start, int logPE_stride, int PE_size, void *stream);
void shmemx_short_sum_to_all_on_stream (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync, void *stream);
void shmemx_int_sum_to_all_on_stream (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync, void *stream);
void shmemx_long_sum_to_all_on_stream (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync, void *stream);
void shmemx_longlong_sum_to_all_on_stream (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync, void *stream);
void shmemx_float_sum_to_all_on_stream (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync, void *stream);
void shmemx_double_sum_to_all_on_stream (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync, void *stream);
void shmemx_longdouble_sum_to_all_on_stream (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync, void *stream);
void shmemx_complexf_sum_to_all_on_stream (COMPLEXIFY (float) *target, COMPLEXIFY (float) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (float) *pWrk, long *pSync, void *stream);
void shmemx_complexd_sum_to_all_on_stream (COMPLEXIFY (double) *target, COMPLEXIFY (double) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (double) *pWrk, long *pSync, void *stream);
void shmemx_short_prod_to_all_on_stream (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync, void *stream);
void shmemx_int_prod_to_all_on_stream (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync, void *stream);
void shmemx_long_prod_to_all_on_stream (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync, void *stream);
void shmemx_longlong_prod_to_all_on_stream (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync, void *stream);
void shmemx_float_prod_to_all_on_stream (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync, void *stream);
void shmemx_double_prod_to_all_on_stream (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync, void *stream);
void shmemx_longdouble_prod_to_all_on_stream (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync, void *stream);
void shmemx_complexf_prod_to_all_on_stream (COMPLEXIFY (float) *target, COMPLEXIFY (float) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (float) *pWrk, long *pSync, void *stream);
void shmemx_complexd_prod_to_all_on_stream (COMPLEXIFY (double) *target, COMPLEXIFY (double) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (double) *pWrk, long *pSync, void *stream);
void shmemx_short_and_to_all_on_stream (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync, void *stream);
void shmemx_int_and_to_all_on_stream (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync, void *stream);
void shmemx_long_and_to_all_on_stream (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync, void *stream);
void shmemx_longlong_and_to_all_on_stream (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync, void *stream);
void shmemx_short_or_to_all_on_stream (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync, void *stream);
void shmemx_int_or_to_all_on_stream (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync, void *stream);
void shmemx_long_or_to_all_on_stream (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync, void *stream);
void shmemx_longlong_or_to_all_on_stream (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync, void *stream);
void shmemx_short_xor_to_all_on_stream (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync, void *stream);
void shmemx_int_xor_to_all_on_stream (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync, void *stream);
void shmemx_long_xor_to_all_on_stream (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync, void *stream);
void shmemx_longlong_xor_to_all_on_stream (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync, void *stream);
void shmemx_short_max_to_all_on_stream (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync, void *stream);
void shmemx_int_max_to_all_on_stream (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync, void *stream);
void shmemx_long_max_to_all_on_stream (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync, void *stream);
void shmemx_longlong_max_to_all_on_stream (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync, void *stream);
void shmemx_float_max_to_all_on_stream (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync, void *stream);
void shmemx_double_max_to_all_on_stream (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync, void *stream);
void shmemx_longdouble_max_to_all_on_stream (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync, void *stream);
void shmemx_short_min_to_all_on_stream (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync, void *stream);
void shmemx_int_min_to_all_on_stream (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync, void *stream);
void shmemx_long_min_to_all_on_stream (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync, void *stream);
void shmemx_longlong_min_to_all_on_stream (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync, void *stream);
void shmemx_float_min_to_all_on_stream (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync, void *stream);
void shmemx_double_min_to_all_on_stream (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync, void *stream);
void shmemx_longdouble_min_to_all_on_stream (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync, void *stream);

/* ---- 16-bit floating-point reductions (not in the reference) ----
 * Elements are passed as their 16 bits: half is IEEE binary16, bfloat16 the
 * upper 16 bits of binary32. sum, prod, min and max; no bitwise operators.
 * The fold order is float's: in SHMEMX_ORDER_REFERENCE PE q receives
 * (((src_q op src_m0) op src_m1) ...) over the other members m0 < m1 < ... of
 * the active set, in SHMEMX_ORDER_PE_START every PE receives PE_start's
 * result. EVERY step is rounded to the type: for sum and prod
 * r = round (float (a) op float (b)), to nearest, ties to even, subnormals
 * kept, overflow to +-inf -- the correctly rounded 16-bit operation -- and a
 * NaN result is the canonical quiet NaN (0x7E00 half, 0x7FC0 bfloat16)
 * whatever the operands' payloads. min and max are `a < b ? a : b` and
 * `a > b ? a : b` on the values and return the chosen operand's bits
 * unchanged (a NaN or a +-0 pair selects by position, as for float). The
 * result does not depend on the schedule. There is no pshmem_ twin.
 * These types take the multi-launch schedules (no one-launch fused kernel or
 * persistent server yet), and SHMEM_REDUCE_ALGORITHM=rccl falls back to P2P. */
typedef unsigned short shmemx_half_t, shmemx_bfloat16_t;
void shmemx_half_sum_to_all (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_half_prod_to_all (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_half_max_to_all (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_half_min_to_all (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_bfloat16_sum_to_all (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_bfloat16_prod_to_all (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_bfloat16_max_to_all (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_bfloat16_min_to_all (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_half_sum_to_all_on_stream (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync, void *stream);
void shmemx_half_prod_to_all_on_stream (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync, void *stream);
void shmemx_half_max_to_all_on_stream (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync, void *stream);
void shmemx_half_min_to_all_on_stream (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync, void *stream);
void shmemx_bfloat16_sum_to_all_on_stream (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync, void *stream);
void shmemx_bfloat16_prod_to_all_on_stream (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync, void *stream);
void shmemx_bfloat16_max_to_all_on_stream (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync, void *stream);
void shmemx_bfloat16_min_to_all_on_stream (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync, void *stream);

/* ---- scan collectives: inclusive and exclusive prefix reductions ----
 * shmemx_<T>_<op>_inscan / _exscan for exactly the (type, op) pairs that have
 * a *_to_all (the reference's 44 and half/bfloat16 sum, prod, max, min), with
 * the arguments of that *_to_all. Member j of the active set (its index in
 * it) receives
 *   inscan:  src_0 op src_1 op ... op src_j      (member 0: a copy of its source)
 *   exscan:  src_0 op src_1 op ... op src_(j-1)  (member 0: its target is left
 *            UNTOUCHED, as MPI_Exscan leaves rank 0's)
 * as a left fold in ascending member order with the accumulator on the left,
 * every step the operator *_to_all uses (SSE's NaN rule, libgcc's complex
 * product, x87 long double; half and bfloat16 rounded to the type at every
 * step, a NaN out of their sum or prod canonical): member j's inscan is bit
 * for bit the reference's result on the FIRST member of the set reduced over
 * members 0 .. j. A scan has one order: shmemx_set_reduce_order does not
 * apply, and shmemx_set_reduce_algorithm does not change the bits (EXACT and
 * RCCL requests run the scan schedule; a trace line says so).
 * As *_to_all: collective and blocking; nreduce == 0 still synchronizes; pWrk
 * and pSync are never written; target == source is allowed, and partially
 * overlapping target and source give the result of a call with a copied
 * source; a one-member set gives inscan = copy, exscan = nothing;
 * SHMEM_DEBUG=1 exchanges the arguments first. Buffers: the device symmetric
 * heap, and host objects (staged through the scratch buffers); a device
 * buffer outside the heap aborts with a message naming the function and the
 * buffer. shmemx_last_call_info reports "scan-p2p", "scan-p2p-host",
 * "scan-p2p-rounds", "scan-p2p-host-rounds", "scan-direct", "scan-staged" or
 * "scan-local". SHMEM_SCAN_DIRECT=1 (a testing aid; set on every PE) forces
 * the direct schedule of the sets larger than 32 members. There is no
 * pshmem_ twin, no Fortran wrapper and no stream-ordered form. */
void shmemx_short_sum_inscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_prod_inscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_and_inscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_or_inscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_xor_inscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_max_inscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_min_inscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_int_sum_inscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_prod_inscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_and_inscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_or_inscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_xor_inscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_max_inscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_min_inscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_long_sum_inscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_prod_inscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_and_inscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_or_inscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_xor_inscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_max_inscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_min_inscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_longlong_sum_inscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_prod_inscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_and_inscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_or_inscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_xor_inscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_max_inscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_min_inscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_float_sum_inscan (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync);
void shmemx_float_prod_inscan (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync);
void shmemx_float_max_inscan (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync);
void shmemx_float_min_inscan (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync);
void shmemx_double_sum_inscan (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync);
void shmemx_double_prod_inscan (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync);
void shmemx_double_max_inscan (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync);
void shmemx_double_min_inscan (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync);
void shmemx_longdouble_sum_inscan (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync);
void shmemx_longdouble_prod_inscan (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync);
void shmemx_longdouble_max_inscan (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync);
void shmemx_longdouble_min_inscan (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync);
void shmemx_complexf_sum_inscan (COMPLEXIFY (float) *target, COMPLEXIFY (float) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (float) *pWrk, long *pSync);
void shmemx_complexf_prod_inscan (COMPLEXIFY (float) *target, COMPLEXIFY (float) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (float) *pWrk, long *pSync);
void shmemx_complexd_sum_inscan (COMPLEXIFY (double) *target, COMPLEXIFY (double) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (double) *pWrk, long *pSync);
void shmemx_complexd_prod_inscan (COMPLEXIFY (double) *target, COMPLEXIFY (double) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (double) *pWrk, long *pSync);
void shmemx_half_sum_inscan (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_half_prod_inscan (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_half_max_inscan (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_half_min_inscan (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_bfloat16_sum_inscan (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_bfloat16_prod_inscan (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_bfloat16_max_inscan (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_bfloat16_min_inscan (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_short_sum_exscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_prod_exscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_and_exscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_or_exscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_xor_exscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_max_exscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_short_min_exscan (short *target, short *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        short *pWrk, long *pSync);
void shmemx_int_sum_exscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_prod_exscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_and_exscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_or_exscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_xor_exscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_max_exscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_int_min_exscan (int *target, int *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        int *pWrk, long *pSync);
void shmemx_long_sum_exscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_prod_exscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_and_exscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_or_exscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_xor_exscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_max_exscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_long_min_exscan (long *target, long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long *pWrk, long *pSync);
void shmemx_longlong_sum_exscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_prod_exscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_and_exscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_or_exscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_xor_exscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_max_exscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_longlong_min_exscan (long long *target, long long *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long long *pWrk, long *pSync);
void shmemx_float_sum_exscan (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync);
void shmemx_float_prod_exscan (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync);
void shmemx_float_max_exscan (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync);
void shmemx_float_min_exscan (float *target, float *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        float *pWrk, long *pSync);
void shmemx_double_sum_exscan (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync);
void shmemx_double_prod_exscan (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync);
void shmemx_double_max_exscan (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync);
void shmemx_double_min_exscan (double *target, double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        double *pWrk, long *pSync);
void shmemx_longdouble_sum_exscan (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync);
void shmemx_longdouble_prod_exscan (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync);
void shmemx_longdouble_max_exscan (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync);
void shmemx_longdouble_min_exscan (long double *target, long double *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        long double *pWrk, long *pSync);
void shmemx_complexf_sum_exscan (COMPLEXIFY (float) *target, COMPLEXIFY (float) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (float) *pWrk, long *pSync);
void shmemx_complexf_prod_exscan (COMPLEXIFY (float) *target, COMPLEXIFY (float) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (float) *pWrk, long *pSync);
void shmemx_complexd_sum_exscan (COMPLEXIFY (double) *target, COMPLEXIFY (double) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (double) *pWrk, long *pSync);
void shmemx_complexd_prod_exscan (COMPLEXIFY (double) *target, COMPLEXIFY (double) *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        COMPLEXIFY (double) *pWrk, long *pSync);
void shmemx_half_sum_exscan (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_half_prod_exscan (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_half_max_exscan (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_half_min_exscan (shmemx_half_t *target, shmemx_half_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_half_t *pWrk, long *pSync);
void shmemx_bfloat16_sum_exscan (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_bfloat16_prod_exscan (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_bfloat16_max_exscan (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);
void shmemx_bfloat16_min_exscan (shmemx_bfloat16_t *target, shmemx_bfloat16_t *source,
        int nreduce, int PE_start, int logPE_stride, int PE_size,
        shmemx_bfloat16_t *pWrk, long *pSync);

/* ---- atomic accumulate: target_on_pe[i] += source[i] atomically, i < nelems.
 *      The one-sided sibling of a sum reduction (MPI_Accumulate, a scatter-add
 *      into a peer's buffer): several PEs may add into one target at once, and
 *      the same target may take shmem_<T>_add / fadd meanwhile. The target is
 *      symmetric, in the device heap (one launch of the accumulate kernel,
 *      mi355_atomic_add_v, on the peer's mapped heap; the source may be device
 *      memory or any host memory, which is staged through device scratch) or
 *      in the host heap (a host loop of atomic adds; for float and double a
 *      compare-and-swap on the bit pattern). Integers wrap. A float or double
 *      sum depends on the arrival order in its last bits when several PEs add
 *      at once. Each float or double add is one correctly rounded IEEE add
 *      (nearest-even, gradual underflow, overflow to Inf, IEEE zero signs),
 *      the same bits in either heap. Where an add's result is a NaN (a NaN
 *      operand, Inf + -Inf) the element holds a NaN and nothing more is
 *      specified: its sign, payload and quiet bit may differ between the
 *      heaps and between builds (the host compiler may commute the operands).
 *      Blocking: complete at the target on return. Not collective. ---- */
void shmemx_int_atomic_add_v (int *target, const int *source, size_t nelems, int pe);
void shmemx_long_atomic_add_v (long *target, const long *source, size_t nelems, int pe);
void shmemx_longlong_atomic_add_v (long long *target, const long long *source, size_t nelems, int pe);
void shmemx_float_atomic_add_v (float *target, const float *source, size_t nelems, int pe);
void shmemx_double_atomic_add_v (double *target, const double *source, size_t nelems, int pe);

/* ---- value and location: maxloc / minloc reductions (MPI_MAXLOC / MPI_MINLOC) ----
 * shmemx_<T>_maxloc_to_all / _minloc_to_all for T = short, int, long, longlong,
 * float, double, half, bfloat16. Member j of the active set (its index in the
 * set, 0 .. PE_size - 1) contributes, for each i < nreduce, the candidate pair
 * (source[i], source_loc[i]); with source_loc == NULL the location is the
 * member index j (not the PE number). b beats a for maxloc when
 *   b.v is a NaN and (a.v is not a NaN, or b.l < a.l), or
 *   neither is a NaN and (b.v > a.v, or (b.v == a.v and b.l < a.l));
 * minloc has < for > on the values. A NaN beats every number in BOTH operators:
 * it propagates and reports where it is, as torch.max / torch.min do. -0 and +0
 * are equal (the smaller location decides); half and bfloat16 compare by their
 * exact float values; integers have no NaN branch. The result is the left fold
 * over members 0, 1, ... in ascending order from member 0's pair,
 *   acc = beats (cand_j, acc) ? cand_j : acc,
 * so two candidates that tie in class and in location keep the lower member.
 * The winner's value bits arrive in target[i] unchanged (NaN payload, zero
 * sign, 16-bit pattern), its location in target_loc[i]; every member receives
 * the same pair, and nothing is rounded, so the bits do not depend on the
 * schedule.
 * Collective and blocking; nreduce == 0 still synchronizes ("barrier-only").
 * All four arrays lie in the device symmetric heap (shmemx_malloc_device); any
 * other memory aborts with a message naming the function and the argument --
 * host arrays are not staged. target == source together with target_loc ==
 * source_loc is allowed (in place); any other overlap between the arrays is
 * undefined. There is no pWrk or pSync: nothing would use them.
 * Schedule (shmemx_last_call_info: "loc-p2p"; "loc-local" for a one-member set,
 * which is one local fold with no barrier): barrier, every member folds its
 * shard (mi355_shard_bounds; the same element range of the 8-byte locations)
 * of every member's arrays into its own target / target_loc, barrier, one copy
 * launch pulls the other owners' value and location shards from their targets,
 * barrier. Host barriers only. Sets above 32 members chain fold launches.
 * Not built: long double and complex; a stream-ordered or graph-captured form;
 * the fused one-launch kernel and the persistent server; RCCL; Fortran
 * wrappers; a pshmem_ twin; the SHMEM_DEBUG argument exchange. */
void shmemx_short_maxloc_to_all (short *target, long *target_loc, const short *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_short_minloc_to_all (short *target, long *target_loc, const short *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_int_maxloc_to_all (int *target, long *target_loc, const int *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_int_minloc_to_all (int *target, long *target_loc, const int *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_long_maxloc_to_all (long *target, long *target_loc, const long *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_long_minloc_to_all (long *target, long *target_loc, const long *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_longlong_maxloc_to_all (long long *target, long *target_loc, const long long *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_longlong_minloc_to_all (long long *target, long *target_loc, const long long *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_float_maxloc_to_all (float *target, long *target_loc, const float *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_float_minloc_to_all (float *target, long *target_loc, const float *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_double_maxloc_to_all (double *target, long *target_loc, const double *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_double_minloc_to_all (double *target, long *target_loc, const double *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_half_maxloc_to_all (shmemx_half_t *target, long *target_loc, const shmemx_half_t *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_half_minloc_to_all (shmemx_half_t *target, long *target_loc, const shmemx_half_t *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_bfloat16_maxloc_to_all (shmemx_bfloat16_t *target, long *target_loc, const shmemx_bfloat16_t *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_bfloat16_minloc_to_all (shmemx_bfloat16_t *target, long *target_loc, const shmemx_bfloat16_t *source, const long *source_loc,
        int nreduce, int PE_start, int logPE_stride, int PE_size);

/* ---- wide sum: half / bfloat16 sums accumulated in binary32 ----
 * shmemx_<T>_wsum_to_all (a result of the type) and shmemx_<T>_wsum_to_all_float
 * (a float result) for T = half, bfloat16. With the members j = 0 .. PE_size - 1
 * of the active set in ascending order, for each i < nreduce
 *   acc = (float) source_0[i]                      exact
 *   acc = acc + (float) source_j[i]                IEEE binary32 add: to nearest
 *                                                  even, subnormals kept
 *   target[i] = acc rounded once to T (to nearest even, subnormals kept, overflow
 *               to +-inf), or acc itself (_float)
 * on EVERY member, whatever SHMEM_REDUCE_ORDER / shmemx_set_reduce_order says:
 * all members receive the same bits, independent of shard bounds and schedule.
 * Unlike shmemx_<T>_sum_to_all, whose every step is rounded to the 16-bit type
 * and whose members fold in their own orders from three members on, an
 * intermediate beyond the type's range does not become an infinity (half:
 * 60000 + 60000 - 60000 is 60000) and the low bits survive to the one rounding.
 * A NaN result is the canonical quiet NaN (0x7E00, 0x7FC0, float: 0x7FC00000),
 * in a one-member set too: that call converts, it does not copy bytes.
 * Collective and blocking; nreduce == 0 still synchronizes ("barrier-only").
 * Both arrays lie in the device symmetric heap (shmemx_malloc_device). There
 * is no pWrk or pSync: nothing would use them. target == source is allowed for
 * the 16-bit result (in place). The library aborts with a message naming the
 * function and the argument for: any other overlap; a float target that
 * overlaps the source at all; an array outside the device symmetric heap (host
 * arrays are not staged, other device memory is not mapped); a NULL pointer;
 * nreduce < 0; an active set above 32 members; peer reads that failed the init
 * self-test.
 * Schedule (shmemx_last_call_info: "wide-p2p"; "wide-local" for a one-member
 * set, which is one local fold with no barrier): barrier, every member folds
 * its shard (mi355_shard_bounds of the 2-byte source elements, so a float
 * shard starts on a 512-byte boundary) of every member's source into its own
 * target with one mi355_combine_wide launch (kernel mi355k::wide_fold_*),
 * barrier, one copy launch pulls the other owners' shards from their targets,
 * barrier. Host barriers only.
 * Deliberately not built: a stream-ordered or graph-captured form; the fused
 * one-launch kernel, the persistent server and RCCL; Fortran wrappers; host-heap
 * or external (non-heap) buffers; prod, min and max (min and max round nothing,
 * a wide product is a different contract); sets above 32 members. */
void shmemx_half_wsum_to_all (shmemx_half_t *target, const shmemx_half_t *source, int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_half_wsum_to_all_float (float *target, const shmemx_half_t *source, int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_bfloat16_wsum_to_all (shmemx_bfloat16_t *target, const shmemx_bfloat16_t *source, int nreduce, int PE_start, int logPE_stride, int PE_size);
void shmemx_bfloat16_wsum_to_all_float (float *target, const shmemx_bfloat16_t *source, int nreduce, int PE_start, int logPE_stride, int PE_size);

#ifdef __cplusplus
}
#endif

#endif /* _SHMEMX_H */
