/*
 * shmem.h -- OpenSHMEM 1.3 reduction surface of the MI355X reduction path.
 *
 * Drop-in for the reduction subset of the reference header
 * (openshmem-org/osss-gasnet src/shmem.h):
 *   - constants           src/shmem.h:1495-1505 (values identical, LP64)
 *   - 44 *_to_all          src/shmem.h:1507-1743 (signatures identical)
 *   - _SHMEM_* aliases    src/shmem.h:2210-2218
 *   - the minimal runtime  src/shmem.h:156-328 (start_pes/init/finalize/
 *     my_pe/n_pes), :692-797 (barrier_all, barrier, quiet), :974-993
 *     (shmem_malloc/shmem_free)
 *
 * Everything here is implemented in libshmem_reduce.so. The element-wise
 * combine runs as HIP kernels on the PE's GPU (gfx950); see DESIGN.md.
 */
#ifndef _SHMEM_H
#define _SHMEM_H 1

#include <sys/types.h>
#include <stddef.h>

/* C and C++ spell complex numbers differently (reference src/shmem.h:74-80) */
#ifdef __cplusplus
# include <complex>
# define COMPLEXIFY(T) std::complex<T>
#else
# include <complex.h>
# define COMPLEXIFY(T) T _Complex
#endif

/* results that must not be dropped (reference src/shmem.h:94-102) */
#if defined(__GNUC__)                                                   \
    || defined(__PGIC__)                                                \
    || defined(__INTEL_COMPILER)                                        \
    || defined(__OPEN64__)                                              \
    || defined(__OPENUH__)
# define _WUR __attribute__((__warn_unused_result__))
#else
# define _WUR
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define SHMEM_MAJOR_VERSION 1
#define SHMEM_MINOR_VERSION 3
#define SHMEM_MAX_NAME_LEN 64
#define SHMEM_VENDOR_STRING "MI355X OpenSHMEM reduction path"

/* Fortran values are multiples of these (reference src/shmem.h:1495) */
#define SHMEM_INTERNAL_F2C_SCALE        ( sizeof (long) / sizeof (int) )
#define SHMEM_BCAST_SYNC_SIZE           (128L / SHMEM_INTERNAL_F2C_SCALE)
#define SHMEM_BARRIER_SYNC_SIZE         (128L / SHMEM_INTERNAL_F2C_SCALE)
#define SHMEM_REDUCE_SYNC_SIZE          (256L / SHMEM_INTERNAL_F2C_SCALE)
#define SHMEM_REDUCE_MIN_WRKDATA_SIZE   (128L / SHMEM_INTERNAL_F2C_SCALE)

/* pSync arrays must hold this value on entry (reference src/shmem.h:1505) */
#define SHMEM_SYNC_VALUE (-1L)

/* deprecated spellings (reference src/shmem.h:2210-2218) */
#define _SHMEM_MAJOR_VERSION            SHMEM_MAJOR_VERSION
#define _SHMEM_MINOR_VERSION            SHMEM_MINOR_VERSION
#define _SHMEM_MAX_NAME_LEN             SHMEM_MAX_NAME_LEN
#define _SHMEM_VENDOR_STRING            SHMEM_VENDOR_STRING
#define _SHMEM_BCAST_SYNC_SIZE          SHMEM_BCAST_SYNC_SIZE
#define _SHMEM_BARRIER_SYNC_SIZE        SHMEM_BARRIER_SYNC_SIZE
#define _SHMEM_REDUCE_SYNC_SIZE         SHMEM_REDUCE_SYNC_SIZE
#define _SHMEM_REDUCE_MIN_WRKDATA_SIZE  SHMEM_REDUCE_MIN_WRKDATA_SIZE
#define _SHMEM_SYNC_VALUE               SHMEM_SYNC_VALUE

/* ---- minimal runtime (the reduction path needs PEs, a heap, barriers) ---- */
void start_pes (int npes);
void shmem_init (void);
void shmem_finalize (void);
void shmem_global_exit (int status);
int shmem_my_pe (void);
int shmem_n_pes (void);
int _my_pe (void);
int _num_pes (void);
void *shmem_malloc (size_t size);
void shmem_free (void *ptr);
void shmem_barrier_all (void);
void shmem_barrier (int PE_start, int logPE_stride, int PE_size, long *pSync);
void shmem_quiet (void);

/* ---- one-sided put/get (reference src/shmem.h:395-470); the remote
 *      address must be in the device symmetric heap (shmemx_malloc_device) ---- */
void shmem_putmem (void *dest, const void *src, size_t nelems, int pe);
void shmem_getmem (void *dest, const void *src, size_t nelems, int pe);
void shmem_put32 (void *dest, const void *src, size_t nelems, int pe);
void shmem_put64 (void *dest, const void *src, size_t nelems, int pe);
void shmem_put128 (void *dest, const void *src, size_t nelems, int pe);
void shmem_get32 (void *dest, const void *src, size_t nelems, int pe);
void shmem_get64 (void *dest, const void *src, size_t nelems, int pe);
void shmem_get128 (void *dest, const void *src, size_t nelems, int pe);
void shmem_char_put (char *dest, const char *src, size_t nelems, int pe);
void shmem_short_put (short *dest, const short *src, size_t nelems, int pe);
void shmem_int_put (int *dest, const int *src, size_t nelems, int pe);
void shmem_long_put (long *dest, const long *src, size_t nelems, int pe);
void shmem_longlong_put (long long *dest, const long long *src, size_t nelems, int pe);
void shmem_longdouble_put (long double *dest, const long double *src, size_t nelems, int pe);
void shmem_double_put (double *dest, const double *src, size_t nelems, int pe);
void shmem_float_put (float *dest, const float *src, size_t nelems, int pe);
void shmem_char_get (char *dest, const char *src, size_t nelems, int pe);
void shmem_short_get (short *dest, const short *src, size_t nelems, int pe);
void shmem_int_get (int *dest, const int *src, size_t nelems, int pe);
void shmem_long_get (long *dest, const long *src, size_t nelems, int pe);
void shmem_longlong_get (long long *dest, const long long *src, size_t nelems, int pe);
void shmem_longdouble_get (long double *dest, const long double *src, size_t nelems, int pe);
void shmem_double_get (double *dest, const double *src, size_t nelems, int pe);
void shmem_float_get (float *dest, const float *src, size_t nelems, int pe);

/* ---- strided put/get and single elements (reference src/shmem.h:472-560):
 *      target[k * tst] = source[k * sst] for k < nelems, strides in elements
 *      and >= 1; the remote side in the device symmetric heap or the
 *      symmetric host heap. Every other element of the target is left alone.
 *      Blocking, like put/get. ---- */
void shmem_char_iput (char *target, const char *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                      int pe);
void shmem_short_iput (short *target, const short *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                       int pe);
void shmem_int_iput (int *target, const int *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                     int pe);
void shmem_long_iput (long *target, const long *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                      int pe);
void shmem_longlong_iput (long long *target, const long long *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                          int pe);
void shmem_float_iput (float *target, const float *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                       int pe);
void shmem_double_iput (double *target, const double *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                        int pe);
void shmem_longdouble_iput (long double *target, const long double *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                            int pe);
void shmem_iput32 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void shmem_iput64 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void shmem_iput128 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void shmem_char_iget (char *target, const char *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                      int pe);
void shmem_short_iget (short *target, const short *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                       int pe);
void shmem_int_iget (int *target, const int *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                     int pe);
void shmem_long_iget (long *target, const long *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                      int pe);
void shmem_longlong_iget (long long *target, const long long *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                          int pe);
void shmem_float_iget (float *target, const float *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                       int pe);
void shmem_double_iget (double *target, const double *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                        int pe);
void shmem_longdouble_iget (long double *target, const long double *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                            int pe);
void shmem_iget32 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void shmem_iget64 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void shmem_iget128 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void shmem_char_p (char *addr, char value, int pe);
void shmem_short_p (short *addr, short value, int pe);
void shmem_int_p (int *addr, int value, int pe);
void shmem_long_p (long *addr, long value, int pe);
void shmem_longlong_p (long long *addr, long long value, int pe);
void shmem_float_p (float *addr, float value, int pe);
void shmem_double_p (double *addr, double value, int pe);
void shmem_longdouble_p (long double *addr, long double value, int pe);
char shmem_char_g (char *addr, int pe);
short shmem_short_g (short *addr, int pe);
int shmem_int_g (int *addr, int pe);
long shmem_long_g (long *addr, int pe);
long long shmem_longlong_g (long long *addr, int pe);
float shmem_float_g (float *addr, int pe);
double shmem_double_g (double *addr, int pe);
long double shmem_longdouble_g (long double *addr, int pe);

/* ---- ordering (reference src/shmem.h:759-797): every put and atomic of this
 *      build is complete at its target once the library stream has drained,
 *      so shmem_fence is shmem_quiet ---- */
void shmem_fence (void);

/* ---- point-to-point synchronisation (reference src/shmem.h:1044-1123): wait
 *      until this PE's copy of a symmetric variable, in either symmetric
 *      heap, compares true against cmp_value (shmem_wait: until it differs).
 *      A host loop, bounded by SHMEM_WAIT_TIMEOUT ---- */
    enum shmem_cmp_constants
        {
            SHMEM_CMP_EQ = 0,
            SHMEM_CMP_NE,
            SHMEM_CMP_GT,
            SHMEM_CMP_LE,
            SHMEM_CMP_LT,
            SHMEM_CMP_GE
        };
    void shmem_long_wait_until (volatile long *ivar, int cmp, long cmp_value);
    void shmem_short_wait_until (volatile short *ivar, int cmp,
                                 short cmp_value);
    void shmem_int_wait_until (volatile int *ivar, int cmp, int cmp_value);
    void shmem_longlong_wait_until (volatile long long *ivar, int cmp,
                                    long long cmp_value);
    void shmem_long_wait (volatile long *ivar, long cmp_value);
    void shmem_short_wait (volatile short *ivar, short cmp_value);
    void shmem_int_wait (volatile int *ivar, int cmp_value);
    void shmem_longlong_wait (volatile long long *ivar, long long cmp_value);

/* ---- atomics (reference src/shmem.h:1126-1314, :1899-2027): the target in the
 *      device symmetric heap or the symmetric host heap; complete at the
 *      target on return. Integer arithmetic wraps; the float and double forms
 *      move bit patterns ---- */
    long shmem_long_swap (long *target, long value, int pe) _WUR;
    int shmem_int_swap (int *target, int value, int pe) _WUR;
    long long shmem_longlong_swap (long long *target, long long value,
                                   int pe) _WUR;
    float shmem_float_swap (float *target, float value, int pe) _WUR;
    double shmem_double_swap (double *target, double value, int pe) _WUR;
    long shmem_long_cswap (long *target, long cond, long value,
                           int pe) _WUR;
    int shmem_int_cswap (int *target, int cond, int value, int pe) _WUR;
    long long shmem_longlong_cswap (long long *target, long long cond,
                                    long long value, int pe) _WUR;
    long shmem_long_fadd (long *target, long value, int pe) _WUR;
    int shmem_int_fadd (int *target, int value, int pe) _WUR;
    long long shmem_longlong_fadd (long long *target, long long value,
                                   int pe) _WUR;
    long shmem_long_finc (long *target, int pe) _WUR;
    int shmem_int_finc (int *target, int pe) _WUR;
    long long shmem_longlong_finc (long long *target, int pe) _WUR;
    void shmem_long_add (long *target, long value, int pe);
    void shmem_int_add (int *target, int value, int pe);
    void shmem_longlong_add (long long *target, long long value, int pe);
    void shmem_long_inc (long *target, int pe);
    void shmem_int_inc (int *target, int pe);
    void shmem_longlong_inc (long long *target, int pe);
    int shmem_int_fetch (const int *dest, int pe);
    long shmem_long_fetch (const long *dest, int pe);
    long long shmem_longlong_fetch (const long long *dest, int pe);
    float shmem_float_fetch (const float *dest, int pe);
    double shmem_double_fetch (const double *dest, int pe);
    void shmem_int_set (int *dest, int value, int pe);
    void shmem_long_set (long *dest, long value, int pe);
    void shmem_longlong_set (long long *dest, long long value, int pe);
    void shmem_float_set (float *dest, float value, int pe);
    void shmem_double_set (double *dest, double value, int pe);

/* ---- locks (reference src/shmem.h:1808-1896): a symmetric long that starts
 *      at 0; shmem_test_lock returns 0 when it took the lock and never blocks ---- */
    void shmem_set_lock (volatile long *lock);
    void shmem_clear_lock (volatile long *lock);
    int shmem_test_lock (volatile long *lock) _WUR;

/* ---- broadcast / collect (reference src/shmem.h:1746-1779); sources in the
 *      device symmetric heap ---- */
#define SHMEM_COLLECT_SYNC_SIZE (128L / SHMEM_INTERNAL_F2C_SCALE)
#define _SHMEM_COLLECT_SYNC_SIZE SHMEM_COLLECT_SYNC_SIZE
void shmem_broadcast64 (void *target, const void *source, size_t nelems, int PE_root, int PE_start,
                        int logPE_stride, int PE_size, long *pSync);
void shmem_broadcast32 (void *target, const void *source, size_t nelems, int PE_root, int PE_start,
                        int logPE_stride, int PE_size, long *pSync);
void shmem_fcollect64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync);
void shmem_fcollect32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync);
void shmem_collect64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                      int PE_size, long *pSync);
void shmem_collect32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                      int PE_size, long *pSync);

/* ---- all-to-all (reference src/shmem.h:1785-1805); sources in the device
 *      symmetric heap or the symmetric host heap. Member i's block m lands
 *      as block i of member m's target, m and i being indices IN THE ACTIVE
 *      SET; the strided form places and reads elements dst / sst (>= 1)
 *      elements apart and leaves every other element of the target alone. ---- */
#define SHMEM_ALLTOALL_SYNC_SIZE (128L / SHMEM_INTERNAL_F2C_SCALE)
#define SHMEM_ALLTOALLS_SYNC_SIZE (128L / SHMEM_INTERNAL_F2C_SCALE)
void shmem_alltoall32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync);
void shmem_alltoall64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync);
void shmem_alltoalls32 (void *target, const void *source, ptrdiff_t dst, ptrdiff_t sst, size_t nelems,
                        int PE_start, int logPE_stride, int PE_size, long *pSync);
void shmem_alltoalls64 (void *target, const void *source, ptrdiff_t dst, ptrdiff_t sst, size_t nelems,
                        int PE_start, int logPE_stride, int PE_size, long *pSync);

/* ---- reductions: target = op-fold over the active set of source ---- */
    void shmem_short_sum_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void shmem_int_sum_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void shmem_long_sum_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void shmem_longlong_sum_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void shmem_float_sum_to_all (float *target, float *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            float *pWrk, long *pSync);
    void shmem_double_sum_to_all (double *target, double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            double *pWrk, long *pSync);
    void shmem_longdouble_sum_to_all (long double *target, long double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long double *pWrk, long *pSync);
    void shmem_complexf_sum_to_all (COMPLEXIFY (float) *target, COMPLEXIFY (float) *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            COMPLEXIFY (float) *pWrk, long *pSync);
    void shmem_complexd_sum_to_all (COMPLEXIFY (double) *target, COMPLEXIFY (double) *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            COMPLEXIFY (double) *pWrk, long *pSync);
    void shmem_short_prod_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void shmem_int_prod_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void shmem_long_prod_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void shmem_longlong_prod_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void shmem_float_prod_to_all (float *target, float *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            float *pWrk, long *pSync);
    void shmem_double_prod_to_all (double *target, double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            double *pWrk, long *pSync);
    void shmem_longdouble_prod_to_all (long double *target, long double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long double *pWrk, long *pSync);
    void shmem_complexf_prod_to_all (COMPLEXIFY (float) *target, COMPLEXIFY (float) *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            COMPLEXIFY (float) *pWrk, long *pSync);
    void shmem_complexd_prod_to_all (COMPLEXIFY (double) *target, COMPLEXIFY (double) *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            COMPLEXIFY (double) *pWrk, long *pSync);
    void shmem_short_and_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void shmem_int_and_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void shmem_long_and_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void shmem_longlong_and_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void shmem_short_or_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void shmem_int_or_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void shmem_long_or_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void shmem_longlong_or_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void shmem_short_xor_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void shmem_int_xor_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void shmem_long_xor_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void shmem_longlong_xor_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void shmem_short_max_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void shmem_int_max_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void shmem_long_max_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void shmem_longlong_max_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void shmem_float_max_to_all (float *target, float *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            float *pWrk, long *pSync);
    void shmem_double_max_to_all (double *target, double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            double *pWrk, long *pSync);
    void shmem_longdouble_max_to_all (long double *target, long double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long double *pWrk, long *pSync);
    void shmem_short_min_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void shmem_int_min_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void shmem_long_min_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void shmem_longlong_min_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void shmem_float_min_to_all (float *target, float *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            float *pWrk, long *pSync);
    void shmem_double_min_to_all (double *target, double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            double *pWrk, long *pSync);
    void shmem_longdouble_min_to_all (long double *target, long double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long double *pWrk, long *pSync);

/* ---- C11 generic selection over the atomics and waits (reference
 *      src/shmem.h:2112-2201) ---- */
#ifdef __STDC_VERSION__
#if  __STDC_VERSION__ >= 201112L

#define shmem_swap(dest, value, pe)                             \
    _Generic(*(dest),                                           \
             int:          shmem_int_swap,                      \
             long:         shmem_long_swap,                     \
             long long:    shmem_longlong_swap,                 \
             float:        shmem_float_swap,                    \
             double:       shmem_double_swap) (dest, value, pe)

#define shmem_cswap(dest, cond, value, pe)                              \
    _Generic(*(dest),                                                   \
             int:          shmem_int_cswap,                             \
             long:         shmem_long_cswap,                            \
             long long:    shmem_longlong_cswap) (dest, cond, value, pe)

#define shmem_fadd(dest, value, pe)                                 \
    _Generic(*(dest),                                               \
             int:          shmem_int_fadd,                          \
             long:         shmem_long_fadd,                         \
             long long:    shmem_longlong_fadd) (dest, value, pe)

#define shmem_finc(dest, pe)                                \
    _Generic(*(dest),                                       \
             int:          shmem_int_finc,                  \
             long:         shmem_long_finc,                 \
             long long:    shmem_longlong_finc) (dest, pe)

#define shmem_add(dest, value, pe)                                  \
    _Generic(*(dest),                                               \
             int:          shmem_int_add,                           \
             long:         shmem_long_add,                          \
             long long:    shmem_longlong_add) (dest, value, pe)

#define shmem_inc(dest, pe)                                 \
    _Generic(*(dest),                                       \
             int:          shmem_int_inc,                   \
             long:         shmem_long_inc,                  \
             long long:    shmem_longlong_inc) (dest, pe)

#define shmem_fetch(dest, pe)                               \
    _Generic(*(dest),                                       \
             int:          shmem_int_fetch,                 \
             const int:    shmem_int_fetch,                 \
             long:         shmem_long_fetch,                \
             const long:   shmem_long_fetch,                \
             long long:    shmem_longlong_fetch,            \
             const long long: shmem_longlong_fetch,         \
             float:        shmem_float_fetch,               \
             const float:  shmem_float_fetch,               \
             double:       shmem_double_fetch,              \
             const double: shmem_double_fetch) (dest, pe)

#define shmem_set(dest, value, pe)                              \
    _Generic(*(dest),                                           \
             int:          shmem_int_set,                       \
             long:         shmem_long_set,                      \
             long long:    shmem_longlong_set,                  \
             float:        shmem_float_set,                     \
             double:       shmem_double_set) (dest, value, pe)

#define shmem_wait(ivar, cmp_value)                                 \
    _Generic(*(ivar),                                               \
             short:        shmem_short_wait,                        \
             int:          shmem_int_wait,                          \
             long:         shmem_long_wait,                         \
             long long:    shmem_longlong_wait) (ivar, cmp_value)

#define shmem_wait_until(ivar, cmp, cmp_value)                          \
    _Generic(*(ivar),                                                   \
             short:        shmem_short_wait_until,                      \
             int:          shmem_int_wait_until,                        \
             long:         shmem_long_wait_until,                       \
             long long:    shmem_longlong_wait_until) (ivar, cmp, cmp_value)

#endif   /* __STDC_VERSION__ >= 201112L test */
#endif /* __STDC_VERSION__ defined test */

#define _SHMEM_CMP_EQ                   SHMEM_CMP_EQ
#define _SHMEM_CMP_NE                   SHMEM_CMP_NE
#define _SHMEM_CMP_GT                   SHMEM_CMP_GT
#define _SHMEM_CMP_LE                   SHMEM_CMP_LE
#define _SHMEM_CMP_LT                   SHMEM_CMP_LT
#define _SHMEM_CMP_GE                   SHMEM_CMP_GE

#ifdef __cplusplus
}
#endif

#endif /* _SHMEM_H */
