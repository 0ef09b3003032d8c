/*
 * pshmem.h -- profiling (PSHMEM) names of the reduction surface.
 *
 * The reference exports every reduction as a strong pshmem_ symbol with the
 * shmem_ name as a weak alias (src/reduce/reduce-op.c:291-380; declarations
 * src/pshmem.h:545-735). libshmem_reduce.so does the same, so a tool can
 * interpose shmem_* and forward to pshmem_*.
 */
#ifndef _PSHMEM_H
#define _PSHMEM_H 1

#include <shmem.h>

#ifdef __cplusplus
extern "C" {
#endif

void pstart_pes (int npes);
void pshmem_init (void);
void pshmem_finalize (void);
void pshmem_global_exit (int status);
int pshmem_my_pe (void);
int pshmem_n_pes (void);
void *pshmem_malloc (size_t size);
void pshmem_free (void *ptr);
void pshmem_barrier_all (void);
void pshmem_barrier (int PE_start, int logPE_stride, int PE_size, long *pSync);
void pshmem_quiet (void);

void pshmem_fence (void);

    void pshmem_short_wait_until (volatile short *ivar, int cmp,
                                  short cmp_value);
    void pshmem_int_wait_until (volatile int *ivar, int cmp, int cmp_value);
    void pshmem_long_wait_until (volatile long *ivar, int cmp, long cmp_value);
    void pshmem_longlong_wait_until (volatile long long *ivar, int cmp,
                                            long long cmp_value);
    void pshmem_short_wait (volatile short *ivar, short cmp_value);
    void pshmem_int_wait (volatile int *ivar, int cmp_value);
    void pshmem_long_wait (volatile long *ivar, long cmp_value);
    void pshmem_longlong_wait (volatile long long *ivar, long long cmp_value);
    int pshmem_int_swap (int *target, int value, int pe) _WUR;
    long pshmem_long_swap (long *target, long value, int pe) _WUR;
    long long pshmem_longlong_swap (long long *target, long long value,
                                           int pe) _WUR;
    float pshmem_float_swap (float *target, float value, int pe) _WUR;
    double pshmem_double_swap (double *target, double value,
                                      int pe) _WUR;
    int pshmem_int_cswap (int *target, int cond, int value, int pe) _WUR;
    long pshmem_long_cswap (long *target, long cond, long value,
                                   int pe) _WUR;
    long long pshmem_longlong_cswap (long long *target, long long cond,
                                            long long value, int pe) _WUR;
    int pshmem_int_fadd (int *target, int value, int pe) _WUR;
    long pshmem_long_fadd (long *target, long value, int pe) _WUR;
    long long pshmem_longlong_fadd (long long *target, long long value,
                                           int pe) _WUR;
    int pshmem_int_finc (int *target, int pe) _WUR;
    long pshmem_long_finc (long *target, int pe) _WUR;
    long long pshmem_longlong_finc (long long *target, int pe) _WUR;
    void pshmem_int_add (int *target, int value, int pe);
    void pshmem_long_add (long *target, long value, int pe);
    void pshmem_longlong_add (long long *target, long long value,
                                     int pe);
    void pshmem_int_inc (int *target, int pe);
    void pshmem_long_inc (long *target, int pe);
    void pshmem_longlong_inc (long long *target, int pe);
    void pshmem_set_lock (volatile long *lock);
    void pshmem_clear_lock (volatile long *lock);
    int  pshmem_test_lock (volatile long *lock) _WUR;
    int pshmem_int_fetch (const int *target, int pe);
    long pshmem_long_fetch (const long *target, int pe);
    long long pshmem_longlong_fetch (const long long *target, int pe);
    float pshmem_float_fetch (const float *target, int pe);
    double pshmem_double_fetch (const double *target, int pe);
    void pshmem_int_set (int *target, int value, int pe);
    void pshmem_long_set (long *target, long value, int pe);
    void pshmem_longlong_set (long long *target, long long value, int pe);
    void pshmem_float_set (float *target, float value, int pe);
    void pshmem_double_set (double *target, double value, int pe);

void pshmem_putmem (void *dest, const void *src, size_t nelems, int pe);
void pshmem_getmem (void *dest, const void *src, size_t nelems, int pe);
void pshmem_put32 (void *dest, const void *src, size_t nelems, int pe);
void pshmem_put64 (void *dest, const void *src, size_t nelems, int pe);
void pshmem_put128 (void *dest, const void *src, size_t nelems, int pe);
void pshmem_get32 (void *dest, const void *src, size_t nelems, int pe);
void pshmem_get64 (void *dest, const void *src, size_t nelems, int pe);
void pshmem_get128 (void *dest, const void *src, size_t nelems, int pe);
void pshmem_char_put (char *dest, const char *src, size_t nelems, int pe);
void pshmem_short_put (short *dest, const short *src, size_t nelems, int pe);
void pshmem_int_put (int *dest, const int *src, size_t nelems, int pe);
void pshmem_long_put (long *dest, const long *src, size_t nelems, int pe);
void pshmem_longlong_put (long long *dest, const long long *src, size_t nelems, int pe);
void pshmem_longdouble_put (long double *dest, const long double *src, size_t nelems, int pe);
void pshmem_double_put (double *dest, const double *src, size_t nelems, int pe);
void pshmem_float_put (float *dest, const float *src, size_t nelems, int pe);
void pshmem_char_get (char *dest, const char *src, size_t nelems, int pe);
void pshmem_short_get (short *dest, const short *src, size_t nelems, int pe);
void pshmem_int_get (int *dest, const int *src, size_t nelems, int pe);
void pshmem_long_get (long *dest, const long *src, size_t nelems, int pe);
void pshmem_longlong_get (long long *dest, const long long *src, size_t nelems, int pe);
void pshmem_longdouble_get (long double *dest, const long double *src, size_t nelems, int pe);
void pshmem_double_get (double *dest, const double *src, size_t nelems, int pe);
void pshmem_float_get (float *dest, const float *src, size_t nelems, int pe);
void pshmem_char_iput (char *target, const char *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                       int pe);
void pshmem_short_iput (short *target, const short *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                        int pe);
void pshmem_int_iput (int *target, const int *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                      int pe);
void pshmem_long_iput (long *target, const long *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                       int pe);
void pshmem_longlong_iput (long long *target, const long long *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                           int pe);
void pshmem_float_iput (float *target, const float *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                        int pe);
void pshmem_double_iput (double *target, const double *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                         int pe);
void pshmem_longdouble_iput (long double *target, const long double *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                             int pe);
void pshmem_iput32 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void pshmem_iput64 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void pshmem_iput128 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void pshmem_char_iget (char *target, const char *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                       int pe);
void pshmem_short_iget (short *target, const short *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                        int pe);
void pshmem_int_iget (int *target, const int *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                      int pe);
void pshmem_long_iget (long *target, const long *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                       int pe);
void pshmem_longlong_iget (long long *target, const long long *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                           int pe);
void pshmem_float_iget (float *target, const float *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                        int pe);
void pshmem_double_iget (double *target, const double *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                         int pe);
void pshmem_longdouble_iget (long double *target, const long double *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                             int pe);
void pshmem_iget32 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void pshmem_iget64 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void pshmem_iget128 (void *target, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems, int pe);
void pshmem_char_p (char *addr, char value, int pe);
void pshmem_short_p (short *addr, short value, int pe);
void pshmem_int_p (int *addr, int value, int pe);
void pshmem_long_p (long *addr, long value, int pe);
void pshmem_longlong_p (long long *addr, long long value, int pe);
void pshmem_float_p (float *addr, float value, int pe);
void pshmem_double_p (double *addr, double value, int pe);
void pshmem_longdouble_p (long double *addr, long double value, int pe);
char pshmem_char_g (char *addr, int pe);
short pshmem_short_g (short *addr, int pe);
int pshmem_int_g (int *addr, int pe);
long pshmem_long_g (long *addr, int pe);
long long pshmem_longlong_g (long long *addr, int pe);
float pshmem_float_g (float *addr, int pe);
double pshmem_double_g (double *addr, int pe);
long double pshmem_longdouble_g (long double *addr, int pe);
void pshmem_broadcast64 (void *target, const void *source, size_t nelems, int PE_root, int PE_start,
                         int logPE_stride, int PE_size, long *pSync);
void pshmem_broadcast32 (void *target, const void *source, size_t nelems, int PE_root, int PE_start,
                         int logPE_stride, int PE_size, long *pSync);
void pshmem_fcollect64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                        int PE_size, long *pSync);
void pshmem_fcollect32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                        int PE_size, long *pSync);
void pshmem_collect64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync);
void pshmem_collect32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                       int PE_size, long *pSync);
void pshmem_alltoall32 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                        int PE_size, long *pSync);
void pshmem_alltoall64 (void *target, const void *source, size_t nelems, int PE_start, int logPE_stride,
                        int PE_size, long *pSync);
void pshmem_alltoalls32 (void *target, const void *source, ptrdiff_t dst, ptrdiff_t sst, size_t nelems,
                         int PE_start, int logPE_stride, int PE_size, long *pSync);
void pshmem_alltoalls64 (void *target, const void *source, ptrdiff_t dst, ptrdiff_t sst, size_t nelems,
                         int PE_start, int logPE_stride, int PE_size, long *pSync);

    void pshmem_short_sum_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void pshmem_int_sum_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void pshmem_long_sum_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void pshmem_longlong_sum_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void pshmem_float_sum_to_all (float *target, float *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            float *pWrk, long *pSync);
    void pshmem_double_sum_to_all (double *target, double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            double *pWrk, long *pSync);
    void pshmem_longdouble_sum_to_all (long double *target, long double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long double *pWrk, long *pSync);
    void pshmem_complexf_sum_to_all (COMPLEXIFY (float) *target, COMPLEXIFY (float) *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            COMPLEXIFY (float) *pWrk, long *pSync);
    void pshmem_complexd_sum_to_all (COMPLEXIFY (double) *target, COMPLEXIFY (double) *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            COMPLEXIFY (double) *pWrk, long *pSync);
    void pshmem_short_prod_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void pshmem_int_prod_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void pshmem_long_prod_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void pshmem_longlong_prod_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void pshmem_float_prod_to_all (float *target, float *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            float *pWrk, long *pSync);
    void pshmem_double_prod_to_all (double *target, double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            double *pWrk, long *pSync);
    void pshmem_longdouble_prod_to_all (long double *target, long double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long double *pWrk, long *pSync);
    void pshmem_complexf_prod_to_all (COMPLEXIFY (float) *target, COMPLEXIFY (float) *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            COMPLEXIFY (float) *pWrk, long *pSync);
    void pshmem_complexd_prod_to_all (COMPLEXIFY (double) *target, COMPLEXIFY (double) *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            COMPLEXIFY (double) *pWrk, long *pSync);
    void pshmem_short_and_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void pshmem_int_and_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void pshmem_long_and_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void pshmem_longlong_and_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void pshmem_short_or_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void pshmem_int_or_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void pshmem_long_or_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void pshmem_longlong_or_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void pshmem_short_xor_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void pshmem_int_xor_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void pshmem_long_xor_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void pshmem_longlong_xor_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void pshmem_short_max_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void pshmem_int_max_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void pshmem_long_max_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void pshmem_longlong_max_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void pshmem_float_max_to_all (float *target, float *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            float *pWrk, long *pSync);
    void pshmem_double_max_to_all (double *target, double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            double *pWrk, long *pSync);
    void pshmem_longdouble_max_to_all (long double *target, long double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long double *pWrk, long *pSync);
    void pshmem_short_min_to_all (short *target, short *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            short *pWrk, long *pSync);
    void pshmem_int_min_to_all (int *target, int *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            int *pWrk, long *pSync);
    void pshmem_long_min_to_all (long *target, long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long *pWrk, long *pSync);
    void pshmem_longlong_min_to_all (long long *target, long long *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long long *pWrk, long *pSync);
    void pshmem_float_min_to_all (float *target, float *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            float *pWrk, long *pSync);
    void pshmem_double_min_to_all (double *target, double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            double *pWrk, long *pSync);
    void pshmem_longdouble_min_to_all (long double *target, long double *source,
            int nreduce, int PE_start, int logPE_stride, int PE_size,
            long double *pWrk, long *pSync);

#ifdef __cplusplus
}
#endif

#endif /* _PSHMEM_H */
