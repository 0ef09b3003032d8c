/*
 * shmem_fortran.h -- C prototypes of the Fortran-callable names exported by
 * libshmem_reduce.so (osss-gasnet_amd/csrc/fortran.c). Fortran programs do not
 * include this; it documents the ABI (every argument by reference, single
 * trailing underscore, INTEGER pSync) for C/ctypes callers and the ABI test.
 *
 * Reference interface: src/fortran/fortran.c:1218-1256 (the 37 REDUCIFY
 * reductions), :95-134 (init and PE queries), :636-645 (barriers, quiet).
 * Each shmem_*_ name is a weak alias of the strong pshmem_*_ name
 * (reference: the #pragma weak block at fortran.c:1108-1216).
 */
#ifndef SHMEM_FORTRAN_H
#define SHMEM_FORTRAN_H 1

#include <stddef.h>

#ifdef __cplusplus
# include <complex>
# define SHMEM_F_COMPLEX(T) std::complex<T>
extern "C" {
#else
# include <complex.h>
# define SHMEM_F_COMPLEX(T) T _Complex
#endif

/* weak names */
void start_pes_ (int *npes);
void shmem_init_ (void);
void shmem_finalize_ (void);
void shmem_global_exit_ (int *status);
int my_pe_ (void);
int num_pes_ (void);
int shmem_my_pe_ (void);
int shmem_n_pes_ (void);
void shmem_barrier_all_ (void);
void shmem_quiet_ (void);
void shmem_barrier_ (int *PE_start, int *logPE_stride, int *PE_size, int *pSync);
void shmem_int2_sum_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void shmem_int4_sum_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void shmem_int8_sum_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void shmem_real4_sum_to_all_ (float *target, float *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, float *pWrk, int *pSync);
void shmem_real8_sum_to_all_ (double *target, double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, double *pWrk, int *pSync);
void shmem_real16_sum_to_all_ (long double *target, long double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long double *pWrk, int *pSync);
void shmem_int2_prod_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void shmem_int4_prod_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void shmem_int8_prod_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void shmem_real4_prod_to_all_ (float *target, float *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, float *pWrk, int *pSync);
void shmem_real8_prod_to_all_ (double *target, double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, double *pWrk, int *pSync);
void shmem_real16_prod_to_all_ (long double *target, long double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long double *pWrk, int *pSync);
void shmem_int2_max_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void shmem_int4_max_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void shmem_int8_max_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void shmem_real4_max_to_all_ (float *target, float *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, float *pWrk, int *pSync);
void shmem_real8_max_to_all_ (double *target, double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, double *pWrk, int *pSync);
void shmem_real16_max_to_all_ (long double *target, long double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long double *pWrk, int *pSync);
void shmem_int2_min_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void shmem_int4_min_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void shmem_int8_min_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void shmem_real4_min_to_all_ (float *target, float *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, float *pWrk, int *pSync);
void shmem_real8_min_to_all_ (double *target, double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, double *pWrk, int *pSync);
void shmem_real16_min_to_all_ (long double *target, long double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long double *pWrk, int *pSync);
void shmem_int2_and_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void shmem_int4_and_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void shmem_int8_and_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void shmem_int2_or_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void shmem_int4_or_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void shmem_int8_or_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void shmem_int2_xor_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void shmem_int4_xor_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void shmem_int8_xor_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void shmem_comp4_sum_to_all_ (SHMEM_F_COMPLEX (float) *target, SHMEM_F_COMPLEX (float) *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, SHMEM_F_COMPLEX (float) *pWrk, int *pSync);
void shmem_comp8_sum_to_all_ (SHMEM_F_COMPLEX (double) *target, SHMEM_F_COMPLEX (double) *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, SHMEM_F_COMPLEX (double) *pWrk, int *pSync);
void shmem_comp4_prod_to_all_ (SHMEM_F_COMPLEX (float) *target, SHMEM_F_COMPLEX (float) *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, SHMEM_F_COMPLEX (float) *pWrk, int *pSync);
void shmem_comp8_prod_to_all_ (SHMEM_F_COMPLEX (double) *target, SHMEM_F_COMPLEX (double) *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, SHMEM_F_COMPLEX (double) *pWrk, int *pSync);
/* all-to-all (reference src/fortran/fortran.c:1272-1321) */
void shmem_alltoall32_ (void *target, const void *source, int *nelems,
        int *PE_start, int *logPE_stride, int *PE_size, int *pSync);
void shmem_alltoall64_ (void *target, const void *source, int *nelems,
        int *PE_start, int *logPE_stride, int *PE_size, int *pSync);
void shmem_alltoalls32_ (void *target, const void *source, ptrdiff_t *dst, ptrdiff_t *sst, int *nelems,
        int *PE_start, int *logPE_stride, int *PE_size, int *pSync);
void shmem_alltoalls64_ (void *target, const void *source, ptrdiff_t *dst, ptrdiff_t *sst, int *nelems,
        int *PE_start, int *logPE_stride, int *PE_size, int *pSync);
/* strided put/get (reference src/fortran/fortran.c:482-573): strides and counts
 * are INTEGERs by reference; element sizes: character 1; integer, logical,
 * real, 4, 32: 4 bytes; double, complex, 8, 64: 8 bytes; 128: 16 bytes */
void shmem_character_iput_ (char *target, const char *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_double_iput_ (double *target, const double *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_integer_iput_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_logical_iput_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_real_iput_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_complex_iput_ (SHMEM_F_COMPLEX (float) *target, const SHMEM_F_COMPLEX (float) *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_iput4_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_iput8_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_iput32_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_iput64_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_iput128_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_character_iget_ (char *target, const char *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_double_iget_ (double *target, const double *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_integer_iget_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_logical_iget_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_real_iget_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_complex_iget_ (SHMEM_F_COMPLEX (float) *target, const SHMEM_F_COMPLEX (float) *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_iget4_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_iget8_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_iget32_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_iget64_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void shmem_iget128_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
/* atomics, waits, locks, fence (reference src/fortran/fortran.c:630-645, :648-938,
 * :1324-1353): int4 int, int8 long, real4 float, real8 double; the untyped names
 * act on default INTEGERs */
void shmem_fence_ (void);
void shmem_int4_wait_until_ (int *ivar, int *cmp, int *cmp_value);
void shmem_int8_wait_until_ (long *ivar, int *cmp, long *cmp_value);
void shmem_wait_until_ (int *ivar, int *cmp, int *cmp_value);
void shmem_int4_wait_ (int *ivar, int *cmp_value);
void shmem_int8_wait_ (long *ivar, long *cmp_value);
void shmem_wait_ (int *ivar, int *cmp_value);
void shmem_int4_inc_ (int *target, int *pe);
void shmem_int8_inc_ (long *target, int *pe);
int shmem_int4_finc_ (int *target, int *pe);
long shmem_int8_finc_ (long *target, int *pe);
void shmem_int4_add_ (int *target, int *value, int *pe);
void shmem_int8_add_ (long *target, long *value, int *pe);
int shmem_int4_fadd_ (int *target, int *value, int *pe);
long shmem_int8_fadd_ (long *target, long *value, int *pe);
int shmem_int4_swap_ (int *target, int *value, int *pe);
long shmem_int8_swap_ (long *target, long *value, int *pe);
float shmem_real4_swap_ (float *target, float *value, int *pe);
double shmem_real8_swap_ (double *target, double *value, int *pe);
int shmem_swap_ (int *target, int *value, int *pe);
int shmem_int4_cswap_ (int *target, int *cond, int *value, int *pe);
long shmem_int8_cswap_ (long *target, long *cond, long *value, int *pe);
int shmem_int4_fetch_ (int *target, int *pe);
long shmem_int8_fetch_ (long *target, int *pe);
float shmem_real4_fetch_ (float *target, int *pe);
double shmem_real8_fetch_ (double *target, int *pe);
void shmem_int4_set_ (int *target, int *val, int *pe);
void shmem_int8_set_ (long *target, long *val, int *pe);
void shmem_real4_set_ (float *target, float *val, int *pe);
void shmem_real8_set_ (double *target, double *val, int *pe);
void shmem_clear_lock_ (long *lock);
void shmem_set_lock_ (long *lock);
int shmem_test_lock_ (long *lock);

/* strong (PSHMEM) names */
void pstart_pes_ (int *npes);
void pshmem_init_ (void);
void pshmem_finalize_ (void);
void pshmem_global_exit_ (int *status);
int pmy_pe_ (void);
int pnum_pes_ (void);
int pshmem_my_pe_ (void);
int pshmem_n_pes_ (void);
void pshmem_barrier_all_ (void);
void pshmem_quiet_ (void);
void pshmem_barrier_ (int *PE_start, int *logPE_stride, int *PE_size, int *pSync);
void pshmem_int2_sum_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void pshmem_int4_sum_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void pshmem_int8_sum_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void pshmem_real4_sum_to_all_ (float *target, float *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, float *pWrk, int *pSync);
void pshmem_real8_sum_to_all_ (double *target, double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, double *pWrk, int *pSync);
void pshmem_real16_sum_to_all_ (long double *target, long double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long double *pWrk, int *pSync);
void pshmem_int2_prod_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void pshmem_int4_prod_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void pshmem_int8_prod_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void pshmem_real4_prod_to_all_ (float *target, float *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, float *pWrk, int *pSync);
void pshmem_real8_prod_to_all_ (double *target, double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, double *pWrk, int *pSync);
void pshmem_real16_prod_to_all_ (long double *target, long double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long double *pWrk, int *pSync);
void pshmem_int2_max_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void pshmem_int4_max_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void pshmem_int8_max_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void pshmem_real4_max_to_all_ (float *target, float *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, float *pWrk, int *pSync);
void pshmem_real8_max_to_all_ (double *target, double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, double *pWrk, int *pSync);
void pshmem_real16_max_to_all_ (long double *target, long double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long double *pWrk, int *pSync);
void pshmem_int2_min_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void pshmem_int4_min_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void pshmem_int8_min_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void pshmem_real4_min_to_all_ (float *target, float *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, float *pWrk, int *pSync);
void pshmem_real8_min_to_all_ (double *target, double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, double *pWrk, int *pSync);
void pshmem_real16_min_to_all_ (long double *target, long double *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long double *pWrk, int *pSync);
void pshmem_int2_and_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void pshmem_int4_and_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void pshmem_int8_and_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void pshmem_int2_or_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void pshmem_int4_or_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void pshmem_int8_or_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void pshmem_int2_xor_to_all_ (short *target, short *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, short *pWrk, int *pSync);
void pshmem_int4_xor_to_all_ (int *target, int *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, int *pWrk, int *pSync);
void pshmem_int8_xor_to_all_ (long *target, long *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, long *pWrk, int *pSync);
void pshmem_comp4_sum_to_all_ (SHMEM_F_COMPLEX (float) *target, SHMEM_F_COMPLEX (float) *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, SHMEM_F_COMPLEX (float) *pWrk, int *pSync);
void pshmem_comp8_sum_to_all_ (SHMEM_F_COMPLEX (double) *target, SHMEM_F_COMPLEX (double) *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, SHMEM_F_COMPLEX (double) *pWrk, int *pSync);
void pshmem_comp4_prod_to_all_ (SHMEM_F_COMPLEX (float) *target, SHMEM_F_COMPLEX (float) *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, SHMEM_F_COMPLEX (float) *pWrk, int *pSync);
void pshmem_comp8_prod_to_all_ (SHMEM_F_COMPLEX (double) *target, SHMEM_F_COMPLEX (double) *source, int *nreduce,
        int *PE_start, int *logPE_stride, int *PE_size, SHMEM_F_COMPLEX (double) *pWrk, int *pSync);

void pshmem_alltoall32_ (void *target, const void *source, int *nelems,
        int *PE_start, int *logPE_stride, int *PE_size, int *pSync);
void pshmem_alltoall64_ (void *target, const void *source, int *nelems,
        int *PE_start, int *logPE_stride, int *PE_size, int *pSync);
void pshmem_alltoalls32_ (void *target, const void *source, ptrdiff_t *dst, ptrdiff_t *sst, int *nelems,
        int *PE_start, int *logPE_stride, int *PE_size, int *pSync);
void pshmem_alltoalls64_ (void *target, const void *source, ptrdiff_t *dst, ptrdiff_t *sst, int *nelems,
        int *PE_start, int *logPE_stride, int *PE_size, int *pSync);
void pshmem_character_iput_ (char *target, const char *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_double_iput_ (double *target, const double *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_integer_iput_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_logical_iput_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_real_iput_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_complex_iput_ (SHMEM_F_COMPLEX (float) *target, const SHMEM_F_COMPLEX (float) *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_iput4_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_iput8_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_iput32_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_iput64_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_iput128_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_character_iget_ (char *target, const char *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_double_iget_ (double *target, const double *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_integer_iget_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_logical_iget_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_real_iget_ (int *target, const int *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_complex_iget_ (SHMEM_F_COMPLEX (float) *target, const SHMEM_F_COMPLEX (float) *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_iget4_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_iget8_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_iget32_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_iget64_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_iget128_ (void *target, const void *source, int *tst, int *sst, int *nelems, int *pe);
void pshmem_fence_ (void);
void pshmem_int4_wait_until_ (int *ivar, int *cmp, int *cmp_value);
void pshmem_int8_wait_until_ (long *ivar, int *cmp, long *cmp_value);
void pshmem_wait_until_ (int *ivar, int *cmp, int *cmp_value);
void pshmem_int4_wait_ (int *ivar, int *cmp_value);
void pshmem_int8_wait_ (long *ivar, long *cmp_value);
void pshmem_wait_ (int *ivar, int *cmp_value);
void pshmem_int4_inc_ (int *target, int *pe);
void pshmem_int8_inc_ (long *target, int *pe);
int pshmem_int4_finc_ (int *target, int *pe);
long pshmem_int8_finc_ (long *target, int *pe);
void pshmem_int4_add_ (int *target, int *value, int *pe);
void pshmem_int8_add_ (long *target, long *value, int *pe);
int pshmem_int4_fadd_ (int *target, int *value, int *pe);
long pshmem_int8_fadd_ (long *target, long *value, int *pe);
int pshmem_int4_swap_ (int *target, int *value, int *pe);
long pshmem_int8_swap_ (long *target, long *value, int *pe);
float pshmem_real4_swap_ (float *target, float *value, int *pe);
double pshmem_real8_swap_ (double *target, double *value, int *pe);
int pshmem_swap_ (int *target, int *value, int *pe);
int pshmem_int4_cswap_ (int *target, int *cond, int *value, int *pe);
long pshmem_int8_cswap_ (long *target, long *cond, long *value, int *pe);
int pshmem_int4_fetch_ (int *target, int *pe);
long pshmem_int8_fetch_ (long *target, int *pe);
float pshmem_real4_fetch_ (float *target, int *pe);
double pshmem_real8_fetch_ (double *target, int *pe);
void pshmem_int4_set_ (int *target, int *val, int *pe);
void pshmem_int8_set_ (long *target, long *val, int *pe);
void pshmem_real4_set_ (float *target, float *val, int *pe);
void pshmem_real8_set_ (double *target, double *val, int *pe);
void pshmem_clear_lock_ (long *lock);
void pshmem_set_lock_ (long *lock);
int pshmem_test_lock_ (long *lock);
#ifdef __cplusplus
}
#endif

#endif /* SHMEM_FORTRAN_H */
