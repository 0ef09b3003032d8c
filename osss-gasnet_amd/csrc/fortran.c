/*
 * fortran.c -- the Fortran-callable reduction surface (callers of the path,
 * SURVEY.md 8b): every argument by reference, names with gfortran's single
 * trailing underscore, pshmem_*_ strong and shmem_*_ weak like the C names.
 *
 * Reference interface replaced: src/fortran/fortran.c:1218-1256 (REDUCIFY:
 * 37 <op>_to_all wrappers over the Fortran kinds int2/int4/int8, real4/8/16,
 * comp4/8), :95-134 (start_pes, shmem_init/finalize/global_exit, my_pe,
 * num_pes, shmem_my_pe, shmem_n_pes) and :636-645 (shmem_barrier,
 * shmem_barrier_all, shmem_quiet). As in the reference, a Fortran pSync is an
 * INTEGER array handed on as `long *` (the C side keeps pSync's contract: it
 * is read, never written, by this build).
 *
 * Kind -> C type (fortran.c:1238-1256): int2 short, int4 int, int8 long,
 * real4 float, real8 double, real16 long double, comp4 float complex,
 * comp8 double complex.
 */
#include <complex.h>

#include <pshmem.h>
#include <shmem.h>

#include "shmem_fortran.h"

#define WEAK_F(name) __attribute__ ((weak, alias ("p" #name)))

/* ---- runtime calls a Fortran reduction caller needs ------------------- */

void pstart_pes_ (int *npes) { (void) npes; pshmem_init (); }
void pshmem_init_ (void) { pshmem_init (); }
void pshmem_finalize_ (void) { pshmem_finalize (); }
void pshmem_global_exit_ (int *status) { pshmem_global_exit (*status); }
int pmy_pe_ (void) { return pshmem_my_pe (); }
int pnum_pes_ (void) { return pshmem_n_pes (); }
int pshmem_my_pe_ (void) { return pshmem_my_pe (); }
int pshmem_n_pes_ (void) { return pshmem_n_pes (); }
void pshmem_barrier_all_ (void) { pshmem_barrier_all (); }
void pshmem_quiet_ (void) { pshmem_quiet (); }
void pshmem_barrier_ (int *PE_start, int *logPE_stride, int *PE_size, int *pSync)
{
    pshmem_barrier (*PE_start, *logPE_stride, *PE_size, (long *) pSync);
}

void start_pes_ (int *npes) WEAK_F (start_pes_);
void shmem_init_ (void) WEAK_F (shmem_init_);
void shmem_finalize_ (void) WEAK_F (shmem_finalize_);
void shmem_global_exit_ (int *status) WEAK_F (shmem_global_exit_);
int my_pe_ (void) WEAK_F (my_pe_);
int num_pes_ (void) WEAK_F (num_pes_);
int shmem_my_pe_ (void) WEAK_F (shmem_my_pe_);
int shmem_n_pes_ (void) WEAK_F (shmem_n_pes_);
void shmem_barrier_all_ (void) WEAK_F (shmem_barrier_all_);
void shmem_quiet_ (void) WEAK_F (shmem_quiet_);
void shmem_barrier_ (int *PE_start, int *logPE_stride, int *PE_size, int *pSync) WEAK_F (shmem_barrier_);

/* ---- the 37 reductions ------------------------------------------------- */

/* (Fortran kind, C entry type name, C type) per op, in the reference's order */
#define F_ARITH(X, Op)                                                                                      \
    X (Op, int2, short, short)                                                                              \
    X (Op, int4, int, int)                                                                                  \
    X (Op, int8, long, long)                                                                                \
    X (Op, real4, float, float)                                                                             \
    X (Op, real8, double, double)                                                                           \
    X (Op, real16, longdouble, long double)
#define F_LOGIC(X, Op)                                                                                      \
    X (Op, int2, short, short)                                                                              \
    X (Op, int4, int, int)                                                                                  \
    X (Op, int8, long, long)
#define F_COMPLEX(X, Op)                                                                                    \
    X (Op, comp4, complexf, float _Complex)                                                                 \
    X (Op, comp8, complexd, double _Complex)

#define F_REDUCTION(Op, Kind, Cname, Ctype)                                                                 \
    void pshmem_##Kind##_##Op##_to_all_ (Ctype *target, Ctype *source, int *nreduce, int *PE_start,         \
                                         int *logPE_stride, int *PE_size, Ctype *pWrk, int *pSync)          \
    {                                                                                                       \
        pshmem_##Cname##_##Op##_to_all (target, source, *nreduce, *PE_start, *logPE_stride, *PE_size, pWrk, \
                                        (long *) pSync);                                                    \
    }                                                                                                       \
    void shmem_##Kind##_##Op##_to_all_ (Ctype *target, Ctype *source, int *nreduce, int *PE_start,          \
                                        int *logPE_stride, int *PE_size, Ctype *pWrk, int *pSync)           \
        WEAK_F (shmem_##Kind##_##Op##_to_all_);

F_ARITH (F_REDUCTION, sum)
F_ARITH (F_REDUCTION, prod)
F_ARITH (F_REDUCTION, max)
F_ARITH (F_REDUCTION, min)
F_LOGIC (F_REDUCTION, and)
F_LOGIC (F_REDUCTION, or)
F_LOGIC (F_REDUCTION, xor)
F_COMPLEX (F_REDUCTION, sum)
F_COMPLEX (F_REDUCTION, prod)

/* ---- all-to-all (reference src/fortran/fortran.c:1272-1321) ------------ */

void pshmem_alltoall32_ (void *target, const void *source, int *nelems, int *PE_start, int *logPE_stride,
                         int *PE_size, int *pSync)
{
    pshmem_alltoall32 (target, source, (size_t) *nelems, *PE_start, *logPE_stride, *PE_size, (long *) pSync);
}
void pshmem_alltoall64_ (void *target, const void *source, int *nelems, int *PE_start, int *logPE_stride,
                         int *PE_size, int *pSync)
{
    pshmem_alltoall64 (target, source, (size_t) *nelems, *PE_start, *logPE_stride, *PE_size, (long *) pSync);
}
void pshmem_alltoalls32_ (void *target, const void *source, ptrdiff_t *dst, ptrdiff_t *sst, int *nelems,
                          int *PE_start, int *logPE_stride, int *PE_size, int *pSync)
{
    pshmem_alltoalls32 (target, source, *dst, *sst, (size_t) *nelems, *PE_start, *logPE_stride, *PE_size,
                        (long *) pSync);
}
void pshmem_alltoalls64_ (void *target, const void *source, ptrdiff_t *dst, ptrdiff_t *sst, int *nelems,
                          int *PE_start, int *logPE_stride, int *PE_size, int *pSync)
{
    pshmem_alltoalls64 (target, source, *dst, *sst, (size_t) *nelems, *PE_start, *logPE_stride, *PE_size,
                        (long *) pSync);
}

void shmem_alltoall32_ (void *target, const void *source, int *nelems, int *PE_start, int *logPE_stride,
                        int *PE_size, int *pSync) WEAK_F (shmem_alltoall32_);
void shmem_alltoall64_ (void *target, const void *source, int *nelems, int *PE_start, int *logPE_stride,
                        int *PE_size, int *pSync) WEAK_F (shmem_alltoall64_);
void shmem_alltoalls32_ (void *target, const void *source, ptrdiff_t *dst, ptrdiff_t *sst, int *nelems,
                         int *PE_start, int *logPE_stride, int *PE_size, int *pSync) WEAK_F (shmem_alltoalls32_);
void shmem_alltoalls64_ (void *target, const void *source, ptrdiff_t *dst, ptrdiff_t *sst, int *nelems,
                         int *PE_start, int *logPE_stride, int *PE_size, int *pSync) WEAK_F (shmem_alltoalls64_);

/* ---- strided put/get (reference src/fortran/fortran.c:482-573) ---------- */

/* Fortran name -> the C entry of its element size, as the reference maps
 * them: character 1 byte; integer, logical, real, 4 and 32: 4 bytes; double,
 * complex, 8 and 64: 8 bytes; 128: 16 bytes. Strides and counts are INTEGERs. */
#define F_STRIDED_ALL(X)                                                                                    \
    X (shmem_character_iput_, pshmem_char_iput, char)                                                       \
    X (shmem_double_iput_, pshmem_double_iput, double)                                                      \
    X (shmem_integer_iput_, pshmem_int_iput, int)                                                           \
    X (shmem_logical_iput_, pshmem_int_iput, int)                                                           \
    X (shmem_real_iput_, pshmem_int_iput, int)                                                              \
    X (shmem_complex_iput_, pshmem_iput64, float _Complex)                                                  \
    X (shmem_iput4_, pshmem_iput32, void)                                                                   \
    X (shmem_iput8_, pshmem_iput64, void)                                                                   \
    X (shmem_iput32_, pshmem_iput32, void)                                                                  \
    X (shmem_iput64_, pshmem_iput64, void)                                                                  \
    X (shmem_iput128_, pshmem_iput128, void)                                                                \
    X (shmem_character_iget_, pshmem_char_iget, char)                                                       \
    X (shmem_double_iget_, pshmem_double_iget, double)                                                      \
    X (shmem_integer_iget_, pshmem_int_iget, int)                                                           \
    X (shmem_logical_iget_, pshmem_int_iget, int)                                                           \
    X (shmem_real_iget_, pshmem_int_iget, int)                                                              \
    X (shmem_complex_iget_, pshmem_iget64, float _Complex)                                                  \
    X (shmem_iget4_, pshmem_iget32, void)                                                                   \
    X (shmem_iget8_, pshmem_iget64, void)                                                                   \
    X (shmem_iget32_, pshmem_iget32, void)                                                                  \
    X (shmem_iget64_, pshmem_iget64, void)                                                                  \
    X (shmem_iget128_, pshmem_iget128, void)

#define F_STRIDED(Fname, Centry, Ctype)                                                                     \
    void p##Fname (Ctype *target, const Ctype *source, int *tst, int *sst, int *nelems, int *pe)            \
    {                                                                                                       \
        Centry (target, source, (ptrdiff_t) *tst, (ptrdiff_t) *sst, (size_t) *nelems, *pe);                 \
    }                                                                                                       \
    void Fname (Ctype *target, const Ctype *source, int *tst, int *sst, int *nelems, int *pe) WEAK_F (Fname);

F_STRIDED_ALL (F_STRIDED)

/* ---- atomics, waits, locks, fence (reference src/fortran/fortran.c:630-645,
 *      :648-938, :1324-1353): int4 -> int, int8 -> long, real4 -> float, real8 ->
 *      double; the untyped shmem_wait_, shmem_wait_until_ and shmem_swap_ act on
 *      default INTEGERs, as there ----------------------------------------- */

void pshmem_fence_ (void) { pshmem_fence (); }
void pshmem_int4_wait_until_ (int *ivar, int *cmp, int *cmp_value) { pshmem_int_wait_until (ivar, *cmp, *cmp_value); }
void pshmem_int8_wait_until_ (long *ivar, int *cmp, long *cmp_value) { pshmem_long_wait_until (ivar, *cmp, *cmp_value); }
void pshmem_wait_until_ (int *ivar, int *cmp, int *cmp_value) { pshmem_int_wait_until (ivar, *cmp, *cmp_value); }
void pshmem_int4_wait_ (int *ivar, int *cmp_value) { pshmem_int_wait (ivar, *cmp_value); }
void pshmem_int8_wait_ (long *ivar, long *cmp_value) { pshmem_long_wait (ivar, *cmp_value); }
void pshmem_wait_ (int *ivar, int *cmp_value) { pshmem_int_wait (ivar, *cmp_value); }
void pshmem_int4_inc_ (int *target, int *pe) { pshmem_int_inc (target, *pe); }
void pshmem_int8_inc_ (long *target, int *pe) { pshmem_long_inc (target, *pe); }
int pshmem_int4_finc_ (int *target, int *pe) { return pshmem_int_finc (target, *pe); }
long pshmem_int8_finc_ (long *target, int *pe) { return pshmem_long_finc (target, *pe); }
void pshmem_int4_add_ (int *target, int *value, int *pe) { pshmem_int_add (target, *value, *pe); }
void pshmem_int8_add_ (long *target, long *value, int *pe) { pshmem_long_add (target, *value, *pe); }
int pshmem_int4_fadd_ (int *target, int *value, int *pe) { return pshmem_int_fadd (target, *value, *pe); }
long pshmem_int8_fadd_ (long *target, long *value, int *pe) { return pshmem_long_fadd (target, *value, *pe); }
int pshmem_int4_swap_ (int *target, int *value, int *pe) { return pshmem_int_swap (target, *value, *pe); }
long pshmem_int8_swap_ (long *target, long *value, int *pe) { return pshmem_long_swap (target, *value, *pe); }
float pshmem_real4_swap_ (float *target, float *value, int *pe) { return pshmem_float_swap (target, *value, *pe); }
double pshmem_real8_swap_ (double *target, double *value, int *pe) { return pshmem_double_swap (target, *value, *pe); }
int pshmem_swap_ (int *target, int *value, int *pe) { return pshmem_int_swap (target, *value, *pe); }
int pshmem_int4_cswap_ (int *target, int *cond, int *value, int *pe) { return pshmem_int_cswap (target, *cond, *value, *pe); }
long pshmem_int8_cswap_ (long *target, long *cond, long *value, int *pe) { return pshmem_long_cswap (target, *cond, *value, *pe); }
int pshmem_int4_fetch_ (int *target, int *pe) { return pshmem_int_fetch (target, *pe); }
long pshmem_int8_fetch_ (long *target, int *pe) { return pshmem_long_fetch (target, *pe); }
float pshmem_real4_fetch_ (float *target, int *pe) { return pshmem_float_fetch (target, *pe); }
double pshmem_real8_fetch_ (double *target, int *pe) { return pshmem_double_fetch (target, *pe); }
void pshmem_int4_set_ (int *target, int *val, int *pe) { pshmem_int_set (target, *val, *pe); }
void pshmem_int8_set_ (long *target, long *val, int *pe) { pshmem_long_set (target, *val, *pe); }
void pshmem_real4_set_ (float *target, float *val, int *pe) { pshmem_float_set (target, *val, *pe); }
void pshmem_real8_set_ (double *target, double *val, int *pe) { pshmem_double_set (target, *val, *pe); }
void pshmem_clear_lock_ (long *lock) { pshmem_clear_lock (lock); }
void pshmem_set_lock_ (long *lock) { pshmem_set_lock (lock); }
int pshmem_test_lock_ (long *lock) { return pshmem_test_lock (lock); }
void shmem_fence_ (void) WEAK_F (shmem_fence_);
void shmem_int4_wait_until_ (int *ivar, int *cmp, int *cmp_value) WEAK_F (shmem_int4_wait_until_);
void shmem_int8_wait_until_ (long *ivar, int *cmp, long *cmp_value) WEAK_F (shmem_int8_wait_until_);
void shmem_wait_until_ (int *ivar, int *cmp, int *cmp_value) WEAK_F (shmem_wait_until_);
void shmem_int4_wait_ (int *ivar, int *cmp_value) WEAK_F (shmem_int4_wait_);
void shmem_int8_wait_ (long *ivar, long *cmp_value) WEAK_F (shmem_int8_wait_);
void shmem_wait_ (int *ivar, int *cmp_value) WEAK_F (shmem_wait_);
void shmem_int4_inc_ (int *target, int *pe) WEAK_F (shmem_int4_inc_);
void shmem_int8_inc_ (long *target, int *pe) WEAK_F (shmem_int8_inc_);
int shmem_int4_finc_ (int *target, int *pe) WEAK_F (shmem_int4_finc_);
long shmem_int8_finc_ (long *target, int *pe) WEAK_F (shmem_int8_finc_);
void shmem_int4_add_ (int *target, int *value, int *pe) WEAK_F (shmem_int4_add_);
void shmem_int8_add_ (long *target, long *value, int *pe) WEAK_F (shmem_int8_add_);
int shmem_int4_fadd_ (int *target, int *value, int *pe) WEAK_F (shmem_int4_fadd_);
long shmem_int8_fadd_ (long *target, long *value, int *pe) WEAK_F (shmem_int8_fadd_);
int shmem_int4_swap_ (int *target, int *value, int *pe) WEAK_F (shmem_int4_swap_);
long shmem_int8_swap_ (long *target, long *value, int *pe) WEAK_F (shmem_int8_swap_);
float shmem_real4_swap_ (float *target, float *value, int *pe) WEAK_F (shmem_real4_swap_);
double shmem_real8_swap_ (double *target, double *value, int *pe) WEAK_F (shmem_real8_swap_);
int shmem_swap_ (int *target, int *value, int *pe) WEAK_F (shmem_swap_);
int shmem_int4_cswap_ (int *target, int *cond, int *value, int *pe) WEAK_F (shmem_int4_cswap_);
long shmem_int8_cswap_ (long *target, long *cond, long *value, int *pe) WEAK_F (shmem_int8_cswap_);
int shmem_int4_fetch_ (int *target, int *pe) WEAK_F (shmem_int4_fetch_);
long shmem_int8_fetch_ (long *target, int *pe) WEAK_F (shmem_int8_fetch_);
float shmem_real4_fetch_ (float *target, int *pe) WEAK_F (shmem_real4_fetch_);
double shmem_real8_fetch_ (double *target, int *pe) WEAK_F (shmem_real8_fetch_);
void shmem_int4_set_ (int *target, int *val, int *pe) WEAK_F (shmem_int4_set_);
void shmem_int8_set_ (long *target, long *val, int *pe) WEAK_F (shmem_int8_set_);
void shmem_real4_set_ (float *target, float *val, int *pe) WEAK_F (shmem_real4_set_);
void shmem_real8_set_ (double *target, double *val, int *pe) WEAK_F (shmem_real8_set_);
void shmem_clear_lock_ (long *lock) WEAK_F (shmem_clear_lock_);
void shmem_set_lock_ (long *lock) WEAK_F (shmem_set_lock_);
int shmem_test_lock_ (long *lock) WEAK_F (shmem_test_lock_);
