/* A caller of shmem_iput4_, shmem_character_iget_ and shmem_iget128_ the way
 * gfortran calls them: every argument by reference, strides and counts
 * INTEGERs (tests/test_gpu_iputget.py, 2 PEs).
 *   iput4          device heap -> the next PE's device heap, 3 apart from 2 apart
 *   character_iget the previous PE's host heap -> host memory, 2 apart from 5 apart
 *   iget128        the previous PE's device heap -> host memory, packed from 3 apart */
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <shmem.h>
#include <shmem_fortran.h>
#include <shmemx.h>

#define N 300

int main (void)
{
    shmem_init_ ();
    const int me = shmem_my_pe_ (), npes = shmem_n_pes_ ();
    int right = (me + 1) % npes, left = (me + npes - 1) % npes, nelems = N, bad = 0;

    /* shmem_iput4_ */
    int *dsrc = (int *) shmemx_malloc_device (N * 2 * sizeof (int));
    int *ddst = (int *) shmemx_malloc_device (N * 3 * sizeof (int));
    int *h = (int *) malloc (N * 3 * sizeof (int));
    for (int j = 0; j < N * 2; ++j)
        h[j] = 100003 * me + j;
    shmemx_memcpy (dsrc, h, N * 2 * sizeof (int));
    for (int j = 0; j < N * 3; ++j)
        h[j] = -7;
    shmemx_memcpy (ddst, h, N * 3 * sizeof (int));
    shmem_barrier_all_ ();
    int tst = 3, sst = 2;
    shmem_iput4_ (ddst, dsrc, &tst, &sst, &nelems, &right);
    shmem_barrier_all_ ();
    shmemx_memcpy (h, ddst, N * 3 * sizeof (int));
    for (int j = 0; j < N * 3; ++j)
        bad += h[j] != (j % 3 == 0 ? 100003 * left + (j / 3) * 2 : -7);

    /* shmem_character_iget_ */
    char *csrc = (char *) shmem_malloc (N * 5);
    char cdst[N * 2];
    for (int j = 0; j < N * 5; ++j)
        csrc[j] = (char) (me * 31 + j);
    memset (cdst, 'x', sizeof cdst);
    shmem_barrier_all_ ();
    tst = 2, sst = 5;
    shmem_character_iget_ (cdst, csrc, &tst, &sst, &nelems, &left);
    for (int j = 0; j < N * 2; ++j)
        bad += cdst[j] != (j % 2 == 0 ? (char) (left * 31 + (j / 2) * 5) : 'x');

    /* shmem_iget128_ */
    long double *qsrc = (long double *) shmemx_malloc_device (N * 3 * sizeof (long double));
    long double *q = (long double *) malloc (N * 3 * sizeof (long double));
    long double qdst[N + 1];
    memset (q, 0, N * 3 * sizeof (long double));
    for (int j = 0; j < N * 3; ++j)
        q[j] = 0.5L * j + me;
    shmemx_memcpy (qsrc, q, N * 3 * sizeof (long double));
    for (int j = 0; j < N + 1; ++j)
        qdst[j] = -7.0L;
    shmem_barrier_all_ ();
    tst = 1, sst = 3;
    shmem_iget128_ (qdst, qsrc, &tst, &sst, &nelems, &left);
    for (int k = 0; k < N; ++k)
        bad += qdst[k] != 0.5L * (k * 3) + left;
    bad += qdst[N] != -7.0L;

    printf ("PE %d of %d: %s\n", me, npes, bad ? "FAILED" : "PASS");
    shmem_barrier_all_ ();
    free (q);
    free (h);
    shmemx_free_device (qsrc);
    shmem_free (csrc);
    shmemx_free_device (ddst);
    shmemx_free_device (dsrc);
    shmem_finalize_ ();
    return bad != 0;
}
