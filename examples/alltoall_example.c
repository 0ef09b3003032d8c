/*
 * alltoall_example.c -- shmem_alltoall64 and shmem_alltoalls32 from a plain
 * OpenSHMEM 1.3 program, built against this library:
 *
 *   gcc -std=c99 -Iinclude examples/alltoall_example.c \
 *       -Losss-gasnet_amd/lib -lshmem_reduce -Wl,-rpath,$PWD/osss-gasnet_amd/lib -o alltoall_example
 *   tools/oshrun -np 4 ./alltoall_example
 *
 * Every PE sends block m of its source to PE m and receives PE i's block as
 * block i of its target: first device-resident 64-bit elements, contiguous,
 * then 32-bit elements in the symmetric host heap, placed 2 apart in the
 * target and read 3 apart in the source. Each PE checks its own result and
 * that the elements between the strided ones were left alone.
 */
#include <stdio.h>
#include <stdlib.h>

#include <shmem.h>
#include <shmemx.h>

#define NELEMS 300
#define DST 2
#define SST 3

static long pSync[SHMEM_ALLTOALL_SYNC_SIZE];

static long value (int pe, int block, int k) { return 1000003L * pe + 1009L * block + k; }

int main (void)
{
    for (int i = 0; i < SHMEM_ALLTOALL_SYNC_SIZE; ++i)
        pSync[i] = SHMEM_SYNC_VALUE;
    shmem_init ();
    const int me = shmem_my_pe (), npes = shmem_n_pes ();
    const size_t total = (size_t) npes * NELEMS;
    int bad = 0;

    /* contiguous, device-resident */
    long *dsrc = (long *) shmemx_malloc_device (total * sizeof (long));
    long *ddst = (long *) shmemx_malloc_device (total * sizeof (long));
    long *host = (long *) malloc (total * sizeof (long));
    for (int b = 0; b < npes; ++b)
        for (int k = 0; k < NELEMS; ++k)
            host[b * NELEMS + k] = value (me, b, k);
    shmemx_memcpy (dsrc, host, total * sizeof (long));
    shmem_alltoall64 (ddst, dsrc, NELEMS, 0, 0, npes, pSync);
    shmemx_memcpy (host, ddst, total * sizeof (long));
    for (int i = 0; i < npes; ++i)
        for (int k = 0; k < NELEMS; ++k)
            bad += host[i * NELEMS + k] != value (i, me, k);
    shmem_barrier_all (); /* pSync may be reused after a barrier */

    /* strided, in the symmetric host heap */
    int *ssrc = (int *) shmem_malloc (total * SST * sizeof (int));
    int *sdst = (int *) shmem_malloc (total * DST * sizeof (int));
    for (size_t j = 0; j < total * SST; ++j)
        ssrc[j] = -1;
    for (size_t j = 0; j < total * DST; ++j)
        sdst[j] = -7;
    for (int b = 0; b < npes; ++b)
        for (int k = 0; k < NELEMS; ++k)
            ssrc[(size_t) (b * NELEMS + k) * SST] = (int) value (me, b, k);
    shmem_barrier_all ();
    shmem_alltoalls32 (sdst, ssrc, DST, SST, NELEMS, 0, 0, npes, pSync);
    for (int i = 0; i < npes; ++i)
        for (int k = 0; k < NELEMS; ++k) {
            const size_t j = (size_t) (i * NELEMS + k) * DST;
            bad += sdst[j] != (int) value (i, me, k);
            bad += sdst[j + 1] != -7; /* the gap element */
        }

    printf ("PE %d of %d: %s\n", me, npes, bad ? "FAILED" : "PASS");
    shmem_free (sdst);
    shmem_free (ssrc);
    free (host);
    shmemx_free_device (ddst);
    shmemx_free_device (dsrc);
    shmem_finalize ();
    return bad != 0;
}
