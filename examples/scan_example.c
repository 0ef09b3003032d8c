/*
 * scan_example.c -- the scan collectives from a plain OpenSHMEM program built
 * against this library:
 *
 *   gcc -std=c99 -Iinclude examples/scan_example.c \
 *       -Losss-gasnet_amd/lib -lshmem_reduce -Wl,-rpath,$PWD/osss-gasnet_amd/lib -o scan_example
 *   tools/oshrun -np 3 ./scan_example
 *
 * 1. Offsets from counts: every PE holds how many records it has in each of
 *    NBINS bins; an exscan of the counts gives, per bin, the offset at which
 *    this PE's records start in the concatenation over the PEs. PE 0's target
 *    is left untouched by an exscan, so it is set to 0 beforehand.
 * 2. A running sum of doubles with inscan: PE j receives the sum over PEs
 *    0 .. j, added in that order -- checked bit for bit against the same
 *    additions done on the host.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <shmem.h>
#include <shmemx.h>

#define NBINS 1000
#define N 50003

static int count_of (int pe, int bin) { return (bin * 7 + pe * 13) % 23; }

static double value (int pe, int i) { return (double) ((i * 37 + pe * 101) % 1999 - 999) / (double) (1 << ((i + pe) % 9)) + 1e-3 * pe; }

long pSync[SHMEM_REDUCE_SYNC_SIZE];

int main (void)
{
    for (int i = 0; i < SHMEM_REDUCE_SYNC_SIZE; ++i)
        pSync[i] = SHMEM_SYNC_VALUE;
    shmem_init ();
    const int me = shmem_my_pe (), npes = shmem_n_pes ();
    int bad = 0;

    /* 1. offsets = exscan of the counts */
    int *counts = (int *) shmemx_malloc_device (NBINS * sizeof *counts);
    int *offsets = (int *) shmemx_malloc_device (NBINS * sizeof *offsets);
    int *hi = (int *) malloc (NBINS * sizeof *hi);
    for (int b = 0; b < NBINS; ++b)
        hi[b] = count_of (me, b);
    shmemx_memcpy (counts, hi, NBINS * sizeof *counts);
    memset (hi, 0, NBINS * sizeof *hi); /* PE 0 keeps these zeros: exscan does not write its target */
    shmemx_memcpy (offsets, hi, NBINS * sizeof *offsets);
    shmem_barrier_all ();

    shmemx_int_sum_exscan (offsets, counts, NBINS, 0, 0, npes, NULL, pSync);

    shmemx_memcpy (hi, offsets, NBINS * sizeof *offsets);
    for (int b = 0; b < NBINS; ++b) {
        int want = 0;
        for (int pe = 0; pe < me; ++pe)
            want += count_of (pe, b);
        bad += hi[b] != want;
    }

    /* 2. a running sum of doubles */
    double *x = (double *) shmemx_malloc_device (N * sizeof *x);
    double *run = (double *) shmemx_malloc_device (N * sizeof *run);
    double *hd = (double *) malloc (N * sizeof *hd);
    for (int i = 0; i < N; ++i)
        hd[i] = value (me, i);
    shmemx_memcpy (x, hd, N * sizeof *x);
    shmem_barrier_all ();

    shmemx_double_sum_inscan (run, x, N, 0, 0, npes, NULL, pSync);

    shmemx_memcpy (hd, run, N * sizeof *run);
    for (int i = 0; i < N; ++i) {
        volatile double want = value (0, i);
        for (int pe = 1; pe <= me; ++pe)
            want = want + value (pe, i);
        const double w = want;
        bad += memcmp (&hd[i], &w, sizeof w) != 0;
    }

    printf ("PE %d of %d: %s\n", me, npes, bad ? "FAILED" : "PASS");
    shmem_barrier_all ();
    free (hd);
    free (hi);
    shmemx_free_device (run);
    shmemx_free_device (x);
    shmemx_free_device (offsets);
    shmemx_free_device (counts);
    shmem_finalize ();
    return bad != 0;
}
