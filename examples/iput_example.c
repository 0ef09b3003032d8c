/*
 * iput_example.c -- a halo exchange of a matrix column with shmem_double_iput
 * and shmem_double_iget, from a plain OpenSHMEM program built against this
 * library:
 *
 *   gcc -std=c99 -Iinclude examples/iput_example.c \
 *       -Losss-gasnet_amd/lib -lshmem_reduce -Wl,-rpath,$PWD/osss-gasnet_amd/lib -o iput_example
 *   tools/oshrun -np 2 ./iput_example
 *
 * Every PE holds a ROWS x COLS row-major matrix of doubles in the device
 * symmetric heap. It puts its last interior column into the left halo column
 * (column 0) of its right-hand neighbour: ROWS elements, COLS apart on both
 * sides, one strided launch. After a barrier it fetches that halo column
 * back from the neighbour with shmem_double_iget into a contiguous host
 * array and checks it, then checks its own halo and that the rest of its
 * matrix was left alone.
 */
#include <stdio.h>
#include <stdlib.h>

#include <shmem.h>
#include <shmemx.h>

#define ROWS 300
#define COLS 37

static double value (int pe, int r, int c) { return 1000.0 * pe + r + c / 64.0; }

int main (void)
{
    shmem_init ();
    const int me = shmem_my_pe (), npes = shmem_n_pes ();
    const int right = (me + 1) % npes, left = (me + npes - 1) % npes;
    const size_t total = (size_t) ROWS * COLS;
    int bad = 0;

    double *mat = (double *) shmemx_malloc_device (total * sizeof (double));
    double *host = (double *) malloc (total * sizeof (double));
    double *col = (double *) malloc (ROWS * sizeof (double));
    for (int r = 0; r < ROWS; ++r)
        for (int c = 0; c < COLS; ++c)
            host[r * COLS + c] = value (me, r, c);
    shmemx_memcpy (mat, host, total * sizeof (double));
    shmem_barrier_all ();

    /* my column COLS - 2 becomes the right-hand neighbour's column 0 */
    shmem_double_iput (mat, mat + (COLS - 2), COLS, COLS, ROWS, right);
    shmem_barrier_all ();

    /* fetch it back: the neighbour's column 0, packed */
    shmem_double_iget (col, mat, 1, COLS, ROWS, right);
    for (int r = 0; r < ROWS; ++r)
        bad += col[r] != value (me, r, COLS - 2);

    /* my own halo came from the left; everything else is as I wrote it */
    shmemx_memcpy (host, mat, total * sizeof (double));
    for (int r = 0; r < ROWS; ++r)
        for (int c = 0; c < COLS; ++c)
            bad += host[r * COLS + c] != (c == 0 ? value (left, r, COLS - 2) : value (me, r, c));

    printf ("PE %d of %d: %s\n", me, npes, bad ? "FAILED" : "PASS");
    shmem_barrier_all ();
    free (col);
    free (host);
    shmemx_free_device (mat);
    shmem_finalize ();
    return bad != 0;
}
