/*
 * wsum_example.c -- bfloat16 partial gradients summed into an fp32 buffer on
 * every PE with shmemx_bfloat16_wsum_to_all_float, from a plain OpenSHMEM
 * program built against this library:
 *
 *   gcc -std=c99 -Iinclude examples/wsum_example.c \
 *       -Losss-gasnet_amd/lib -lshmem_reduce -Wl,-rpath,$PWD/osss-gasnet_amd/lib -o wsum_example
 *   tools/oshrun -np 2 ./wsum_example
 *
 * Data-parallel training: every PE holds its replica's gradient in bfloat16
 * and an fp32 master buffer the optimizer reads. One wide sum gives every PE
 * the gradients' sum accumulated in binary32, in ascending PE order, with no
 * rounding to bfloat16 on the way and no second pass -- and the same bits on
 * every PE, so the replicas cannot drift apart. Checked element by element
 * against the same float additions on the host; PE 0's digest of the result is
 * compared with every other PE's.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <shmem.h>
#include <shmemx.h>

#define N 100003

static float widen (shmemx_bfloat16_t b)
{
    const uint32_t u = (uint32_t) b << 16;
    float f;
    memcpy (&f, &u, sizeof f);
    return f;
}

static shmemx_bfloat16_t round_bf16 (float f)
{
    uint32_t u;
    memcpy (&u, &f, sizeof u);
    return (shmemx_bfloat16_t) ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

/* PE pe's gradient element i: both signs over a few binades, so that a sum
 * rounded to bfloat16 at every step would lose bits the float sum keeps */
static shmemx_bfloat16_t grad (int pe, int i)
{
    return round_bf16 ((float) ((i * 37 + pe * 101) % 1999 - 999) / (float) (1 << ((i + pe) % 9)));
}

int main (void)
{
    shmem_init ();
    const int me = shmem_my_pe (), npes = shmem_n_pes ();
    int bad = 0;

    shmemx_bfloat16_t *g = (shmemx_bfloat16_t *) shmemx_malloc_device (N * sizeof *g);
    float *master = (float *) shmemx_malloc_device (N * sizeof *master);
    shmemx_bfloat16_t *hg = (shmemx_bfloat16_t *) malloc (N * sizeof *hg);
    float *hm = (float *) malloc (N * sizeof *hm);
    for (int i = 0; i < N; ++i)
        hg[i] = grad (me, i);
    shmemx_memcpy (g, hg, N * sizeof *g);
    shmem_barrier_all ();

    shmemx_bfloat16_wsum_to_all_float (master, g, N, 0, 0, npes);

    shmemx_memcpy (hm, master, N * sizeof *master);
    unsigned long digest = 0;
    for (int i = 0; i < N; ++i) {
        volatile float want = widen (grad (0, i));
        for (int pe = 1; pe < npes; ++pe)
            want = want + widen (grad (pe, i)); /* one float addition per PE, ascending */
        const float w = want;
        uint32_t u;
        bad += memcmp (&hm[i], &w, sizeof w) != 0;
        memcpy (&u, &hm[i], sizeof u);
        digest = digest * 31 + u;
    }

    /* every replica holds the same bits: PE p's digest lands in slot p on PE 0 */
    long *digest_all = (long *) shmem_malloc ((size_t) npes * sizeof *digest_all);
    shmem_long_p (&digest_all[me], (long) digest, 0);
    shmem_barrier_all ();
    if (me == 0)
        for (int pe = 1; pe < npes; ++pe)
            bad += (unsigned long) digest_all[pe] != digest;

    printf ("PE %d of %d: %s\n", me, npes, bad ? "FAILED" : "OK");
    shmem_barrier_all ();
    shmem_free (digest_all);
    free (hm);
    free (hg);
    shmemx_free_device (master);
    shmemx_free_device (g);
    shmem_finalize ();
    return bad != 0;
}
