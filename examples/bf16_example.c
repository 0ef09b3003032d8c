/*
 * bf16_example.c -- a bfloat16 sum over all PEs with shmemx_bfloat16_sum_to_all,
 * from a plain OpenSHMEM program built against this library:
 *
 *   gcc -std=c99 -Iinclude examples/bf16_example.c \
 *       -Losss-gasnet_amd/lib -lshmem_reduce -Wl,-rpath,$PWD/osss-gasnet_amd/lib -o bf16_example
 *   tools/oshrun -np 2 ./bf16_example
 *
 * Elements travel as their 16 bits (shmemx_bfloat16_t: the upper half of a
 * float). Every PE fills an array in the device symmetric heap, reduces it,
 * and checks EVERY element against the fold done on the host the way the
 * library defines it: this PE's value first, then the other PEs' in ascending
 * order, each step a float addition rounded to bfloat16 (to nearest, ties to
 * even), a NaN result the canonical 0x7FC0.
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
    if (f != f)
        return 0x7FC0;
    return (shmemx_bfloat16_t) ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

static shmemx_bfloat16_t add_bf16 (shmemx_bfloat16_t a, shmemx_bfloat16_t b)
{
    volatile float r = widen (a) + widen (b); /* one float addition, then one rounding */
    return round_bf16 (r);
}

/* PE pe's element i: values of both signs over a few binades, so the
 * roundings matter and the PEs' orders differ */
static shmemx_bfloat16_t value (int pe, int i)
{
    const float x = (float) ((i * 37 + pe * 101) % 1999 - 999) / (float) (1 << ((i + pe) % 9));
    return round_bf16 (x);
}

long pSync[SHMEM_REDUCE_SYNC_SIZE];

int main (void)
{
    for (int i = 0; i < SHMEM_REDUCE_SYNC_SIZE; ++i)
        pSync[i] = SHMEM_SYNC_VALUE;
    shmem_init ();
    const int me = shmem_my_pe (), npes = shmem_n_pes ();
    int bad = 0;

    shmemx_bfloat16_t *src = (shmemx_bfloat16_t *) shmemx_malloc_device (N * sizeof *src);
    shmemx_bfloat16_t *dst = (shmemx_bfloat16_t *) shmemx_malloc_device (N * sizeof *dst);
    shmemx_bfloat16_t *host = (shmemx_bfloat16_t *) malloc (N * sizeof *host);
    for (int i = 0; i < N; ++i)
        host[i] = value (me, i);
    shmemx_memcpy (src, host, N * sizeof *src);
    shmem_barrier_all ();

    shmemx_bfloat16_sum_to_all (dst, src, N, 0, 0, npes, NULL, pSync);

    shmemx_memcpy (host, dst, N * sizeof *dst);
    for (int i = 0; i < N; ++i) {
        shmemx_bfloat16_t want = value (me, i);
        for (int pe = 0; pe < npes; ++pe)
            if (pe != me)
                want = add_bf16 (want, value (pe, i));
        bad += host[i] != want;
    }

    printf ("PE %d of %d: %s\n", me, npes, bad ? "FAILED" : "PASS");
    shmem_barrier_all ();
    free (host);
    shmemx_free_device (dst);
    shmemx_free_device (src);
    shmem_finalize ();
    return bad != 0;
}
