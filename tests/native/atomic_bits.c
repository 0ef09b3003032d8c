/*
 * atomic_bits.c -- the float and double forms of shmem_<T>_set / fetch / swap
 * move bit patterns: a signalling-NaN payload, -0.0 and a subnormal arrive
 * bit for bit on the right-hand neighbour and come back bit for bit. Written
 * in C because a float signalling NaN does not survive a conversion to a
 * Python float. Argument "host": shmem_malloc's heap (runs without a GPU);
 * otherwise the device heap.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <shmem.h>
#include <shmemx.h>

static int host;

static void copy (void *dst, const void *src, size_t n)
{
    if (host)
        memcpy (dst, src, n);
    else
        shmemx_memcpy (dst, src, n);
}

static float f_of (uint32_t b) { float v; memcpy (&v, &b, 4); return v; }
static uint32_t b_of_f (float v) { uint32_t b; memcpy (&b, &v, 4); return b; }
static double d_of (uint64_t b) { double v; memcpy (&v, &b, 8); return v; }
static uint64_t b_of_d (double v) { uint64_t b; memcpy (&b, &v, 8); return b; }

int main (int argc, char **argv)
{
    host = argc > 1 && strcmp (argv[1], "host") == 0;
    shmem_init ();
    const int me = shmem_my_pe (), npes = shmem_n_pes (), right = (me + 1) % npes;
    static const uint32_t fp[] = {0x7FA12345u /* sNaN + payload */, 0xFFA00001u, 0x80000000u /* -0.0 */,
                                  0x00000001u /* subnormal */, 0x807FFFFFu, 0x3F800000u};
    static const uint64_t dp[] = {0x7FF4000012345678ull, 0xFFF0000000000001ull, 0x8000000000000000ull,
                                  0x0000000000000001ull, 0x800FFFFFFFFFFFFFull, 0x3FF0000000000000ull};
    int bad = 0;
    /* [0] sentinel, [1] float at 4 mod 8, [2..3] double, [4..5] sentinel */
    uint32_t *sym = (uint32_t *) (host ? shmem_malloc (24) : shmemx_malloc_device (24));
    const uint32_t SENT = 0x5A5A5A5Au;
    for (unsigned k = 0; k < sizeof fp / sizeof fp[0]; ++k) {
        const uint32_t init[6] = {SENT, 0x11111111u, 0x22222222u, 0x33333333u, SENT, SENT};
        uint32_t now[6];
        copy (sym, init, sizeof init);
        shmem_barrier_all ();
        float *f = (float *) &sym[1];
        double *d = (double *) &sym[2];
        /* set, fetch back, swap in the next pattern and get this one back */
        shmem_float_set (f, f_of (fp[k]), right);
        bad += b_of_f (shmem_float_fetch (f, right)) != fp[k];
        bad += b_of_f (shmem_float_swap (f, f_of (fp[(k + 1) % 6]), right)) != fp[k];
        shmem_double_set (d, d_of (dp[k]), right);
        bad += b_of_d (shmem_double_fetch (d, right)) != dp[k];
        bad += b_of_d (shmem_double_swap (d, d_of (dp[(k + 1) % 6]), right)) != dp[k];
        shmem_barrier_all ();
        copy (now, sym, sizeof now);
        const uint64_t dn = dp[(k + 1) % 6];
        bad += now[0] != SENT || now[4] != SENT || now[5] != SENT;
        bad += now[1] != fp[(k + 1) % 6];
        bad += now[2] != (uint32_t) dn || now[3] != (uint32_t) (dn >> 32);
        shmem_barrier_all ();
    }
    printf ("PE %d of %d: %s\n", me, npes, bad ? "FAILED" : "PASS");
    shmem_barrier_all ();
    if (host)
        shmem_free (sym);
    else
        shmemx_free_device (sym);
    shmem_finalize ();
    return bad != 0;
}
