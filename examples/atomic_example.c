/*
 * atomic_example.c -- a ticket counter, a lock-protected update and a flag
 * with shmem_wait_until, from a plain OpenSHMEM program built against this
 * library:
 *
 *   gcc -std=c11 -Iinclude examples/atomic_example.c \
 *       -Losss-gasnet_amd/lib -lshmem_reduce -Wl,-rpath,$PWD/osss-gasnet_amd/lib -o atomic_example
 *   tools/oshrun -np 4 ./atomic_example            (device heap)
 *   tools/oshrun -np 4 ./atomic_example host       (shmem_malloc's host heap)
 *
 * 1. Tickets: every PE draws TICKETS numbers from a counter on PE 0 with
 *    shmem_int_finc; a PE's numbers increase, and the counter ends at
 *    PEs x TICKETS.
 * 2. Lock: every PE adds its number + 1 to a sum on the last PE ROUNDS times,
 *    read and written back with shmem_long_g / shmem_long_p under
 *    shmem_set_lock; the sum ends at ROUNDS x (1 + ... + PEs).
 * 3. Flag: a token goes round the ring. Every PE but 0 waits for its flag
 *    with shmem_long_wait_until, then puts the token it received + 1 into its
 *    right-hand neighbour and sets that neighbour's flag; PE 0 starts the
 *    ring and receives PEs back.
 */
#include <stdio.h>
#include <string.h>

#include <shmem.h>
#include <shmemx.h>

#define TICKETS 16
#define ROUNDS 8

static int host; /* the symmetric block is host memory: plain copies */

static void copy (void *dst, const void *src, size_t nbytes)
{
    if (host)
        memcpy (dst, src, nbytes);
    else
        shmemx_memcpy (dst, src, nbytes);
}

int main (int argc, char **argv)
{
    host = argc > 1 && strcmp (argv[1], "host") == 0;
    shmem_init ();
    const int me = shmem_my_pe (), npes = shmem_n_pes ();
    const int right = (me + 1) % npes, last = npes - 1;
    int bad = 0;

    /* one symmetric block: [0] counter (int), [1] lock, [2] sum, [3] flag, [4] token */
    long *sym = (long *) (host ? shmem_malloc (5 * sizeof (long)) : shmemx_malloc_device (5 * sizeof (long)));
    const long zeros[5] = {0, 0, 0, 0, 0};
    copy (sym, zeros, sizeof zeros);
    int *counter = (int *) &sym[0];
    long *lock = &sym[1], *sum = &sym[2], *flag = &sym[3], *token = &sym[4];
    shmem_barrier_all ();

    /* 1. tickets */
    int prev = -1;
    for (int i = 0; i < TICKETS; ++i) {
        const int t = shmem_int_finc (counter, 0);
        bad += t <= prev || t >= npes * TICKETS;
        prev = t;
    }
    shmem_barrier_all ();
    bad += shmem_int_fetch (counter, 0) != npes * TICKETS;

    /* 2. a read-modify-write that is only safe under the lock */
    for (int i = 0; i < ROUNDS; ++i) {
        shmem_set_lock (lock);
        shmem_long_p (sum, shmem_long_g (sum, last) + me + 1, last);
        shmem_clear_lock (lock);
    }
    shmem_barrier_all ();
    bad += shmem_long_g (sum, last) != (long) ROUNDS * npes * (npes + 1) / 2;

    /* 3. the ring */
    if (me != 0)
        shmem_long_wait_until (flag, SHMEM_CMP_EQ, 1);
    long mine = 0;
    copy (&mine, token, sizeof mine);
    bad += mine != me;
    shmem_long_p (token, mine + 1, right);
    shmem_fence (); /* the token before the flag */
    shmem_long_set (flag, 1, right);
    if (me == 0) {
        shmem_long_wait_until (flag, SHMEM_CMP_EQ, 1);
        copy (&mine, token, sizeof mine);
        bad += mine != npes;
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
