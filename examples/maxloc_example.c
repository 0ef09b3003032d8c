/*
 * maxloc_example.c -- an argmax over vocabulary shards with
 * shmemx_float_maxloc_to_all, from a plain OpenSHMEM program built against
 * this library:
 *
 *   gcc -std=c99 -Iinclude examples/maxloc_example.c \
 *       -Losss-gasnet_amd/lib -lshmem_reduce -Wl,-rpath,$PWD/osss-gasnet_amd/lib -o maxloc_example
 *   tools/oshrun -np 2 ./maxloc_example
 *
 * Greedy decoding with the vocabulary sharded over the PEs: for each of BATCH
 * sequences every PE holds the logits of its SHARD vocabulary entries. Each PE
 * first reduces its shard to one candidate per sequence -- its best logit and
 * that entry's GLOBAL vocabulary index -- and one maxloc over the PEs then
 * gives every PE the winning logit and token of every sequence. Ties go to
 * the smaller index, a NaN logit wins and reports its index (as torch.max
 * does). Checked against a host loop over the whole vocabulary.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <shmem.h>
#include <shmemx.h>

#define BATCH 1000
#define SHARD 64

/* the logit of vocabulary entry v for sequence b: plenty of ties */
static float logit (int b, long v) { return (float) ((b * 31 + v * 17) % 97) * 0.25f - 3.0f; }

int main (void)
{
    shmem_init ();
    const int me = shmem_my_pe (), npes = shmem_n_pes ();
    const long vocab = (long) SHARD * npes;

    float *best = (float *) shmemx_malloc_device (BATCH * sizeof *best);
    long *best_idx = (long *) shmemx_malloc_device (BATCH * sizeof *best_idx);
    float *top = (float *) shmemx_malloc_device (BATCH * sizeof *top);
    long *token = (long *) shmemx_malloc_device (BATCH * sizeof *token);
    float *hv = (float *) malloc (BATCH * sizeof *hv);
    long *hl = (long *) malloc (BATCH * sizeof *hl);

    /* the local part: this PE's shard, entries me * SHARD .. (me + 1) * SHARD - 1 */
    for (int b = 0; b < BATCH; ++b) {
        hv[b] = logit (b, (long) me * SHARD);
        hl[b] = (long) me * SHARD;
        for (long v = (long) me * SHARD + 1; v < (long) (me + 1) * SHARD; ++v)
            if (logit (b, v) > hv[b]) {
                hv[b] = logit (b, v);
                hl[b] = v;
            }
    }
    shmemx_memcpy (best, hv, BATCH * sizeof *best);
    shmemx_memcpy (best_idx, hl, BATCH * sizeof *best_idx);
    shmem_barrier_all ();

    shmemx_float_maxloc_to_all (top, token, best, best_idx, BATCH, 0, 0, npes);

    shmemx_memcpy (hv, top, BATCH * sizeof *top);
    shmemx_memcpy (hl, token, BATCH * sizeof *token);
    int bad = 0;
    for (int b = 0; b < BATCH; ++b) {
        float w = logit (b, 0);
        long wi = 0;
        for (long v = 1; v < vocab; ++v)
            if (logit (b, v) > w) {
                w = logit (b, v);
                wi = v;
            }
        bad += memcmp (&hv[b], &w, sizeof w) != 0 || hl[b] != wi;
    }

    printf ("PE %d of %d: %s\n", me, npes, bad ? "FAILED" : "OK");
    shmem_barrier_all ();
    free (hl);
    free (hv);
    shmemx_free_device (token);
    shmemx_free_device (top);
    shmemx_free_device (best_idx);
    shmemx_free_device (best);
    shmem_finalize ();
    return bad != 0;
}
