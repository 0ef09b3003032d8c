/* A caller of shmem_alltoalls64_ the way gfortran calls it: every argument by
 * reference, an INTEGER pSync (tests/test_gpu_alltoall.py, 2 PEs). The data
 * lives in the symmetric host heap; elements land 2 apart and are read 3
 * apart. */
#include <stddef.h>
#include <stdio.h>

#include <shmem.h>
#include <shmem_fortran.h>

#define N 100

int main (void)
{
    static int psync[2 * SHMEM_ALLTOALLS_SYNC_SIZE];
    for (int i = 0; i < (int) (2 * SHMEM_ALLTOALLS_SYNC_SIZE); ++i)
        psync[i] = -1;
    shmem_init_ ();
    const int me = shmem_my_pe_ (), npes = shmem_n_pes_ ();
    long *src = (long *) shmem_malloc ((size_t) npes * N * 3 * sizeof (long));
    long *dst = (long *) shmem_malloc ((size_t) npes * N * 2 * sizeof (long));
    for (int j = 0; j < npes * N * 3; ++j)
        src[j] = 1000003L * me + j;
    for (int j = 0; j < npes * N * 2; ++j)
        dst[j] = -7;
    shmem_barrier_all_ ();
    ptrdiff_t dstride = 2, sstride = 3;
    int nelems = N, start = 0, logstride = 0, size = npes;
    shmem_alltoalls64_ (dst, src, &dstride, &sstride, &nelems, &start, &logstride, &size, psync);
    int bad = 0;
    for (int i = 0; i < npes; ++i)
        for (int k = 0; k < N; ++k) {
            bad += dst[(i * N + k) * 2] != 1000003L * i + (long) (me * N + k) * 3;
            bad += dst[(i * N + k) * 2 + 1] != -7;
        }
    for (int i = 0; i < (int) (2 * SHMEM_ALLTOALLS_SYNC_SIZE); ++i)
        bad += psync[i] != -1;
    printf ("PE %d of %d: %s\n", me, npes, bad ? "FAILED" : "PASS");
    shmem_free (dst);
    shmem_free (src);
    shmem_finalize_ ();
    return bad != 0;
}
