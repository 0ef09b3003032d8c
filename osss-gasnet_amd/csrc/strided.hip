// strided.hip -- the strided copy kernel of shmem_iput / shmem_iget and of
// shmem_alltoalls32/64 (gfx950).
//
// The reference runs a strided put or get as one network call per element
// (shmem_<T>_p / _g in a host loop, src/ptp/strided.c:110-238) and alltoalls
// as one shmem_iget per peer (src/alltoall/alltoall-linear.c). Here one launch
// moves up to 64 independent strided blocks (blockIdx.y = block):
//     dst[k * dst_stride] = src[k * src_stride]        k < nelems
// with elements of 1, 2, 4, 8 or 16 bytes and strides in elements (>= 1). The
// sources may be peers' mapped memory; every store goes to this GPU's (or this
// process's page-locked host) memory, the rule of coll.c's file header.
//
// Access pattern, per side, for elements of 1 to 8 bytes:
//   stride 1   16-byte vectors, after a head peeled so that side starts on a
//              128-byte line (as copy_segments peels its target)
//   stride > 1 consecutive lanes take consecutive elements, so one wave
//              instruction touches the fewest lines the stride allows
//              (64 * stride * size bytes); 1 / stride of every fetched line
//              is useful, up to one element per line
// One side contiguous and the other strided cannot have both from registers
// alone (a lane's 16-byte vector holds V = 16, 8, 4 or 2 CONSECUTIVE elements,
// the lane-consecutive accesses hold elements 256 apart), so a block turns its
// tile of 256 * V elements through 4 KiB of LDS: written one way, read the
// other, between two block barriers. The loads of the next tile are issued
// before the stores of this one. Both sides contiguous is the copy kernel
// (mi355_copy_segments); both strided needs no LDS.
//
// The tile is addressed in ELEMENTS on the lane-consecutive side (element
// j * 256 + tid, a byte, short, dword or qword access) and in 16-byte vectors
// on the other (vector tid = elements tid * V ... tid * V + V - 1), so the two
// views agree for every sizeof(T) dividing 16. With 1- and 2-byte elements the
// element-side LDS accesses are sub-dword: the 4 (2) lanes whose elements
// share a dword hit one bank, 32 lanes cover 8 (16) banks. That is within
// what ds_write_b32's issue already costs (MI355X: a 4-way store conflict
// doubles a 4-cycle instruction). Measured (strided
// put/get): the forms that store with a stride take the same time from 8-byte
// elements down to 1-byte ones, bound by partially written lines; the 1-byte
// gathers are 40-45 % behind the 4-byte ones, bound by their V = 16 one-byte
// global loads per lane and tile, which packing in registers would not remove.
//
// A 16-byte element is a vector already: no LDS and no tile, every lane moves
// one element per slot on both sides (the "both" form with T = u32x4),
// whatever the strides.
//
// Every offset is 64-bit: nelems * stride * size passes 4 GiB easily.
// Grid-stride over a capped grid; the tile loop's trip count is uniform per
// block (the barriers). Strided stores are plain stores, so the completion
// signal writes the L2 back first (signal_done's plain_stores).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "combine_kernels.h"
#include "mi355_reduce.h"

namespace mi355k {

constexpr int kStridedMaxSeg = 64;

template <int NS>
struct StridedParams {
    void *dst[NS];
    const void *src[NS];
    int64_t dst_stride, src_stride;  // elements
    uint64_t n;                      // elements per block
    Signal sig;
};

// Elements before the first 128-byte line of p (at most n).
template <typename T>
__device__ __forceinline__ uint64_t line_head(const void *p, uint64_t n) {
    const uint64_t h = ((128u - (unsigned)((uintptr_t)p & 127)) & 127u) / sizeof(T);
    return h < n ? h : n;
}

enum { STRIDED_GATHER = 0, STRIDED_SCATTER = 1, STRIDED_BOTH = 2 };

// The elements outside the vector part, [0, head) and [vend, n): element-wise over the whole grid row.
template <typename T>
__device__ __forceinline__ bool strided_rest(T *dst, const T *src, int64_t ds, int64_t ss, uint64_t head,
                                             uint64_t vend, uint64_t n) {
    bool any = false;
    const uint64_t nrest = head + (n - vend);
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < nrest; r += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = r < head ? r : vend + (r - head);
        dst[(int64_t)i * ds] = src[(int64_t)i * ss];
        any = true;
    }
    return any;
}

template <typename T, int MODE, int NS>
__global__ __launch_bounds__(kBlock) void strided_pull(StridedParams<NS> p) {
    constexpr int V = 16 / sizeof(T);          // elements per 16-byte vector
    constexpr uint64_t kTile = (uint64_t)kBlock * V;  // elements per block pass
    const int sg = blockIdx.y;
    T *dst = (T *)p.dst[sg];
    const T *src = (const T *)p.src[sg];
    const uint64_t n = p.n;
    const int64_t ds = p.dst_stride, ss = p.src_stride;
    const unsigned tid = threadIdx.x;
    bool plain = false;

    if constexpr (MODE == STRIDED_BOTH) {
        constexpr int U = 4;
        const uint64_t step = (uint64_t)gridDim.x * kBlock * U;
        for (uint64_t base = (uint64_t)blockIdx.x * kBlock * U + tid; base < n; base += step) {
            T x[U] = {};
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t i = base + (uint64_t)u * kBlock;
                if (i < n) x[u] = src[(int64_t)i * ss];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t i = base + (uint64_t)u * kBlock;
                if (i < n) dst[(int64_t)i * ds] = x[u];
            }
        }
        plain = n > 0;
    } else {
        __shared__ u32x4 lds_v[kBlock];  // one tile: 256 * V elements = 4 KiB
        T *lds = (T *)lds_v;
        // the contiguous side, peeled to its line
        const uint64_t head = line_head<T>(MODE == STRIDED_GATHER ? (const void *)dst : (const void *)src, n);
        const uint64_t nvec = (n - head) / V;
        const uint64_t vend = head + nvec * V;
        const uint64_t ntiles = (nvec + kBlock - 1) / kBlock;
        if constexpr (MODE == STRIDED_GATHER) {
            // strided loads, lane-consecutive -> LDS -> one 16-byte store per lane
            u32x4 *dv = (u32x4 *)(dst + head);
            T x[V] = {};
            uint64_t t = blockIdx.x;
            if (t < ntiles) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const uint64_t i = head + t * kTile + (uint64_t)j * kBlock + tid;
                    if (i < vend) x[j] = src[(int64_t)i * ss];
                }
            }
            for (; t < ntiles; t += gridDim.x) {
#pragma unroll
                for (int j = 0; j < V; ++j) lds[j * kBlock + tid] = x[j];
                __syncthreads();
                const uint64_t tn = t + gridDim.x;
                if (tn < ntiles) {
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const uint64_t i = head + tn * kTile + (uint64_t)j * kBlock + tid;
                        if (i < vend) x[j] = src[(int64_t)i * ss];
                    }
                }
                const uint64_t v = t * kBlock + tid;
                if (v < nvec) st16(dv + v, lds_v[tid]);
                __syncthreads();
            }
        } else {
            // one 16-byte load per lane -> LDS -> strided stores, lane-consecutive
            const u32x4 *sv = (const u32x4 *)(src + head);
            u32x4 x = {0, 0, 0, 0};
            uint64_t t = blockIdx.x;
            if (t * kBlock + tid < nvec) x = ld16<POL_PLAIN>(sv + t * kBlock + tid);
            for (; t < ntiles; t += gridDim.x) {
                lds_v[tid] = x;
                __syncthreads();
                const uint64_t tn = t + gridDim.x;
                if (tn * kBlock + tid < nvec) x = ld16<POL_PLAIN>(sv + tn * kBlock + tid);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const uint64_t i = head + t * kTile + (uint64_t)j * kBlock + tid;
                    if (i < vend) dst[(int64_t)i * ds] = lds[j * kBlock + tid];
                }
                __syncthreads();
            }
            plain = nvec > 0;
        }
        plain |= strided_rest<T>(dst, src, ds, ss, head, vend, n);
    }
    signal_done(p.sig, __syncthreads_or(plain));
}

template <typename T, int MODE>
static int strided_launch(const StridedParams<kStridedMaxSeg> &p, int used, hipStream_t st) {
    constexpr int V = 16 / sizeof(T);  // 1 for a 16-byte element (no tile: STRIDED_BOTH only)
    // a few resident blocks per CU: the strided side is latency-bound (one
    // element per lane per load), more waves keep more lines in flight
    constexpr int kPerCU = 8;
    unsigned gx = grid_for((uint64_t)kBlock * (MODE == STRIDED_BOTH ? 4 : V), p.n, kPerCU);
    const unsigned cap = (unsigned)device_cus() * kPerCU;
    if ((uint64_t)gx * used > cap) gx = cap / used > 0 ? cap / used : 1;
    if (used == 1) {
        StridedParams<1> p1{};
        p1.dst[0] = p.dst[0];
        p1.src[0] = p.src[0];
        p1.dst_stride = p.dst_stride;
        p1.src_stride = p.src_stride;
        p1.n = p.n;
        return launch(strided_pull<T, MODE, 1>, dim3(gx, 1), st, p1);
    }
    return launch(strided_pull<T, MODE, kStridedMaxSeg>, dim3(gx, used), st, p);
}

template <typename T>
static int strided_mode(const StridedParams<kStridedMaxSeg> &p, int used, hipStream_t st) {
    if (p.dst_stride == 1) return strided_launch<T, STRIDED_GATHER>(p, used, st);
    if (p.src_stride == 1) return strided_launch<T, STRIDED_SCATTER>(p, used, st);
    return strided_launch<T, STRIDED_BOTH>(p, used, st);
}

}  // namespace mi355k

using namespace mi355k;

static int strided_copy_impl(int elem_size, void *const *dsts, const void *const *srcs, ptrdiff_t dst_stride,
                             ptrdiff_t src_stride, size_t nelems, int nseg, void *stream) {
    if ((elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8 && elem_size != 16) || dst_stride < 1 ||
        src_stride < 1 || nseg < 0 || nseg > kStridedMaxSeg)
        return MI355_E_INVAL;
    if (nseg > 0 && (dsts == nullptr || srcs == nullptr)) return MI355_E_INVAL;
    if (dst_stride == 1 && src_stride == 1) {
        // both sides contiguous: the copy kernel
        size_t nb[kStridedMaxSeg];
        for (int k = 0; k < nseg; ++k) nb[k] = nelems * (size_t)elem_size;
        return mi355_copy_segments(dsts, srcs, nb, nseg, stream);
    }
    StridedParams<kStridedMaxSeg> p{};
    int used = 0;
    for (int k = 0; k < nseg && nelems != 0; ++k) {
        if (dsts[k] == nullptr || srcs[k] == nullptr) return MI355_E_INVAL;
        if ((((uintptr_t)dsts[k] | (uintptr_t)srcs[k]) & (uintptr_t)(elem_size - 1)) != 0)
            return MI355_E_INVAL;  // elements are read and written whole
        p.dst[used] = dsts[k];
        p.src[used] = srcs[k];
        ++used;
    }
    if (used == 0) {
        fire_on_host((hipStream_t)stream);
        return 0;
    }
    p.dst_stride = dst_stride;
    p.src_stride = src_stride;
    p.n = nelems;
    hipStream_t st = (hipStream_t)stream;
    switch (elem_size) {
        case 1: return strided_mode<uint8_t>(p, used, st);
        case 2: return strided_mode<uint16_t>(p, used, st);
        case 4: return strided_mode<uint32_t>(p, used, st);
        case 8: return strided_mode<uint64_t>(p, used, st);
        default: return strided_launch<u32x4, STRIDED_BOTH>(p, used, st);  // an element is a vector
    }
}

extern "C" int mi355_strided_copy(int elem_size, void *const *dsts, const void *const *srcs, ptrdiff_t dst_stride,
                                  ptrdiff_t src_stride, size_t nelems, int nseg, void *stream) {
    return t_launch.end_call(strided_copy_impl(elem_size, dsts, srcs, dst_stride, src_stride, nelems, nseg, stream));
}

// The all-to-all's front: 4- and 8-byte elements only, the same launches.
extern "C" int mi355_strided_pull(int elem_size, void *const *dsts, const void *const *srcs, ptrdiff_t dst_stride,
                                  ptrdiff_t src_stride, size_t nelems, int nseg, void *stream) {
    if (elem_size != 4 && elem_size != 8) return t_launch.end_call(MI355_E_INVAL);
    return mi355_strided_copy(elem_size, dsts, srcs, dst_stride, src_stride, nelems, nseg, stream);
}
