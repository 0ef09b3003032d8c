// loc_kernels.h -- the value-and-location fold's kernels (loc.hip has the C
// ABI and the design notes): the comparison rule, the 16-byte vector form and
// the element-per-lane form, and the launcher that turns loc_plan.h's plan
// into a kernel and a grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "combine_kernels.h"
#include "loc_plan.h"

namespace mi355k {

static_assert(MI355_LOC_BLOCK == kBlock, "loc_plan.h counts in blocks of kBlock threads");
static_assert(MI355_LOC_MAX_SOURCES == MI355_ORDERS_MAX_SOURCES, "one call's sources");
static_assert(MI355_LOC_BLOCKS_PER_CU == kBlocksPerCU, "the streaming cap");

struct LocParams {
    void *dst_val;
    long long *dst_loc;
    const void *src_val[MI355_LOC_MAX_SOURCES];
    const long long *src_loc[MI355_LOC_MAX_SOURCES];  // nullptr: source j's location is loc_base + j
    long long loc_base;
    uint64_t nvec;  // vector kernel: whole 16-byte value vectors; element kernel: elements
    uint32_t tail;  // vector kernel: elements after nvec * V (< V)
    int nsrc;
    Signal sig;
};

// The values travel as their bit patterns: the winner's bits are stored as
// they were loaded (NaN payload, zero sign, 16-bit pattern), and only the
// comparison looks at what they denote.
template <typename T> struct LocBits { using type = T; };
template <> struct LocBits<float> { using type = uint32_t; };
template <> struct LocBits<double> { using type = uint64_t; };
template <> struct LocBits<f16> { using type = uint16_t; };
template <> struct LocBits<bf16> { using type = uint16_t; };

template <typename T>
__device__ __forceinline__ auto loc_value(typename LocBits<T>::type b) {
    if constexpr (std::is_same<T, f16>::value || std::is_same<T, bf16>::value)
        return F16Traits<T>::widen(T{b});  // exact
    else
        return __builtin_bit_cast(T, b);
}

// b beats a (shmemx.h, "Value and location"): a NaN beats every number, in
// both operators; between two NaNs, and between two equal numbers (-0 == +0),
// the smaller location; else the larger (max) or smaller (min) value. Equal in
// both: false, the earlier source stays.
template <int OP, typename T>
__device__ __forceinline__ bool loc_beats(typename LocBits<T>::type bb, long long lb, typename LocBits<T>::type ab,
                                          long long la) {
    const auto b = loc_value<T>(bb), a = loc_value<T>(ab);
    const bool better = OP == MI355_OP_MAX ? b > a : b < a;
    const bool number = better || (b == a && lb < la);  // false when either is a NaN
    if constexpr (std::is_integral<T>::value) {
        return number;
    } else {
        const bool nb = b != b, na = a != a;
        return nb ? (!na || lb < la) : number;
    }
}

// One element: every source's pair at index i, then the store -- so the
// output may be one of the sources (every load of a position precedes its
// store, and no other lane touches it).
template <int OP, typename T>
__device__ __forceinline__ void loc_fold_element(const LocParams &p, uint64_t i) {
    using B = typename LocBits<T>::type;
    B wv = ((const B *)p.src_val[0])[i];
    long long wl = p.src_loc[0] != nullptr ? p.src_loc[0][i] : p.loc_base;
    for (int j = 1; j < p.nsrc; ++j) {
        const B cv = ((const B *)p.src_val[j])[i];
        const long long *lp = p.src_loc[j];
        const long long cl = lp != nullptr ? lp[i] : p.loc_base + j;
        const bool take = loc_beats<OP, T>(cv, cl, wv, wl);
        wv = take ? cv : wv;
        wl = take ? cl : wl;
    }
    ((B *)p.dst_val)[i] = wv;
    p.dst_loc[i] = wl;
}

// Source j's vector i: V values in one 16-byte load, their V locations in
// V / 2 more (or none: the implicit location is the same for every element).
template <typename B, int V>
__device__ __forceinline__ void loc_load_vector(const LocParams &p, int j, uint64_t i, Pack<B> &v, long long (&l)[V]) {
    v.v = __builtin_nontemporal_load((const u32x4 *)p.src_val[j] + i);
    const long long *lp = p.src_loc[j];
    if (lp != nullptr) {
        const u32x4 *q = (const u32x4 *)lp + i * (V / 2);
#pragma unroll
        for (int k = 0; k < V / 2; ++k) {
            Pack<long long> t;
            t.v = __builtin_nontemporal_load(q + k);
            l[2 * k] = t.e[0];
            l[2 * k + 1] = t.e[1];
        }
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) l[e] = p.loc_base + j;
    }
}

// The vector form: every pointer 16-byte aligned. A grid-stride loop over
// the whole vectors; the running winner of a vector's V elements stays in
// registers (V values in 4 VGPRs, V locations in 2 V) while the sources pass
// by, looped over at run time from the pointer table in the kernel arguments.
// Stores are write-through (st16_fold), as the folds', so the completion
// signal needs no write-back; block 0, whose first lanes fold the tail
// elements with plain stores, releases first.
template <int OP, typename T>
__global__ __launch_bounds__(kBlock) void loc_fold_vec(LocParams p) {
    using B = typename LocBits<T>::type;
    constexpr int V = 16 / sizeof(T);
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const int nsrc = p.nsrc;
    for (uint64_t i = g; i < p.nvec; i += step) {
        Pack<B> wv;
        long long wl[V];
        loc_load_vector<B, V>(p, 0, i, wv, wl);
        for (int j = 1; j < nsrc; ++j) {
            Pack<B> cv;
            long long cl[V];
            loc_load_vector<B, V>(p, j, i, cv, cl);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const bool take = loc_beats<OP, T>(cv.e[e], cl[e], wv.e[e], wl[e]);
                wv.e[e] = take ? cv.e[e] : wv.e[e];
                wl[e] = take ? cl[e] : wl[e];
            }
        }
        st16_fold((u32x4 *)p.dst_val + i, wv.v);
        u32x4 *q = (u32x4 *)p.dst_loc + i * (V / 2);
#pragma unroll
        for (int k = 0; k < V / 2; ++k) {
            Pack<long long> t;
            t.e[0] = wl[2 * k];
            t.e[1] = wl[2 * k + 1];
            st16_fold(q + k, t.v);
        }
    }
    if (g < p.tail) loc_fold_element<OP, T>(p, p.nvec * V + g);
    signal_done(p.sig, blockIdx.x == 0 && p.tail != 0);
}

// The element form: any element-aligned pointers, one element per lane and
// pass; consecutive lanes take consecutive elements.
template <int OP, typename T>
__global__ __launch_bounds__(kBlock) void loc_fold_elem(LocParams p) {
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < p.nvec; i += step) loc_fold_element<OP, T>(p, i);
    signal_done(p.sig, true);
}

template <int OP, typename T>
int loc_launch(LocParams &p, const mi355_loc_plan &plan, hipStream_t st) {
    p.nvec = plan.nvec;
    p.tail = plan.tail;
    if (plan.form == MI355_LOC_VECTOR) return launch(loc_fold_vec<OP, T>, dim3(plan.grid), st, p);
    return launch(loc_fold_elem<OP, T>, dim3(plan.grid), st, p);
}

}  // namespace mi355k
