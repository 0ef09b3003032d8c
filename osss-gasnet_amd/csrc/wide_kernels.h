// wide_kernels.h -- the widening fold's kernels (wide.hip has the C ABI and
// the design notes): the widen / narrow conversions, the two vector
// forms and the element-per-lane form, and the launcher that turns
// wide_plan.h's plan into a kernel and a grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "combine_kernels.h"
#include "wide_plan.h"

namespace mi355k {

static_assert(MI355_WIDE_BLOCK == kBlock, "wide_plan.h counts in blocks of kBlock threads");
static_assert(MI355_WIDE_MAX_SOURCES == MI355_ORDERS_MAX_SOURCES, "one call's sources");
static_assert(MI355_WIDE_BLOCKS_PER_CU <= kBlocksPerCU, "the streaming cap");

// Elements of one lane's unit: a 16-byte load of 8 for the 16-bit output; for
// the float output an 8-byte load of 4, whose results are one 16-byte store
// (wide_plan.h, MI355_WIDE_PER_LANE_FLOAT).
template <bool FLOAT_OUT> constexpr int kWidePerLane = FLOAT_OUT ? MI355_WIDE_PER_LANE_FLOAT : MI355_WIDE_PER_LANE;
// sources whose loads a lane issues before it adds the first of them: 128
// bytes in flight per lane in either shape
template <bool FLOAT_OUT> constexpr int kWideBatch = 64 / kWidePerLane<FLOAT_OUT>;

struct WideParams {
    void *dst;
    const void *src[MI355_WIDE_MAX_SOURCES];
    uint64_t nvec;  // vector kernels: whole units of 8 (float output: 4) elements; element kernel: elements
    uint32_t tail;  // vector kernels: elements after the last whole unit
    int nsrc;
    Signal sig;
};

// 16 bits -> the binary32 value they denote, exact: v_cvt_f32_f16 (subnormals
// kept), and a shift for bfloat16
template <typename T>
__device__ __forceinline__ float wide_in(uint16_t b) {
    return F16Traits<T>::widen(T{b});
}

// The one rounding, to nearest even: v_cvt_f16_f32 / v_cvt_pk_bf16_f32
// (subnormals kept, overflow to +-inf); a NaN is the type's canonical one.
template <typename T>
__device__ __forceinline__ uint16_t wide_narrow(float a) {
    uint16_t r;
    if constexpr (std::is_same<T, f16>::value) r = __builtin_bit_cast(uint16_t, (_Float16)a);
    else r = __builtin_bit_cast(uint16_t, (__bf16)a);
    return a != a ? F16Traits<T>::canonical_nan : r;
}

// The binary32 sum as it is; a NaN is 0x7FC00000.
__device__ __forceinline__ uint32_t wide_float_bits(float a) {
    return a != a ? 0x7FC00000u : __builtin_bit_cast(uint32_t, a);
}

// One element: every source's value at index i, then the store -- so the
// 16-bit output may be one of the sources (every load of a position precedes
// its store, and no other lane touches it).
template <typename T, bool FLOAT_OUT>
__device__ __forceinline__ void wide_fold_element(const WideParams &p, uint64_t i) {
    float acc = wide_in<T>(((const uint16_t *)p.src[0])[i]);
    for (int j = 1; j < p.nsrc; ++j) acc = acc + wide_in<T>(((const uint16_t *)p.src[j])[i]);
    if constexpr (FLOAT_OUT) ((uint32_t *)p.dst)[i] = wide_float_bits(acc);
    else ((uint16_t *)p.dst)[i] = wide_narrow<T>(acc);
}

// One lane's unit of source elements: 16 bytes (8 elements) or 8 bytes (4),
// loaded non-temporally from an aligned or (UNALIGNED) any 2-byte-aligned
// address; gfx950 runs in unaligned access mode (combine_kernels.h, ld16_src).
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2_any __attribute__((ext_vector_type(2), aligned(1)));
template <int V> struct WideUnit;
template <> struct WideUnit<8> {
    union {
        u32x4 v;
        uint16_t e[8];
    };
    template <bool UNALIGNED>
    __device__ __forceinline__ void load(const void *s, uint64_t i) {
        v = ld16_src<POL_NT_LOAD, UNALIGNED>((const u32x4 *)s, i);
    }
};
template <> struct WideUnit<4> {
    union {
        u32x2 v;
        uint16_t e[4];
    };
    template <bool UNALIGNED>
    __device__ __forceinline__ void load(const void *s, uint64_t i) {
        if constexpr (UNALIGNED) v = __builtin_nontemporal_load((const u32x2_any *)s + i);
        else v = __builtin_nontemporal_load((const u32x2 *)s + i);
    }
};

// The vector forms: the target 16-byte aligned, the sources aligned to their
// unit or (UNALIGNED) read with unaligned loads. A grid-stride loop over the
// whole units; a unit's running sums stay in VGPRs as binary32 while the
// sources pass by in ascending order, looped over at run time from the pointer
// table in the kernel arguments, a batch of loads issued before its first add.
// Either output is ONE 16-byte store per lane, lane i at base + 16 i, so a
// wave's store instruction writes 1 KiB contiguous: 8 elements per lane for
// the 16-bit output (a 16-byte load per source), 4 for the float output (an
// 8-byte load per source). The other float shape -- 8 elements per lane as two
// 16-byte stores 32 bytes from the next lane's -- ran at half the rate at 2
// sources (DESIGN.md section 6 "Wide sum" has both). Stores are
// write-through (st16_fold), as the folds', so the completion signal needs no
// write-back; block 0, whose first lanes fold the tail elements with plain
// stores, releases first.
template <typename T, bool FLOAT_OUT, bool UNALIGNED>
__device__ __forceinline__ void wide_fold_vectors(const WideParams &p) {
    constexpr int V = kWidePerLane<FLOAT_OUT>;
    constexpr int B = kWideBatch<FLOAT_OUT>;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const int nsrc = p.nsrc;
    for (uint64_t i = g; i < p.nvec; i += step) {
        float acc[V] = {};
        for (int j0 = 0; j0 < nsrc; j0 += B) {
            WideUnit<V> x[B];
#pragma unroll
            for (int k = 0; k < B; ++k)
                if (j0 + k < nsrc) x[k].template load<UNALIGNED>(p.src[j0 + k], i);
            __builtin_amdgcn_sched_barrier(0);  // loads first (fold_vectors)
#pragma unroll
            for (int k = 0; k < B; ++k) {
                if (j0 + k < nsrc) {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const float w = wide_in<T>(x[k].e[e]);
                        // source 0 starts the sum (0 + -0 would lose the sign)
                        acc[e] = k == 0 && j0 == 0 ? w : acc[e] + w;
                    }
                }
            }
        }
        if constexpr (FLOAT_OUT) {
            Pack<uint32_t> o;
#pragma unroll
            for (int e = 0; e < V; ++e) o.e[e] = wide_float_bits(acc[e]);
            st16_fold((u32x4 *)p.dst + i, o.v);
        } else {
            Pack<uint16_t> o;
#pragma unroll
            for (int e = 0; e < V; ++e) o.e[e] = wide_narrow<T>(acc[e]);
            st16_fold((u32x4 *)p.dst + i, o.v);
        }
    }
    if (g < p.tail) wide_fold_element<T, FLOAT_OUT>(p, p.nvec * V + g);
    signal_done(p.sig, blockIdx.x == 0 && p.tail != 0);
}

template <typename T, bool FLOAT_OUT>
__global__ __launch_bounds__(kBlock) void wide_fold_vec(WideParams p) {
    wide_fold_vectors<T, FLOAT_OUT, false>(p);
}

template <typename T, bool FLOAT_OUT>
__global__ __launch_bounds__(kBlock) void wide_fold_unal(WideParams p) {
    wide_fold_vectors<T, FLOAT_OUT, true>(p);
}

// The element form: any element-aligned pointers, one element per lane and
// pass; consecutive lanes take consecutive elements.
template <typename T, bool FLOAT_OUT>
__global__ __launch_bounds__(kBlock) void wide_fold_elem(WideParams p) {
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < p.nvec; i += step)
        wide_fold_element<T, FLOAT_OUT>(p, i);
    signal_done(p.sig, true);
}

template <typename T, bool FLOAT_OUT>
int wide_launch(WideParams &p, const mi355_wide_plan &plan, hipStream_t st) {
    p.nvec = plan.nvec;
    p.tail = plan.tail;
    if (plan.form == MI355_WIDE_VECTOR) return launch(wide_fold_vec<T, FLOAT_OUT>, dim3(plan.grid), st, p);
    if (plan.form == MI355_WIDE_UNALIGNED) return launch(wide_fold_unal<T, FLOAT_OUT>, dim3(plan.grid), st, p);
    return launch(wide_fold_elem<T, FLOAT_OUT>, dim3(plan.grid), st, p);
}

}  // namespace mi355k
