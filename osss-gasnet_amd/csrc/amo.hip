// amo.hip -- remote atomics on the symmetric device heap (gfx950): the
// single-operation kernel behind shmem_<T>_swap / cswap / fadd / finc / add /
// inc / fetch / set (and, through its FETCH, behind shmem_wait_until on a
// device-heap word), and the atomic accumulate of shmemx_<T>_atomic_add_v.
//
// The reference runs every atomic as an active message to the target PE
// (src/atomic/atomic.c -> shmemi_comms_*_request), whose handler takes a lock
// and updates the word. Here the target PE's heap is mapped into this
// process (runtime.c peer_heap), so the initiating PE's GPU performs the
// operation itself with a system-scope atomic on the mapped address: gfx950
// executes global atomics at the memory side (MI355X_MICROARCH.md, "Global
// float atomics"), where the operations of every XCD and every process on
// the device meet. The target PE takes no part.
//
// No kernel in this file spins or waits on another process: each runs to
// completion on its own. Waiting (shmem_wait_until, shmem_set_lock) is a host
// loop around single FETCH / CSWAP launches (amo.c).
//
// Single operation: one wave, one lane. Every op is a read-modify-write so
// that all of them meet at the same place and are mutually atomic: SET is an
// exchange whose result is dropped, FETCH an add of 0. A plain store or load,
// even a write-through one, is served by the issuing XCD's L2 and would not
// be ordered against the other XCDs' memory-side operations. The operands
// are unsigned integers of the width: wrap-around is defined, and the float
// and double forms of swap / fetch / set move bit patterns (the library casts
// them), NaN payloads and -0.0 included. The old value is stored to a
// host-coherent slot before the completion signal, by the same lane.
//
// Accumulate: a grid-stride loop; slot u of lane t in block b takes element
// base + u * 256 + t, so that every wave-instruction, source load or atomic,
// covers 64 consecutive elements -- 256 contiguous bytes of dwords, 512 of
// qwords, the shape the guide measured at the chip's memory-side atomic rate
// -- whatever the two pointers' phases (element alignment is all that is
// assumed; there is no vector access to peel for). The 4 source loads of a
// lane are issued before its first atomic. The atomics return nothing (the
// wave does not wait for them) and are relaxed: the kernel's end orders them
// for whoever learns of it.
//
// Float and double adds compile to global_atomic_add_f32 / _f64, not to a
// compare-and-swap loop (this translation unit alone is built with
// -munsafe-fp-atomics: the heaps are ordinary device memory, hipMalloc'd,
// where the hardware instruction is valid; the Makefile's rule says the
// same). The memory-side add is one correctly rounded IEEE add, as the CAS
// loop's v_add would be and as the host heap's SSE add is: nearest-even with
// ties to the even neighbour, subnormal operands and results kept (MODE.denorm
// does not reach it, and nothing is flushed), max + half an ulp to Inf,
// -0 + -0 = -0 and x + (-x) = +0. Measured, not assumed:
// tests/test_gpu_atomic.py::test_accumulate_kernel_float_semantics runs the
// operand table of tests/_fp_add_cases.py through atomic_add_v<float> and
// <double> and compares every non-NaN row with an exact model in every bit.
// Where the result is a NaN, that it is a NaN is all that is promised: which
// sign, payload and quiet bit the atomic unit returns is not specified.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "amo_plan.h"
#include "combine_kernels.h"
#include "mi355_reduce.h"

namespace mi355k {

static_assert(kAddvBlock == kBlock, "amo_plan.h counts in blocks of kBlock threads");

struct AmoParams {
    void *target;
    unsigned long long value, cond;
    unsigned long long *slot;
    int op;
    Signal sig;
};

template <typename U>
__global__ __launch_bounds__(64) void amo_one(AmoParams p) {
    if (threadIdx.x == 0) {
        U *t = (U *)p.target;
        const U v = (U)p.value;
        U old = 0;
        switch (p.op) {
            case MI355_AMO_SWAP:
            case MI355_AMO_SET:
                old = __hip_atomic_exchange(t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            case MI355_AMO_CSWAP: {
                U expected = (U)p.cond;
                __hip_atomic_compare_exchange_strong(t, &expected, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_SYSTEM);
                old = expected;
                break;
            }
            case MI355_AMO_FADD:
                old = __hip_atomic_fetch_add(t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            default:  // MI355_AMO_FETCH
                old = __hip_atomic_fetch_add(t, (U)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
        }
        if (p.slot != nullptr)
            __hip_atomic_store(p.slot, p.op == MI355_AMO_SET ? 0ull : (unsigned long long)old, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // waits for this lane's atomic and slot store (vmcnt(0)) before the flag
    signal_done(p.sig, false);
}

struct AddvParams {
    void *target;
    const void *source;
    uint64_t n;
    Signal sig;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void atomic_add_v(AddvParams p) {
    constexpr int U = kAddvUnroll;
    T *dst = (T *)p.target;
    const T *src = (const T *)p.source;
    const uint64_t n = p.n;
    const uint64_t step = (uint64_t)gridDim.x * kBlock * U;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock * U + threadIdx.x; base < n; base += step) {
        T x[U] = {};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = base + (uint64_t)u * kBlock;
            if (i < n) x[u] = __builtin_nontemporal_load(src + i);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = base + (uint64_t)u * kBlock;
            if (i < n) (void)__hip_atomic_fetch_add(dst + i, x[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    signal_done(p.sig, false);
}

template <typename T>
static int addv_launch(void *target, const void *source, size_t n, hipStream_t st) {
    if ((((uintptr_t)target | (uintptr_t)source) & (sizeof(T) - 1)) != 0) return MI355_E_INVAL;
    const AddvPlan plan = plan_atomic_add_v(n, device_cus());
    AddvParams p{};
    p.target = target;
    p.source = source;
    p.n = n;
    return launch(atomic_add_v<T>, dim3(plan.grid), st, p);
}

}  // namespace mi355k

using namespace mi355k;

static int amo_impl(int op, int width, void *target, unsigned long long value, unsigned long long cond,
                    unsigned long long *slot, void *stream) {
    if (op < 0 || op >= MI355_NUM_AMO_OPS || (width != 4 && width != 8) || target == nullptr ||
        ((uintptr_t)target & (uintptr_t)(width - 1)) != 0 || ((uintptr_t)slot & 7) != 0)
        return MI355_E_INVAL;
    AmoParams p{};
    p.target = target;
    p.value = value;
    p.cond = cond;
    p.slot = slot;
    p.op = op;
    hipStream_t st = (hipStream_t)stream;
    return width == 4 ? launch(amo_one<uint32_t>, dim3(1), st, p, true, 64)
                      : launch(amo_one<uint64_t>, dim3(1), st, p, true, 64);
}

extern "C" int mi355_amo(int op, int width, void *target, unsigned long long value, unsigned long long cond,
                         unsigned long long *result_slot, void *stream) {
    return t_launch.end_call(amo_impl(op, width, target, value, cond, result_slot, stream));
}

static int addv_impl(int dtype, void *target, const void *source, size_t n, void *stream) {
    if (dtype != MI355_INT && dtype != MI355_LONG && dtype != MI355_LONGLONG && dtype != MI355_FLOAT &&
        dtype != MI355_DOUBLE)
        return MI355_E_UNSUP;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        fire_on_host(st);
        return 0;
    }
    if (target == nullptr || source == nullptr) return MI355_E_INVAL;
    switch (dtype) {
        case MI355_INT: return addv_launch<uint32_t>(target, source, n, st);
        case MI355_FLOAT: return addv_launch<float>(target, source, n, st);
        case MI355_DOUBLE: return addv_launch<double>(target, source, n, st);
        default: return addv_launch<unsigned long long>(target, source, n, st);
    }
}

extern "C" int mi355_atomic_add_v(int dtype, void *target, const void *source, size_t n, void *stream) {
    return t_launch.end_call(addv_impl(dtype, target, source, n, stream));
}

extern "C" void mi355_atomic_add_v_plan(size_t n, int cus, unsigned *grid, unsigned long long *pass) {
    const AddvPlan plan = plan_atomic_add_v(n, cus);
    if (grid != nullptr) *grid = plan.grid;
    if (pass != nullptr) *pass = plan.pass;
}
