// launch.h -- the kernel layer's one host-side launch path: what a caller
// armed for the calling thread's next launch and what that thread launched
// last (LaunchState), the launch itself (launch_recorded, launch), and the
// grids' device-dependent inputs (device_cus, resident_blocks) handed to the
// pure cap arithmetic of launch_plan.h (grid_for, coresident_grid). Host code
// only: combine_kernels.h (the folds, copies, strided pull, atomics, prefix
// folds) and fused.hip (the one-launch collectives) both launch through it.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <type_traits>
#include <utility>

#include "launch_plan.h"
#include "mi355_reduce.h"

namespace mi355k {

constexpr int kBlock = 256;

// Completion signal (mi355_signal_next_launch): the last block to finish
// stores `epoch` into a host-visible word, so the host learns the result is
// in memory ~4 us sooner than through hipStreamSynchronize (tools/probes/latency.hip:
// 6.9 vs 10.7 us for a launch round trip on MI355X).
struct Signal {
    unsigned *count;  // device word, 0 between launches (the last block resets it)
    unsigned *flag;   // host-coherent word the host spins on; nullptr = no signal
    unsigned epoch;
};

inline int g_cus[64];

// What a caller armed for this thread's next launch, and what this thread
// launched last: the one owner of that state. Who takes what:
//   launch_recorded()     the event pair, always; it records the kernel and
//                         its grid, which therefore always describe one and
//                         the same launch. mi355_fused_allreduce and
//                         mi355_fused_pull launch through it directly (their
//                         kernels have no Signal member: the fused protocol
//                         reports through its own host flag).
//   launch()              launch_recorded(), and the signal when the launch
//                         is the call's `final` one (earlier launches of a
//                         multi-launch call run unsignalled)
//   mi355_fused_server    records its kernel and grid (LaunchState::record)
//                         and takes nothing: an armed event pair stays armed
//                         for the next launch (the resident grid ends long
//                         after the call that started it)
//   launch_fixed()        the NaN words, before anything else: the k-source
//                         fold is the only kernel that carries them
//   next_copy_descends()  the direction pin (combine.hip: single-segment copies)
//   fire_on_host()        a call with nothing to launch fires the signal from
//                         the host and takes it; the events stay armed for the
//                         next launch
//   end_call()            every entry point returns through it: `spent` names
//                         what the entry consumes even when it launched
//                         nothing or another kernel than the one that carries
//                         it; an error return also cancels the signal, the
//                         events and `on_error` (nothing will carry them).
//                         mi355_combine: the NaN words spent, the pin dropped
//                         on error; mi355_combine_orders: the pin dropped on
//                         error; mi355_copy_segments: the pin spent (a
//                         multi-segment launch always ascends);
//                         mi355_nan_patch_copy and the strided copies: neither.
// Bare hipLaunchKernelGGL, taking nothing and recording nothing: the device
// barrier (it runs after the strided pull whose grid the all-to-all tests
// then read back), mi355_acquire_system (it runs between the arming and the
// fold that carries the signal and the events), the two short converters and
// the self-test kernels (poke, the three peeks, mark, producer-read).
enum { ARMED_NAN = 1, ARMED_DIR = 2 };
struct LaunchState {
    Signal sig = {nullptr, nullptr, 0};                  // mi355_signal_next_launch
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;    // mi355_time_next_launch
    unsigned long long *nan_set = nullptr, *nan_clear = nullptr;   // mi355_nan_flag_next_launch
    int copy_dir = 0;   // mi355_copy_direction_next_launch: > 0 ascending, < 0 descending, 0: none
    const void *last_kernel = nullptr;   // host stub of the kernel launched last (mi355_last_kernel)
    unsigned last_grid[2] = {0, 0};      // ... and its grid (mi355_last_launch_grid)

    void record(const void *kernel, dim3 grid) {
        last_kernel = kernel;
        last_grid[0] = grid.x, last_grid[1] = grid.y;
    }

    int end_call(int rc, unsigned spent = 0, unsigned on_error = 0) {
        if (rc != 0) {
            sig = Signal{nullptr, nullptr, 0};
            ev_start = ev_stop = nullptr;
            spent |= on_error;
        }
        if (spent & ARMED_NAN) nan_set = nan_clear = nullptr;
        if (spent & ARMED_DIR) copy_dir = 0;
        return rc;
    }
};
inline thread_local LaunchState t_launch;

// A host-visible word the host can also write: an armed signal that no kernel
// will carry (nothing to launch) is fired right here, in stream order.
inline void fire_on_host(hipStream_t st) {
    Signal &sig = t_launch.sig;
    if (sig.flag == nullptr) return;
    if (hipStreamSynchronize(st) == hipSuccess) __atomic_store_n(sig.flag, sig.epoch, __ATOMIC_RELEASE);
    sig = Signal{nullptr, nullptr, 0};
}

// One launch of `kernel(args...)`, recorded, carrying the event pair armed by
// mi355_time_next_launch (if any) as hipExtLaunchKernel stamps: no marker
// packets on the stream. `block`: threads per block.
template <typename K, typename... A>
int launch_recorded(K kernel, dim3 grid, unsigned block, hipStream_t st, const A &...args) {
    LaunchState &s = t_launch;
    s.record((const void *)kernel, grid);
    if (s.ev_start != nullptr || s.ev_stop != nullptr) {
        hipExtLaunchKernelGGL(kernel, grid, dim3(block), 0, st, s.ev_start, s.ev_stop, 0, args...);
        s.ev_start = s.ev_stop = nullptr;
    } else {
        hipLaunchKernelGGL(kernel, grid, dim3(block), 0, st, args...);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// A kernel whose one argument carries a Signal member `sig`.
// `final`: the last launch of an API call, the one that carries the signal;
// `block`: threads per block (amo.hip's one-wave kernel: 64)
template <typename K, typename P>
int launch(K kernel, dim3 grid, hipStream_t st, P p, bool final = true, unsigned block = kBlock) {
    LaunchState &s = t_launch;
    p.sig = Signal{nullptr, nullptr, 0};
    if (final) {
        p.sig = s.sig;
        s.sig = Signal{nullptr, nullptr, 0};
    }
    return launch_recorded(kernel, grid, block, st, p);
}

inline int device_cus() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (g_cus[dev] == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            cus <= 0)
            cus = 256;
        g_cus[dev] = cus;
    }
    return g_cus[dev];
}

// Blocks for a streaming launch: enough to cover the work once, capped at
// kBlocksPerCU resident blocks per CU (grid-stride covers the rest).
constexpr int kBlocksPerCU = 8;

// Blocks of `fn` (256 threads each) one CU holds at once (occupancy API, at
// least 1, cached per kernel).
// A grid-stride launch larger than what is resident runs in rounds, the last
// one partly empty. The VALU-bound x87 folds cap their grids at this (the
// every-member x87 sum at 8 sources: 80 VGPRs, 6 blocks per CU instead of
// the 8 asked: 271 -> 263 us at 8 x 32 MiB, profiles/r03/orders_grid_cap.jsonl).
// The HBM-bound folds do not: capped at their residency (the 8-source fold
// holds 152 VGPRs, 3 blocks per CU) they ran 1-4 % slower -- the queued
// blocks refill CUs as others finish.
// Several host threads may launch (the launch state is per thread):
// readers see an entry only once its key and value are written (release /
// acquire on `used`), writers append under a mutex.
inline int resident_blocks(const void *fn) {
    static const void *keys[512];
    static int vals[512];
    static std::atomic<int> used{0};
    static std::mutex mu;
    const int seen = used.load(std::memory_order_acquire);
    for (int i = 0; i < seen; ++i)
        if (keys[i] == fn) return vals[i];
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, kBlock, 0) != hipSuccess || n < 1) n = 1;
    (void)hipGetLastError();
    std::lock_guard<std::mutex> lock(mu);
    const int u = used.load(std::memory_order_relaxed);
    for (int i = seen; i < u; ++i)
        if (keys[i] == fn) return vals[i];  // another thread added it meanwhile
    if (u < 512) {
        keys[u] = fn;
        vals[u] = n;
        used.store(u + 1, std::memory_order_release);
    }
    return n;
}

inline unsigned grid_for(uint64_t units_per_block_pass, uint64_t units, int blocks_per_cu = kBlocksPerCU) {
    return streaming_grid(units, units_per_block_pass, device_cus(), blocks_per_cu);
}

// Co-residency: every block of the spin-waiting grids (fused_allreduce,
// fused_server, fused_pull) waits for the grid's last block and for the other
// members, so all blocks of every such grid running on this GPU at once must
// be resident together. A launch is capped at the kernel's resident blocks
// per CU x CUs, divided among the `share` processes that may run such grids
// here at the same time (launch_plan.h, coresident_cap). Resident blocks per
// CU: the occupancy query, but at most MI355_FUSED_RESIDENT_PER_CU
// (residency.h) -- 256-thread blocks are admitted per CU up to
// floor(800 / (ceil(sgpr / 16) * 16 + 16)) (MI355X_MICROARCH.md "Residency"),
// which the query ignores (at 103-106 SGPRs: 6 per CU where the query says 8;
// 9 PEs x 174 blocks on one GPU never all started) -- and one fewer as a
// margin. The build checks every such kernel's SGPR/VGPR/LDS use against the
// constant (tools/check_residency.py).
inline unsigned coresident_grid(const void *fn, uint64_t want, int share) {
    return coresident_cap(resident_blocks(fn), device_cus(), share, want);
}

// A run-time v in [Lo, Hi] as a compile-time constant: f(std::integral_constant<int, v>),
// MI355_E_INVAL outside the range. One instantiation of f per value. Compared
// from Hi down: the compiler then emits the kernels those instantiations name
// in ascending order, as the switch ladders this replaces did, which keeps
// each translation unit's device code byte for byte what it was.
template <int Hi, typename F, int... I>
int with_constant(int v, F &&f, std::integer_sequence<int, I...>) {
    int rc = MI355_E_INVAL;
    (void)((v == Hi - I && (rc = f(std::integral_constant<int, Hi - I>{}), true)) || ...);
    return rc;
}
template <int Lo, int Hi, typename F>
int with_constant(int v, F &&f) {
    return with_constant<Hi>(v, f, std::make_integer_sequence<int, Hi - Lo + 1>{});
}

}  // namespace mi355k
