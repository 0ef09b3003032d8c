// prefix_kernels.h -- the prefix fold (mi355_combine_prefix, the scan
// collectives' kernel): dst[k] = src[0] op src[1] op ... op src[k] for every
// k at once, the sources read once. Shared by the per-element-type
// translation units prefix_t_*.hip (as combine_kernels.h is by
// combine_t_*.hip, whose Pack, load/store policies, launch(), grid_for and
// launch state it uses) and prefix.hip (the C ABI).
#pragma once
#include "combine_kernels.h"
#include "prefix_plan.h"

namespace mi355k {

// The parameters are the every-member fold's: NSRC sources, NSRC outputs of
// which some may be null (a kernel argument: the branches are uniform).

// One element of every prefix with the reference's operator: the head and
// tail of the vector kernel and the element-wise kernel. All loads precede
// every store, so an output may alias the source of its own slot.
template <int OP, typename T, int NSRC>
__device__ __forceinline__ void prefix_element(const OrdersParams &p, int64_t i) {
    T v[NSRC];
#pragma unroll
    for (int k = 0; k < NSRC; ++k) v[k] = ((const T *)p.src[k])[i];
    T acc = v[0];
    if (p.dst[0] != nullptr) ((T *)p.dst[0])[i] = acc;
#pragma unroll
    for (int k = 1; k < NSRC; ++k) {
        acc = apply<OP>(acc, v[k]);
        if (p.dst[k] != nullptr) ((T *)p.dst[k])[i] = acc;
    }
}

// Vector i of every prefix, the sources' vectors of that position in x: ONE
// running chain of the fast operator forms (ops.h apply_fast), each prefix
// stored as the chain passes it. 16-bit sums and products store the
// canonicalised value (chain_end) and keep the raw one running, as
// orders_one; prefix 0 is the source's bits as they are. A NaN that enters
// the chain stays to its end, so the chain's last value tells whether any
// prefix took a NaN path: such a lane redoes the chain with the reference's
// operator from the registers and rewrites every output (the same bits
// elsewhere). Every index is a compile-time constant: no register array is
// indexed at run time.
template <int OP, typename T, int NSRC>
__device__ __forceinline__ void prefix_one(const OrdersParams &p, const Pack<T> (&x)[NSRC], uint64_t i) {
    constexpr int V = 16 / sizeof(T);
    Pack<T> acc = x[0];
    if (p.dst[0] != nullptr) st16_fold((u32x4 *)p.dst[0] + i, acc.v);
#pragma unroll
    for (int k = 1; k < NSRC; ++k) {
#pragma unroll
        for (int e = 0; e < V; ++e) acc.e[e] = apply_fast<OP>(acc.e[e], x[k].e[e]);
        if (p.dst[k] != nullptr) {
            Pack<T> o = acc;
            if constexpr (f16_chain<OP, T>()) {
#pragma unroll
                for (int e = 0; e < V; ++e) o.e[e] = chain_end<OP>(acc.e[e]);
            }
            st16_fold((u32x4 *)p.dst[k] + i, o.v);
        }
    }
    if constexpr (NSRC > 1 && has_fast_form<OP, T>()) {
        bool redo = false;
#pragma unroll
        for (int e = 0; e < V; ++e) redo |= redo_needed<OP>(acc.e[e]);
        if (redo) {
            acc = x[0];
#pragma unroll
            for (int k = 1; k < NSRC; ++k) {
#pragma unroll
                for (int e = 0; e < V; ++e) acc.e[e] = apply<OP>(acc.e[e], x[k].e[e]);
                if (p.dst[k] != nullptr) st16_fold((u32x4 *)p.dst[k] + i, acc.v);
            }
        }
    }
}

// Vector path, as combine_orders_vec: every output 16-byte aligned, the
// sources too or (SHIFT) read unaligned; all NSRC * UNROLL loads of a pass
// are issued before the first use.
template <int OP, typename T, int NSRC, int UNROLL, int POL, bool SHIFT = false>
__global__ __launch_bounds__(kBlock) void combine_prefix_vec(OrdersParams p) {
    constexpr int V = 16 / sizeof(T);
    static_assert(!SHIFT || !std::is_same<T, x80>::value, "long double runs aligned or element-wise");
    const uint64_t nvec = p.nvec;
    const uint64_t step = (uint64_t)gridDim.x * kBlock * UNROLL;
    const u32x4 *sb[NSRC];
#pragma unroll
    for (int k = 0; k < NSRC; ++k) sb[k] = (const u32x4 *)p.src[k];
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock * UNROLL + threadIdx.x; base < nvec; base += step) {
        Pack<T> x[UNROLL][NSRC];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint64_t i = base + (uint64_t)u * kBlock;
            if (i < nvec) {
#pragma unroll
                for (int k = 0; k < NSRC; ++k) x[u][k].v = ld16_src<POL, SHIFT>(sb[k], i);
            }
        }
        __builtin_amdgcn_sched_barrier(0);   // loads first (fold_vectors)
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint64_t i = base + (uint64_t)u * kBlock;
            if (i < nvec) prefix_one<OP, T, NSRC>(p, x[u], i);
        }
    }
    const bool tail_block = V > 1 && p.tail != 0 && blockIdx.x == 0;
    if (tail_block && threadIdx.x < p.tail) prefix_element<OP, T, NSRC>(p, (int64_t)(nvec * V + threadIdx.x));
    const bool head_block = V > 1 && p.head != 0 && blockIdx.x == 0;
    if (head_block && threadIdx.x < p.head) prefix_element<OP, T, NSRC>(p, (int64_t)threadIdx.x - (int64_t)p.head);
    signal_done(p.sig, tail_block || head_block);
}

// Element-wise form (PLAN_ELEMENTS): outputs at different 16-byte phases, or
// pointers the vector kernels cannot take.
template <int OP, typename T, int NSRC>
__global__ __launch_bounds__(kBlock) void combine_prefix_scalar(OrdersParams p) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < p.nvec; i += (uint64_t)gridDim.x * kBlock)
        prefix_element<OP, T, NSRC>(p, (int64_t)i);
    signal_done(p.sig, true);
}

// The deepest unroll of combine_prefix_vec over every (op, type, NSRC):
// OrdersShape's, which tests/test_gpu_prefix.py's grid-pass bound assumes.
constexpr int kPrefixMaxUnroll = 4;

// One launch, 2 <= NSRC <= kMaxSrc, at least one output. The launch shape is
// the every-member fold's of the same width (OrdersShape: the same 2 * NSRC
// streams per position when every output is set) -- taken over, not measured
// for this kernel.
template <int OP, typename T, int NSRC>
int launch_prefix_fixed(void *const *dsts, const void *const *srcs, size_t n, hipStream_t st, bool final) {
    constexpr bool shiftable = !std::is_same<T, x80>::value;
    using S = OrdersShape<OP, NSRC, T>;
    static_assert(S::unroll <= kPrefixMaxUnroll, "kPrefixMaxUnroll is the bound the tests use");
    OrdersParams p{};
    const void *outs[kMaxSrc];
    int nout = 0;
    for (int k = 0; k < NSRC; ++k) {
        p.src[k] = srcs[k];
        p.dst[k] = dsts[k];
        if (dsts[k] != nullptr) outs[nout++] = dsts[k];
    }
    // the first non-null output's phase is the target phase; outputs at
    // different phases: element-wise (plan_launch)
    const LaunchPlan plan = plan_launch(sizeof(T), shiftable, outs, nout, srcs, NSRC, n);
    apply_plan(p, p.dst, NSRC, NSRC, plan, sizeof(T));
    if (plan.kind == PLAN_ELEMENTS)
        return launch(combine_prefix_scalar<OP, T, NSRC>, dim3(grid_for((uint64_t)kBlock * 4, n)), st, p, final);
    void (*k)(OrdersParams) = combine_prefix_vec<OP, T, NSRC, S::unroll, S::policy>;
    if constexpr (shiftable) {
        if (plan.kind == PLAN_SHIFT) k = combine_prefix_vec<OP, T, NSRC, S::unroll, S::policy, true>;
    }
    return launch(k, dim3(orders_grid<OP, T, NSRC>((const void *)k, plan.kind, p.nvec)), st, p, final);
}

// Any number of sources >= 2 with a non-null dsts[nsrc - 1]: chained launches
// of at most kMaxSrc sources (prefix_plan.h), the first source of a launch
// the last output of the one before; every launch but the last runs
// unsignalled.
template <int OP, typename T>
int launch_prefix(void *const *dsts, const void *const *srcs, int nsrc, size_t n, hipStream_t st) {
    if constexpr (!valid_pair<OP, T>()) {
        return MI355_E_UNSUP;
    } else {
        static_assert(MI355_PREFIX_LAUNCH_SOURCES == kMaxSrc, "prefix_plan.h cuts the chain at one launch's sources");
        const int chunks = mi355_prefix_chunk_count(nsrc);
        // every chunk planned before the first launch: a fold that cannot run leaves nothing half done
        void *carry = nullptr;
        for (int c = 0; c < chunks; ++c) {
            mi355_prefix_chunk ch;
            if (mi355_prefix_chunk_at(dsts, srcs, nsrc, c, carry, &ch, &carry) != 0) return MI355_E_INVAL;
        }
        carry = nullptr;
        int rc = 0;
        for (int c = 0; c < chunks && rc == 0; ++c) {
            mi355_prefix_chunk ch;
            (void)mi355_prefix_chunk_at(dsts, srcs, nsrc, c, carry, &ch, &carry);
            rc = with_constant<2, kMaxSrc>(ch.nsrc, [&](auto k) {
                return launch_prefix_fixed<OP, T, decltype(k)::value>(ch.dst, ch.src, n, st, ch.final != 0);
            });
        }
        return rc;
    }
}

template <typename T>
int dispatch_prefix(int op, void *const *dsts, const void *const *srcs, int nsrc, size_t n, hipStream_t st) {
    return with_constant<0, MI355_NUM_OPS - 1>(
        op, [&](auto o) { return launch_prefix<decltype(o)::value, T>(dsts, srcs, nsrc, n, st); });
}

// One element type's entry point, defined by prefix_t_<name>.hip
#define MI355_PREFIX_TYPE(T, NAME)                                                                   \
    namespace mi355k {                                                                               \
    int prefix_##NAME(int op, void *const *dsts, const void *const *srcs, int nsrc, size_t n,       \
                      hipStream_t st) {                                                              \
        return dispatch_prefix<T>(op, dsts, srcs, nsrc, n, st);                                      \
    }                                                                                                \
    }
#define MI355_PREFIX_DECL(NAME) \
    int prefix_##NAME(int op, void *const *dsts, const void *const *srcs, int nsrc, size_t n, hipStream_t st);
MI355_PREFIX_DECL(short)
MI355_PREFIX_DECL(int)
MI355_PREFIX_DECL(long)
MI355_PREFIX_DECL(float)
MI355_PREFIX_DECL(double)
MI355_PREFIX_DECL(longdouble)
MI355_PREFIX_DECL(complexf)
MI355_PREFIX_DECL(complexd)
MI355_PREFIX_DECL(half)
MI355_PREFIX_DECL(bfloat16)
#undef MI355_PREFIX_DECL

}  // namespace mi355k
