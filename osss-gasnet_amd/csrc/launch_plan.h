// launch_plan.h -- how a fold over given pointers can run: the one place that
// reads the pointers' phases. Host-only integer arithmetic on addresses (no
// HIP: tests/native/launch_plan_check.cpp compiles it with plain g++ and
// enumerates every phase combination); combine_kernels.h's launchers turn the
// plan into a kernel and a grid. Below the plan, the two grid caps of the
// launch layer (launch.h hands them the device's CU count and the occupancy
// query's answer), the same way: arithmetic only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "residency.h"

namespace mi355k {

enum PlanKind {
    PLAN_ALIGNED,   // 16-byte vectors, every pointer 16-byte aligned after the head
    PLAN_SHIFT,     // 16-byte vectors, aligned outputs, unaligned source loads
    PLAN_ELEMENTS,  // element by element from the pointers as given
};

// Vector kinds: the first `head` elements and the last `tail` (< V = 16 /
// element size) are folded element-wise, `nvec` whole vectors between them
// from the pointers advanced by `head`. ELEMENTS: head = tail = 0, nvec = n
// (the scalar kernels count elements in nvec).
struct LaunchPlan {
    PlanKind kind;
    size_t head, nvec, tail;
};

// es: the element size (2, 4, 8 or 16). shiftable: the type's vector kernels
// exist with unaligned source loads (every type but long double, which runs
// aligned or element-wise). outs: the non-null outputs (none: sources only).
inline LaunchPlan plan_launch(size_t es, bool shiftable, const void *const *outs, int nout,
                              const void *const *srcs, int nsrc, size_t n) {
    const size_t V = 16 / es;
    const LaunchPlan elements = {PLAN_ELEMENTS, 0, n, 0};

    // Vectors need the outputs at one phase within 16 bytes, by whole
    // elements (0, or a user offset into the arrays).
    const uintptr_t pd = nout > 0 ? (uintptr_t)outs[0] & 15 : 0;
    if (pd % es != 0) return elements;
    for (int k = 1; k < nout; ++k)
        if (((uintptr_t)outs[k] & 15) != pd) return elements;

    // The head: elements to peel so that every output starts on a 128-byte
    // line, when the outputs share their offset within one (the symmetric
    // target on each PE) and n reaches past it; else so that they start on
    // 16 bytes. Outputs off their line store partial lines at both ends of
    // every wave's span: a fold or copy whose target sits 16 bytes off its
    // line ran 3-25 % slower warm and up to 30 % slower from HBM
    // (profiles/r05/cold/linepeel_*.jsonl). 16-byte elements and a call
    // without outputs have no head (the kernels fold a head only for V > 1),
    // so they are vectorisable at phase 0 only.
    size_t head = 0;
    if (V > 1 && nout > 0) {
        const uintptr_t pl = (uintptr_t)outs[0] & 127;
        bool line = true;
        for (int k = 1; k < nout; ++k) line = line && ((uintptr_t)outs[k] & 127) == pl;
        const size_t h = ((128 - pl) & 127) / es;
        head = line && n > h ? h : ((16 - pd) & 15) / es;
    }

    bool srcs_aligned = true;
    for (int k = 0; k < nsrc; ++k) srcs_aligned = srcs_aligned && (((uintptr_t)srcs[k] + head * es) & 15) == 0;

    PlanKind kind;
    if (srcs_aligned) {
        // ALIGNED: the sources share the outputs' phase. A head that n does
        // not reach past leaves nothing to run as vectors. (head > 0 with
        // n <= head is always the 16-byte head of a phase other than 0: the
        // line head is only taken when n > it.)
        if (head != 0 && n <= head) return elements;
        kind = PLAN_ALIGNED;
    } else {
        // SHIFT: some source at another phase than the outputs (an offset
        // into some of the arrays; an unaligned-form load of an aligned
        // address is the same instruction, so sources at several phases
        // share the kernel). Needs an output to align to and, unlike
        // ALIGNED, at least one whole vector after the head. At the aligned
        // launch shapes (cold_probe unal: the same rates at 2 or 4 blocks
        // per CU).
        if (!shiftable || nout == 0 || n < head + V) return elements;
        kind = PLAN_SHIFT;
    }
    return {kind, head, (n - head) / V, (n - head) % V};
}

// The streaming cap (launch.h, grid_for): blocks that cover `units` once at
// `per_pass` units per block, at least one, at most blocks_per_cu per CU --
// the kernels' grid-stride loops cover the rest.
inline unsigned streaming_grid(uint64_t units, uint64_t per_pass, int cus, int blocks_per_cu) {
    uint64_t want = (units + per_pass - 1) / per_pass;
    const uint64_t cap = (uint64_t)cus * blocks_per_cu;
    if (want < 1) want = 1;
    return (unsigned)(want < cap ? want : cap);
}

// The co-residency cap (launch.h, coresident_grid): `want` blocks, at most
// what `share` processes on one GPU can each keep resident at once. Per CU:
// `occupancy` (the occupancy query's blocks per CU at 256 threads; a failed
// query counts as 1), at most MI355_FUSED_RESIDENT_PER_CU, one fewer as a
// margin but never none.
inline unsigned coresident_cap(int occupancy, int cus, int share, uint64_t want) {
    int n = occupancy < MI355_FUSED_RESIDENT_PER_CU ? occupancy : MI355_FUSED_RESIDENT_PER_CU;
    const int per_cu = n > 1 ? n - 1 : 1;
    uint64_t cap = (uint64_t)per_cu * (uint64_t)cus / (uint64_t)(share > 1 ? share : 1);
    if (cap < 1) cap = 1;
    if (want > cap) want = cap;
    return (unsigned)(want < 1 ? 1 : want);
}

}  // namespace mi355k
