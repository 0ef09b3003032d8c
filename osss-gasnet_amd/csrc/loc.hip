// loc.hip -- the value-and-location fold (gfx950): mi355_combine_loc, the
// kernel behind shmemx_<T>_maxloc_to_all / _minloc_to_all (reduce.c).
//
// Each source j contributes, per element, a candidate pair (value, location);
// the location is read from src_locs[j] or, where that is NULL, is loc_base + j
// for every element. The result is the left fold over the sources in ascending
// order, acc = beats(cand_j, acc) ? cand_j : acc, with (maxloc; minloc has <
// for >)
//   b beats a  <=>  b.v is a NaN and (a.v is not, or b.l < a.l), or
//                   neither is a NaN and (b.v > a.v, or b.v == a.v and b.l < a.l)
// so a NaN beats every number in both operators and reports where it is, -0
// and +0 tie (the smaller location decides), half and bfloat16 compare by the
// float values they denote, and two candidates equal in class and location
// keep the earlier source. The winner's value bits are stored as they were
// loaded: the kernels move bit patterns and only compare what they denote
// (loc_kernels.h, loc_beats). Nothing is rounded, so every schedule that
// presents the sources in ascending order gives the same bits.
//
// Two forms, chosen in loc_plan.h (mi355_loc_plan_launch) and visible in the
// recorded kernel's name:
//   loc_fold_vec   every value and location pointer 16-byte aligned: one
//                  16-byte vector of values per lane and source (8, 4 or 2
//                  elements) and its locations as 4, 2 or 1 16-byte loads;
//                  non-temporal loads, write-through stores, the tail
//                  (n mod V elements) element-wise by block 0
//   loc_fold_elem  any other element-aligned phase: one element per lane
// Both are grid-stride loops of 256-thread blocks, at most 8 blocks per CU,
// keep the running winner in registers and loop over the sources at run time
// (the pointer table is in the kernel arguments); no LDS, no scratch (the
// build checks). The location loads of a lane are 16-byte loads V * 8 bytes
// apart, so a wave's location instruction touches every line of its span once
// per k -- the V / 2 instructions together read each line whole.
//
// Not here: long double and complex (no total order worth a kernel), a fused
// one-launch collective, and the reference has nothing to compare with -- the
// specification is the model in tests/_loc_ref.py.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "loc_kernels.h"
#include "mi355_reduce.h"

using namespace mi355k;

static_assert(sizeof(long) == 8 && sizeof(long long) == 8, "LP64: locations are 64-bit");

template <typename T>
static int loc_typed(int op, LocParams &p, const mi355_loc_plan &plan, hipStream_t st) {
    return op == MI355_OP_MAX ? loc_launch<MI355_OP_MAX, T>(p, plan, st) : loc_launch<MI355_OP_MIN, T>(p, plan, st);
}

static size_t loc_elem_size(int dtype) {
    switch (dtype) {
        case MI355_SHORT:
        case MI355_HALF:
        case MI355_BFLOAT16: return 2;
        case MI355_INT:
        case MI355_FLOAT: return 4;
        case MI355_LONG:
        case MI355_LONGLONG:
        case MI355_DOUBLE: return 8;
        default: return 0;
    }
}

static int loc_impl(int op, int dtype, void *dst_val, long *dst_loc, const void *const *src_vals,
                    const long *const *src_locs, long loc_base, int nsrc, size_t n, void *stream) {
    const size_t es = loc_elem_size(dtype);
    if ((op != MI355_OP_MIN && op != MI355_OP_MAX) || es == 0) return MI355_E_UNSUP;
    if (nsrc < 1 || nsrc > MI355_LOC_MAX_SOURCES) return MI355_E_INVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        fire_on_host(st);
        return 0;
    }
    if (dst_val == nullptr || dst_loc == nullptr || src_vals == nullptr) return MI355_E_INVAL;
    uintptr_t val_bits = (uintptr_t)dst_val, loc_bits = (uintptr_t)dst_loc;
    for (int j = 0; j < nsrc; ++j) {
        if (src_vals[j] == nullptr) return MI355_E_INVAL;
        val_bits |= (uintptr_t)src_vals[j];
        if (src_locs != nullptr) loc_bits |= (uintptr_t)src_locs[j];
    }
    if ((val_bits & (es - 1)) != 0 || (loc_bits & 7) != 0) return MI355_E_INVAL;

    LocParams p{};
    p.dst_val = dst_val;
    p.dst_loc = (long long *)dst_loc;
    for (int j = 0; j < nsrc; ++j) {
        p.src_val[j] = src_vals[j];
        p.src_loc[j] = src_locs != nullptr ? (const long long *)src_locs[j] : nullptr;
    }
    p.loc_base = loc_base;
    p.nsrc = nsrc;
    const mi355_loc_plan plan =
        mi355_loc_plan_launch(es, mi355_loc_aligned(dst_val, dst_loc, src_vals, src_locs, nsrc), n, device_cus());
    switch (dtype) {
        case MI355_SHORT: return loc_typed<int16_t>(op, p, plan, st);
        case MI355_INT: return loc_typed<int32_t>(op, p, plan, st);
        case MI355_FLOAT: return loc_typed<float>(op, p, plan, st);
        case MI355_DOUBLE: return loc_typed<double>(op, p, plan, st);
        case MI355_HALF: return loc_typed<f16>(op, p, plan, st);
        case MI355_BFLOAT16: return loc_typed<bf16>(op, p, plan, st);
        default: return loc_typed<long long>(op, p, plan, st);  // long and long long: int64
    }
}

extern "C" int mi355_combine_loc(int op, int dtype, void *dst_val, long *dst_loc, const void *const *src_vals,
                                 const long *const *src_locs, long loc_base, int nsrc, size_t n, void *stream) {
    return t_launch.end_call(loc_impl(op, dtype, dst_val, dst_loc, src_vals, src_locs, loc_base, nsrc, n, stream));
}
