// prefix.hip -- the C ABI of the prefix fold (mi355_reduce.h
// mi355_combine_prefix): argument checks and the dispatch to the element
// types' translation units (prefix_t_*.hip, kernels in prefix_kernels.h).
#include <hip/hip_runtime.h>

#include "mi355_reduce.h"
#include "prefix_kernels.h"

using namespace mi355k;

static int combine_prefix_impl(int op, int dtype, void *const *dsts, const void *const *srcs, int nsrc, size_t n,
                               void *stream) {
    if (!mi355_op_supported(op, dtype)) return MI355_E_UNSUP;
    if (nsrc < 1 || nsrc > MI355_ORDERS_MAX_SOURCES || dsts == nullptr || srcs == nullptr) return MI355_E_INVAL;
    for (int k = 0; k < nsrc; ++k)
        if (srcs[k] == nullptr) return MI355_E_INVAL;
    hipStream_t st = (hipStream_t)stream;
    // the prefixes after the last output anybody takes are not computed
    const int used = mi355_prefix_trim(dsts, nsrc);
    if (n == 0 || used == 0) {
        fire_on_host(st);
        return 0;
    }
    // prefix 0 alone is a copy (nothing to do in place): the k-source fold's one-source form
    if (used == 1) return mi355_combine(op, dtype, dsts[0], srcs, 1, n, stream);
    switch (dtype) {
    case MI355_SHORT: return prefix_short(op, dsts, srcs, used, n, st);
    case MI355_INT: return prefix_int(op, dsts, srcs, used, n, st);
    case MI355_LONG:
    case MI355_LONGLONG: return prefix_long(op, dsts, srcs, used, n, st);
    case MI355_FLOAT: return prefix_float(op, dsts, srcs, used, n, st);
    case MI355_DOUBLE: return prefix_double(op, dsts, srcs, used, n, st);
    case MI355_LONGDOUBLE: return prefix_longdouble(op, dsts, srcs, used, n, st);
    case MI355_COMPLEXF: return prefix_complexf(op, dsts, srcs, used, n, st);
    case MI355_COMPLEXD: return prefix_complexd(op, dsts, srcs, used, n, st);
    case MI355_HALF: return prefix_half(op, dsts, srcs, used, n, st);
    case MI355_BFLOAT16: return prefix_bfloat16(op, dsts, srcs, used, n, st);
    default: return MI355_E_INVAL;
    }
}

// Returns through LaunchState::end_call as mi355_combine_orders does: no NaN
// words taken, the copy-direction pin dropped on error.
extern "C" int mi355_combine_prefix(int op, int dtype, void *const *dsts, const void *const *srcs, int nsrc,
                                    size_t n, void *stream) {
    return t_launch.end_call(combine_prefix_impl(op, dtype, dsts, srcs, nsrc, n, stream), 0, ARMED_DIR);
}
