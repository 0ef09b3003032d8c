// wide.hip -- the widening fold (gfx950): mi355_combine_wide, the kernel
// behind shmemx_<T>_wsum_to_all / _wsum_to_all_float (reduce.c).
//
// The sum of nsrc half or bfloat16 arrays accumulated in binary32:
//   acc = float(src_0)                        exact widening
//   acc = fl32(acc + float(src_j))            j = 1 .. nsrc - 1, ascending
//   dst = round_to_T(acc)   or   dst = acc    one rounding, or none
// fl32 is the IEEE binary32 add (to nearest even, subnormal operands and
// results kept: the object is built with -ffp-contract=off and the default
// denormal modes). A NaN result is canonical (0x7E00 / 0x7FC0 / 0x7FC00000)
// at every nsrc, 1 included, so one source is a conversion, not a byte copy.
// The specification is the model in tests/_wide_ref.py; the reference has
// nothing to compare with.
//
// Each source byte is read once, the running sums stay in registers from the
// first source to the last and nothing 16-bit exists in between: that is what
// mi355_combine cannot express (its accumulator has the element type).
//
// Three forms, chosen in wide_plan.h (mi355_wide_form_of) and visible in the
// recorded kernel's name; the same bits in each:
//   wide_fold_vec   the target 16-byte aligned and every source aligned to its
//                   unit: per lane and source one 16-byte load of 8 elements
//                   (float output: one 8-byte load of 4), non-temporal; one
//                   16-byte write-through store per lane; the tail (n mod 8
//                   or 4 elements) element-wise by block 0
//   wide_fold_unal  the target aligned, some source not: the same with
//                   unaligned loads (combine_kernels.h, ld16_src)
//   wide_fold_elem  the target off the 16-byte phase, or less than one unit:
//                   one element per lane
// All are grid-stride loops of 256-thread blocks, at most 4 blocks per CU;
// no LDS, no scratch (the build checks).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mi355_reduce.h"
#include "wide_kernels.h"

using namespace mi355k;

template <typename T>
static int wide_typed(bool float_out, WideParams &p, const mi355_wide_plan &plan, hipStream_t st) {
    return float_out ? wide_launch<T, true>(p, plan, st) : wide_launch<T, false>(p, plan, st);
}

static int wide_impl(int dtype, int out_dtype, void *dst, const void *const *srcs, int nsrc, size_t n, void *stream) {
    if (dtype != MI355_HALF && dtype != MI355_BFLOAT16) return MI355_E_UNSUP;
    if (out_dtype != dtype && out_dtype != MI355_FLOAT) return MI355_E_UNSUP;
    if (nsrc < 1 || nsrc > MI355_WIDE_MAX_SOURCES) return MI355_E_INVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        fire_on_host(st);
        return 0;
    }
    const bool float_out = out_dtype == MI355_FLOAT;
    if (dst == nullptr || srcs == nullptr) return MI355_E_INVAL;
    if (((uintptr_t)dst & (float_out ? 3 : 1)) != 0) return MI355_E_INVAL;
    for (int j = 0; j < nsrc; ++j)
        if (srcs[j] == nullptr || ((uintptr_t)srcs[j] & 1) != 0) return MI355_E_INVAL;

    WideParams p{};
    p.dst = dst;
    for (int j = 0; j < nsrc; ++j) p.src[j] = srcs[j];
    p.nsrc = nsrc;
    const mi355_wide_plan plan =
        mi355_wide_plan_launch(mi355_wide_form_of(float_out, dst, srcs, nsrc, n), float_out, n, device_cus());
    return dtype == MI355_HALF ? wide_typed<f16>(float_out, p, plan, st) : wide_typed<bf16>(float_out, p, plan, st);
}

extern "C" int mi355_combine_wide(int dtype, int out_dtype, void *dst, const void *const *srcs, int nsrc, size_t n,
                                  void *stream) {
    return t_launch.end_call(wide_impl(dtype, out_dtype, dst, srcs, nsrc, n, stream));
}

extern "C" void mi355_combine_wide_plan(size_t n, int out_dtype, int cus, unsigned *grid, unsigned long long *pass) {
    const mi355_wide_plan plan = mi355_wide_plan_launch(MI355_WIDE_VECTOR, out_dtype == MI355_FLOAT, n, cus);
    if (grid != nullptr) *grid = plan.grid;
    if (pass != nullptr) *pass = plan.pass;
}
