"""CPU: the wide sums' ABI -- the four collectives (include/shmemx.h) and
mi355_combine_wide / mi355_combine_wide_plan (include/mi355_reduce.h) are
declared and exported, and the kernel entry rejects what it does not take
before any HIP call (so these run without a GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "osss-gasnet_amd", "lib", "libshmem_reduce.so")
CTYPE = {"half": "shmemx_half_t", "bfloat16": "shmemx_bfloat16_t"}
ENTRY_POINTS = [f"shmemx_{t}_wsum_to_all{suffix}" for t in CTYPE for suffix in ("", "_float")]

MI355_E_INVAL, MI355_E_UNSUP = -1, -2
DT = {"short": 0, "int": 1, "long": 2, "longlong": 3, "float": 4, "double": 5, "longdouble": 6, "complexf": 7,
      "complexd": 8, "half": 9, "bfloat16": 10}
ARGS = r"int nreduce, int PE_start, int logPE_stride, int PE_size\);"


def test_four_entry_points_and_the_kernel_entries_are_exported():
    assert len(ENTRY_POINTS) == 4
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ENTRY_POINTS + ["mi355_combine_wide", "mi355_combine_wide_plan"]:
        assert name in exported, name
    # deliberately not built: no prod / min / max, no stream-ordered form, no pshmem_ twin
    assert not [s for s in exported if re.search(r"_w(prod|min|max)_to_all|wsum_to_all.*on_stream", s)]
    assert not [s for s in exported if s.startswith("pshmem") and "wsum" in s]


def test_declared_in_the_headers():
    x = open(os.path.join(ROOT, "include", "shmemx.h")).read()
    for t, c in CTYPE.items():
        assert re.search(rf"void shmemx_{t}_wsum_to_all \({c} \*target, const {c} \*source, " + ARGS, x), t
        assert re.search(rf"void shmemx_{t}_wsum_to_all_float \(float \*target, const {c} \*source, " + ARGS, x), t
    m = open(os.path.join(ROOT, "include", "mi355_reduce.h")).read()
    assert re.search(r"int mi355_combine_wide \(int dtype, int out_dtype, void \*dst, const void \*const \*srcs, "
                     r"int nsrc, size_t n, void \*stream\);", m)
    assert re.search(r"void mi355_combine_wide_plan \(size_t n, int out_dtype, int cus, unsigned \*grid, "
                     r"unsigned long long \*pass\);", m)


def test_a_c_caller_compiles_against_the_declarations(tmp_path):
    src = tmp_path / "wide_decl.c"
    src.write_text("""#include <shmemx.h>
#include <mi355_reduce.h>
void never_called (shmemx_half_t *h, shmemx_bfloat16_t *b, float *f)
{
    shmemx_half_wsum_to_all (h, h, 0, 0, 0, 1);
    shmemx_half_wsum_to_all_float (f, h, 0, 0, 0, 1);
    shmemx_bfloat16_wsum_to_all (b, b, 0, 0, 0, 1);
    shmemx_bfloat16_wsum_to_all_float (f, b, 0, 0, 0, 1);
    (void) mi355_combine_wide (MI355_BFLOAT16, MI355_FLOAT, 0, 0, 1, 0, 0);
    mi355_combine_wide_plan (0, MI355_FLOAT, 256, 0, 0);
}
int main (void) { return 0; }
""")
    libdir = os.path.dirname(LIB)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir,
                    "-lshmem_reduce", f"-Wl,-rpath,{libdir}", "-o", str(tmp_path / "wide_decl")], check=True)


@pytest.fixture(scope="module")
def combine_wide():
    f = ctypes.CDLL(LIB, mode=ctypes.RTLD_GLOBAL).mi355_combine_wide
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                  ctypes.c_size_t, ctypes.c_void_p]
    return f


def test_rejected_before_any_hip_call(combine_wide):
    """host buffers stand in for device memory: nothing may touch them or the GPU"""
    buf = (ctypes.c_uint32 * 16)()
    v = ctypes.addressof(buf)
    srcs = (ctypes.c_void_p * 33)(*([v] * 33))
    env_before = dict(os.environ)
    H, B, F = DT["half"], DT["bfloat16"], DT["float"]
    # the sources' type: half or bfloat16 only; the output: the same type or float only
    for dtype in range(-1, 12):
        if dtype not in (H, B):
            for out in (dtype, F, H):
                assert combine_wide(dtype, out, v, srcs, 2, 4, None) == MI355_E_UNSUP, (dtype, out)
    for dtype, other in ((H, B), (B, H)):
        for out in list(range(-1, 12)):
            if out not in (dtype, F):
                assert combine_wide(dtype, out, v, srcs, 2, 4, None) == MI355_E_UNSUP, (dtype, out)
        assert combine_wide(dtype, other, v, srcs, 2, 4, None) == MI355_E_UNSUP
    # counts and pointers, for all four (type, output) pairs
    for dtype in (H, B):
        for out in (dtype, F):
            for nsrc in (0, -1, 33, 1 << 20):
                assert combine_wide(dtype, out, v, srcs, nsrc, 4, None) == MI355_E_INVAL, (dtype, out, nsrc)
            assert combine_wide(dtype, out, None, srcs, 2, 4, None) == MI355_E_INVAL
            assert combine_wide(dtype, out, v, None, 2, 4, None) == MI355_E_INVAL
            for bad in (None, v + 1):       # a NULL source; one that is not element-aligned
                for slot in (0, 1, 31):
                    srcs[slot] = bad
                    assert combine_wide(dtype, out, v, srcs, 32, 4, None) == MI355_E_INVAL, (dtype, out, bad, slot)
                    srcs[slot] = v
            assert combine_wide(dtype, out, v + 1, srcs, 2, 4, None) == MI355_E_INVAL
        assert combine_wide(dtype, F, v + 2, srcs, 2, 4, None) == MI355_E_INVAL     # a float target on 2 bytes
        # an error beats the empty call's success only for the type and the count
        assert combine_wide(dtype, DT["double"], v, srcs, 2, 0, None) == MI355_E_UNSUP
        assert combine_wide(dtype, dtype, v, srcs, 0, 0, None) == MI355_E_INVAL
    assert list(buf) == [0] * 16
    assert dict(os.environ) == env_before


def test_n_zero_returns_zero_without_a_gpu(combine_wide):
    buf = (ctypes.c_uint32 * 4)()
    v = ctypes.addressof(buf)
    srcs = (ctypes.c_void_p * 2)(v, v)
    for dtype in (DT["half"], DT["bfloat16"]):
        for out in (dtype, DT["float"]):
            assert combine_wide(dtype, out, v, srcs, 2, 0, None) == 0
            assert combine_wide(dtype, out, None, None, 1, 0, None) == 0
    assert list(buf) == [0] * 4
