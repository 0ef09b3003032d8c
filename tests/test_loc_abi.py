"""CPU: the value-and-location reductions' ABI -- the 16 collectives
(include/shmemx.h) and mi355_combine_loc (include/mi355_reduce.h) are declared
and exported, and the kernel entry rejects what it does not take before any
HIP call (so these run without a GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

import _loc_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "osss-gasnet_amd", "lib", "libshmem_reduce.so")
ENTRY_POINTS = [f"shmemx_{t}_{op}loc_to_all" for t in L.DTYPES for op in L.OPS]

MI355_E_INVAL, MI355_E_UNSUP = -1, -2
OP = {"sum": 0, "min": 5, "max": 6}
DT = {"short": 0, "int": 1, "long": 2, "longlong": 3, "float": 4, "double": 5, "longdouble": 6, "complexf": 7,
      "complexd": 8, "half": 9, "bfloat16": 10}


def test_sixteen_entry_points_and_the_kernel_entry_are_exported():
    assert len(ENTRY_POINTS) == 16
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ENTRY_POINTS + ["mi355_combine_loc"]:
        assert name in exported, name
    assert not [s for s in exported if s.startswith("pshmem") and "loc_to_all" in s]   # no pshmem_ twin


def test_declared_in_the_headers():
    x = open(os.path.join(ROOT, "include", "shmemx.h")).read()
    ctype = {"short": "short", "int": "int", "long": "long", "longlong": "long long", "float": "float",
             "double": "double", "half": "shmemx_half_t", "bfloat16": "shmemx_bfloat16_t"}
    for t in L.DTYPES:
        for op in L.OPS:
            c = re.escape(ctype[t])
            pat = (rf"void shmemx_{t}_{op}loc_to_all \({c} \*target, long \*target_loc, const {c} \*source, "
                   rf"const long \*source_loc,\s+int nreduce, int PE_start, int logPE_stride, int PE_size\);")
            assert re.search(pat, x), f"shmemx_{t}_{op}loc_to_all"
    m = open(os.path.join(ROOT, "include", "mi355_reduce.h")).read()
    assert re.search(r"int mi355_combine_loc \(int op, int dtype, void \*dst_val, long \*dst_loc,\s+"
                     r"const void \*const \*src_vals, const long \*const \*src_locs, long loc_base,\s+"
                     r"int nsrc, size_t n, void \*stream\);", m)


def test_a_c_caller_compiles_against_the_declarations(tmp_path):
    src = tmp_path / "loc_decl.c"
    calls = "\n".join(f"    {name} (0, 0, 0, 0, 0, 0, 0, 1);" for name in ENTRY_POINTS)
    src.write_text("#include <shmemx.h>\n#include <mi355_reduce.h>\nvoid never_called (void)\n{\n" + calls +
                   "\n    (void) mi355_combine_loc (MI355_OP_MAX, MI355_FLOAT, 0, 0, 0, 0, 0L, 1, 0, 0);\n}\n"
                   "int main (void) { return 0; }\n")
    libdir = os.path.dirname(LIB)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir,
                    "-lshmem_reduce", f"-Wl,-rpath,{libdir}", "-o", str(tmp_path / "loc_decl")], check=True)


@pytest.fixture(scope="module")
def combine_loc():
    f = ctypes.CDLL(LIB, mode=ctypes.RTLD_GLOBAL).mi355_combine_loc
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                  ctypes.POINTER(ctypes.c_void_p), ctypes.c_long, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    return f


def test_rejected_before_any_hip_call(combine_loc):
    """host buffers stand in for device memory: nothing may touch them or the GPU"""
    val = (ctypes.c_double * 4)()
    loc = (ctypes.c_long * 4)()
    v, lp = ctypes.addressof(val), ctypes.addressof(loc)
    srcs = (ctypes.c_void_p * 33)(*([v] * 33))
    locs = (ctypes.c_void_p * 33)(*([lp] * 33))
    env_before = dict(os.environ)
    # any op but min and max; any dtype outside the eight
    assert combine_loc(OP["sum"], DT["double"], v, lp, srcs, locs, 0, 2, 4, None) == MI355_E_UNSUP
    assert combine_loc(OP["max"], DT["longdouble"], v, lp, srcs, locs, 0, 2, 4, None) == MI355_E_UNSUP
    assert combine_loc(OP["min"], DT["complexf"], v, lp, srcs, locs, 0, 2, 4, None) == MI355_E_UNSUP
    assert combine_loc(OP["max"], 11, v, lp, srcs, locs, 0, 2, 4, None) == MI355_E_UNSUP
    assert combine_loc(7, DT["double"], v, lp, srcs, locs, 0, 2, 4, None) == MI355_E_UNSUP
    # counts and pointers
    assert combine_loc(OP["max"], DT["double"], v, lp, srcs, locs, 0, 0, 4, None) == MI355_E_INVAL
    assert combine_loc(OP["max"], DT["double"], v, lp, srcs, locs, 0, 33, 4, None) == MI355_E_INVAL
    assert combine_loc(OP["max"], DT["double"], v, lp, srcs, locs, 0, -1, 4, None) == MI355_E_INVAL
    assert combine_loc(OP["max"], DT["double"], None, lp, srcs, locs, 0, 2, 4, None) == MI355_E_INVAL
    assert combine_loc(OP["max"], DT["double"], v, None, srcs, locs, 0, 2, 4, None) == MI355_E_INVAL
    assert combine_loc(OP["max"], DT["double"], v, lp, None, locs, 0, 2, 4, None) == MI355_E_INVAL
    srcs[1] = None
    assert combine_loc(OP["max"], DT["double"], v, lp, srcs, locs, 0, 2, 4, None) == MI355_E_INVAL
    srcs[1] = v + 4     # not element-aligned
    assert combine_loc(OP["max"], DT["double"], v, lp, srcs, locs, 0, 2, 4, None) == MI355_E_INVAL
    srcs[1] = v
    locs[1] = lp + 4
    assert combine_loc(OP["max"], DT["double"], v, lp, srcs, locs, 0, 2, 4, None) == MI355_E_INVAL
    assert list(val) == [0.0] * 4 and list(loc) == [0] * 4
    assert dict(os.environ) == env_before
