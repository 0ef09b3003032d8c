"""CPU: the widening fold's host arithmetic (osss-gasnet_amd/csrc/wide_plan.h:
the form of a launch, its grid and what a pass of it covers) compiled for the
host under AddressSanitizer and UBSan and run as an ordinary program
(tests/native/wide_plan_check.c), and the exported mi355_combine_wide_plan
against the same arithmetic."""
import ctypes
import os
import re
import subprocess

import _wide_ref as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "osss-gasnet_amd", "lib", "libshmem_reduce.so")


def test_grids_stay_under_the_cap_and_ranges_tile_every_size(tmp_path):
    exe = str(tmp_path / "wide_plan_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "osss-gasnet_amd", "csrc"),
                           os.path.join(HERE, "native", "wide_plan_check.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"(\d+) launches, 0 violations", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) == 3 * 2 * 3 * 22      # CU counts x outputs x forms x sizes


def test_the_exported_plan_is_the_vector_forms():
    f = ctypes.CDLL(LIB, mode=ctypes.RTLD_GLOBAL).mi355_combine_wide_plan
    f.restype = None
    f.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint),
                  ctypes.POINTER(ctypes.c_ulonglong)]

    def plan(n, out, cus):
        g, p = ctypes.c_uint(), ctypes.c_ulonglong()
        f(n, out, cus, ctypes.byref(g), ctypes.byref(p))
        return g.value, p.value

    FLOAT, HALF, BF16 = 4, 9, 10
    for out in (FLOAT, HALF, BF16):
        for cus in (1, 64, 256):
            cap = cus * W.BLOCKS_PER_CU
            unit = W.PER_LANE[out == FLOAT]      # elements of a lane's one 16-byte store
            block = W.BLOCK * unit
            for n in (0, 1, 3, 4, 7, 8, 9, 2047, 2048, 2049, cap * block - 1, cap * block, cap * block + 1, 1 << 26):
                grid, per_pass = plan(n, out, cus)
                assert grid == min(max(1, -(-(n // unit) // W.BLOCK)), cap), (n, out, cus, grid)
                assert per_pass == grid * block
            assert plan(1 << 40, out, cus)[1] == W.grid_pass(out == FLOAT, cus)
    f(100, FLOAT, 256, None, None)      # null outputs are skipped
