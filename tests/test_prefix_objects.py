"""CPU: the prefix-fold objects (csrc/prefix_t_*.hip) hold their kernels and
none of them uses scratch memory (tools/check_residency.py --no-scratch, the
check the build runs on each of them)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "osss-gasnet_amd", "lib")
TOOL = os.path.join(ROOT, "tools", "check_residency.py")
TYPES = ["short", "int", "long", "float", "double", "longdouble", "complexf", "complexd", "half", "bfloat16"]


@pytest.mark.parametrize("name", TYPES)
def test_prefix_kernels_present_and_scratch_free(name):
    obj = os.path.join(LIB, f"prefix_t_{name}.o")
    assert os.path.exists(obj), f"{obj} not built (run __graft_entry__.build())"
    r = subprocess.run([sys.executable, TOOL, "--no-scratch", obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) kernels in prefix_t_\w+\.o, 0 with scratch", r.stdout)
    assert m and int(m.group(1)) > 0, r.stdout
    # the tool's per-kernel table, for the rows' names only (its admission
    # verdict is about the spin-waiting grids' cap, which these kernels do not use)
    t = subprocess.run([sys.executable, TOOL, obj, "--kernels", "combine_prefix_"], capture_output=True, text=True)
    rows = [ln for ln in t.stdout.splitlines() if "mi355k::combine_prefix_" in ln]
    assert len(rows) == int(m.group(1)), t.stdout[-2000:] + t.stderr[-2000:]
    assert sum("combine_prefix_vec<" in ln for ln in rows) >= 1
    assert sum("combine_prefix_scalar<" in ln for ln in rows) >= 1
