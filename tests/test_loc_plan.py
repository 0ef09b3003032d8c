"""CPU: the value-and-location fold's host arithmetic
(osss-gasnet_amd/csrc/loc_plan.h: the form of a launch, its grid and what a
pass of it covers, the chained calls beyond one call's sources) compiled for
the host under AddressSanitizer and UBSan and run as an ordinary program
(tests/native/loc_plan_check.cpp), which executes the planned chain on a
symbolic memory and the kernels' index arithmetic on a coverage map."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_chain_visits_every_source_once_and_launches_cover_every_element(tmp_path):
    exe = str(tmp_path / "loc_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "osss-gasnet_amd", "csrc"),
                           os.path.join(HERE, "native", "loc_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"(\d+) chains, (\d+) calls, (\d+) launches, 0 violations", out.stdout)
    assert m, out.stdout
    chains, calls, launches = (int(x) for x in m.groups())
    # 100 source counts x 8 location patterns x 3 bases; 33 .. 100 sources take
    # 2 to 4 calls; 3 element sizes x 2 forms x (5001 sizes + 3 CU counts x 2
    # passes x the sizes within a vector of the pass edge)
    assert chains == 100 * 8 * 3
    per_count = sum(1 if k <= 32 else 1 + -(-(k - 32) // 31) for k in range(1, 101))
    assert calls == per_count * 8 * 3 and calls > chains
    edges = sum(2 * (16 // es) + 3 for es in (2, 4, 8)) + 3 * 5     # 2 V + 3 sizes per edge; element form: V = 1
    assert launches == 3 * 2 * 5001 + 3 * 2 * edges
