"""CPU: the prefix fold's host arithmetic (osss-gasnet_amd/csrc/prefix_plan.h:
which prefix a scan's member takes, the trimming of prefixes nobody takes, the
chained launches beyond one launch's sources and where their carry lives)
compiled for the host under AddressSanitizer and UBSan and run as an ordinary
program (tests/native/prefix_plan_check.cpp), which executes the planned
launches on a symbolic memory."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_chained_launches_deliver_every_prefix(tmp_path):
    exe = str(tmp_path / "prefix_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "osss-gasnet_amd", "csrc"),
                           os.path.join(HERE, "native", "prefix_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"(\d+) cases, (\d+) launches, (\d+) rejected, 0 violations", out.stdout)
    assert m, out.stdout
    cases, launches, rejected = (int(x) for x in m.groups())
    # 32 source counts x (6 fixed + 2 per slot + 4000 random patterns); chained
    # launches and rejected patterns (a NULL slot at a launch's end with no
    # later buffer for the carry) must both occur, or the run checked nothing
    assert cases == 32 * 4006 + 2 * sum(range(1, 33)), cases
    assert launches > cases and rejected > 0, out.stdout
