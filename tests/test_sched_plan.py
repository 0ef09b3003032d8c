"""CPU: the schedule planner (osss-gasnet_amd/csrc/sched_plan.h: which of
identity, fused one-shot or two-shot, shard schedule with device or host
barriers, rounds, the two-member NaN pair, EXACT, direct or shard scan, or a
walk through scratch a reduction or scan call runs) compiled for the host
under AddressSanitizer and UBSan and run as an ordinary program
(tests/native/sched_plan_check.c): its invariants over every supported
(op, type) pair, set size, entry point, overlap and boundary size under every
combination of the job's settings, a digest of all the plans, and two dozen
cases spelt out. The GPU side of the same decisions is
test_gpu_sched_plan.py."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "sched_plan_check.c")
INCLUDES = ["-I", os.path.join(ROOT, "osss-gasnet_amd", "csrc"), "-I", os.path.join(ROOT, "include")]

# FNV-1a over every field of every enumerated plan. Recorded from the control
# flow the planner replaced -- reduce_symmetric, p2p_any, fused_range,
# reduce_on_stream, scan_symmetric and scan_any of reduce.c restated line by
# line as a "legacy chooser" with shmemi.x read as env->x, and run through this
# same enumeration; the planner gave the same plan on every case before the
# chooser was deleted.
CASES = 28836912
DIGEST = "ea375914120d5c15"


def build(tmp_path_factory):
    path = tmp_path_factory.mktemp("sched_plan") / "sched_plan_check"
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined"] + INCLUDES + [SRC, "-o", str(path)])
    return str(path)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory)


def test_every_request_keeps_the_invariants_and_the_recorded_plans(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{CASES} cases" in out.stdout, out.stdout
    assert "0 violations" in out.stdout, out.stdout
    assert f"digest {DIGEST}," in out.stdout, out.stdout


def test_the_planner_is_cxx_too():
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + INCLUDES + [SRC])


S, D = 1 << 20, 1 << 30   # a source and a target far above it, both 16-byte aligned
ENV = ["fused_max=2097152", "oneshot_max=65536", "order_chunk=268435456", "scratch_chunk=268435456", "npes=64"]
ROUND3 = ((256 << 20) // 2 - 512 - 4096) // 256 * 256 * 3 // 8   # doubles per ordered round at 3 PEs
# (why, settings, COLL:ENTRY:OP:TYPE:SIZE:ME, dst, src, n) -> the plan's line
NAMED = [
    ("double sum, 3 PEs, at oneshot_max: one-shot", [], "reduce:blocking:sum:double:3:0", D, S, 8192,
     "fused-oneshot ordered oneshot"),
    ("... one element above it: two-shot", [], "reduce:blocking:sum:double:3:0", D, S, 8193,
     "fused-twoshot ordered"),
    ("... at oneshot_max in place: one-shot would overwrite a source others still read", [],
     "reduce:blocking:sum:double:3:0", S, S, 8192, "fused-twoshot ordered"),
    ("... in place above it", [], "reduce:blocking:sum:double:3:0", S, S, 8193, "fused-twoshot ordered"),
    ("... at fused_max: still one launch", [], "reduce:blocking:sum:double:3:0", D, S, 262144,
     "fused-twoshot ordered"),
    ("... one element above fused_max: shards, every member's order, one round", [],
     "reduce:blocking:sum:double:3:0", D, S, 262145, f"p2p ORDERS DEV round={ROUND3} ordered"),
    ("... one element above the round size: rounds", [], "reduce:blocking:sum:double:3:0", D, S, ROUND3 + 1,
     f"p2p-rounds ORDERS DEV round={ROUND3} ordered"),
    ("double one element off 16 bytes: no fused kernel", [], "reduce:blocking:sum:double:3:0", D + 8, S + 8, 1000,
     f"p2p ORDERS DEV round={ROUND3} ordered"),
    ("double complex one element off: 16 bytes, still aligned", [], "reduce:blocking:sum:complexd:3:0", D + 16, S + 16,
     1000, "fused-oneshot ordered oneshot"),
    ("bfloat16 at a fused size: the fused kernel has no 16-bit types", [], "reduce:blocking:sum:bfloat16:3:0", D, S,
     1000, f"p2p ORDERS DEV round={ROUND3 * 4} ordered"),
    ("long long and: integers have one result, PE_start's order", [], "reduce:blocking:and:longlong:3:0", D, S, 1000,
     "fused-oneshot oneshot"),
    ("float max, 2 PEs above fused_max: ordered (selects by position), not the NaN pair", [],
     "reduce:blocking:max:float:2:0", D, S, 1 << 20, "p2p ORDERS DEV round=134215424 ordered"),
    ("float sum, 2 PEs above fused_max: the NaN pair, no version areas, no rounds", [],
     "reduce:blocking:sum:float:2:1", D, S, 1 << 20, "p2p PAIR DEV round=1048576"),
    ("long double sum, 2 PEs: x87 NaNs agree, order-free", [], "reduce:blocking:sum:longdouble:2:0", D, S, 1 << 20,
     "p2p FOLD DEV round=1048576"),
    ("double sum, 9 PEs, reference order: within MI355_ORDERS_MAX_SOURCES (32), every member's order", [],
     "reduce:blocking:sum:double:9:0", D, S, 1000, "fused-oneshot ordered oneshot"),
    ("double sum, 33 PEs, reference order: beyond it, EXACT", [], "reduce:blocking:sum:double:33:0", D, S, 1000,
     "exact"),
    ("... under pe_start: shards, host barriers (beyond MI355_FUSED_MAX_MEMBERS)", ["order=pe_start"],
     "reduce:blocking:sum:double:33:0", D, S, 1000, "p2p-host FOLD HOST round=1000"),
    ("double sum, 3 PEs, target 5 elements above source: through scratch, top down", [],
     "reduce:blocking:sum:double:3:0", S + 40, S, 1000,
     f"p2p ORDERS DEV round={ROUND3} ordered scratch-down chunk=33554432"),
    ("EXACT by request", ["algorithm=exact"], "reduce:blocking:sum:double:3:0", D, S, 1000, "exact"),
    ("device waits time-sliced: host barriers, but the fused kernel is a matter of fused_max", ["dev_wait_slow=1"],
     "reduce:blocking:sum:double:3:0", D, S, 262145, f"p2p-host ORDERS HOST round={ROUND3} ordered"),
    ("one PE with the persistent server enabled: a copy the server may take", ["persistent=1"],
     "reduce:blocking:sum:double:1:0", D, S, 1000, "identity oneshot servable"),
    ("exscan in place: the owner's prefix would land on a source, through scratch; member 0 receives nothing", [],
     "exscan:blocking:sum:double:3:0", S, S, 1000,
     f"scan-p2p EXSCAN DEV round={ROUND3} ordered scratch-up chunk=33554432 no-target"),
    ("inscan in place, shard schedule: the one aliasing the prefix fold takes", [], "inscan:blocking:sum:double:3:1",
     S, S, 1000, f"scan-p2p INSCAN DEV round={ROUND3} ordered"),
    ("inscan in place, direct schedule: the target would be the fold's last source", ["scan_direct=1"],
     "inscan:blocking:sum:double:3:1", S, S, 1000, "scan-direct scratch-up chunk=33554432"),
    ("17-member scan: shards up to MI355_ORDERS_MAX_SOURCES", [], "inscan:blocking:sum:double:17:0", D, S, 1000,
     "scan-p2p INSCAN DEV round=35641792 ordered"),
    ("33-member scan: direct", [], "inscan:blocking:sum:double:33:0", D, S, 1000, "scan-direct"),
    ("stream call, 9-member double sum: ordered sets up to 32 members run", [], "reduce:stream:sum:double:9:0", D, S,
     1000, "stream-fused-oneshot ordered oneshot"),
    ("stream call, 33 members: an error", [], "reduce:stream:sum:double:33:0", D, S, 1000, "error stream-members"),
    ("stream call under EXACT: the request binds the blocking calls only", ["algorithm=exact"],
     "reduce:stream:sum:double:3:0", D, S, 1000, "stream-fused-oneshot ordered oneshot"),
    ("peer reads broken, 2 PEs: an error", ["p2p_broken=1"], "reduce:blocking:sum:int:2:0", D, S, 1000,
     "error p2p-broken"),
    ("the smallest version area, 33-member pe_start... 17-member scan: too small", ["order_chunk=65536"],
     "inscan:blocking:sum:double:17:0", D, S, 1000, "error order-area"),
]


def test_named_cases(exe):
    for why, settings, head, dst, src, n, want in NAMED:
        out = subprocess.run([exe, "plan"] + ENV + settings + [f"{head}:{dst}:{src}:{n}"], capture_output=True,
                             text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip() == want, why
