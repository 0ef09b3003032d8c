"""CPU: the fold launchers' plan (osss-gasnet_amd/csrc/launch_plan.h: aligned
vectors, vectors with unaligned source loads, or element by element, and the
head peeled to the outputs' 128-byte line) compiled for the host under
AddressSanitizer and UBSan and run as an ordinary program
(tests/native/launch_plan_check.cpp): its invariants over every phase
combination of outputs and sources, a digest of all the plans, and a dozen
cases spelt out; and the launch layer's two grid caps (the streaming cap and
the spin-waiting grids' co-residency cap) the same way. The GPU side of the same decisions is
test_gpu_combine.py::test_launch_identity_matches_recorded_table."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# FNV-1a over (kind, head, nvec, tail) of every enumerated case. Recorded from
# the three functions the planner replaced (line_head, vector_head and
# shift_head of combine_kernels.h, asked in the launchers' order: vectors,
# then shifted vectors, then elements) run through this same enumeration; the
# planner gave the same plan on every case before they were deleted.
CASES = 3075264
DIGEST = "1c6ab20e6c54662d"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("launch_plan") / "launch_plan_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "osss-gasnet_amd", "csrc"),
                           os.path.join(HERE, "native", "launch_plan_check.cpp"), "-o", str(path)])
    return str(path)


def test_every_phase_combination_keeps_the_invariants_and_the_recorded_plans(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{CASES} cases" in out.stdout, out.stdout
    assert "0 violations" in out.stdout, out.stdout
    assert f"digest {DIGEST}," in out.stdout, out.stdout


T, S = 0x1000, (0x2000, 0x3000, 0x4000)   # a target and sources, each on its own 128-byte line
# (what, element size, shiftable, n, outputs, sources) -> "KIND head nvec tail"
NAMED = [
    ("double, target &t[1] over source &s[0]: the line head, unaligned loads",
     8, 1, 1000, [T + 8], [S[0]], "SHIFT 15 492 1"),
    ("... n == the line head: only the 16-byte head is peeled",
     8, 1, 15, [T + 8], [S[0]], "SHIFT 1 7 0"),
    ("... n == head + V: one whole vector is enough",
     8, 1, 3, [T + 8], [S[0]], "SHIFT 1 1 0"),
    ("... n == head + V - 1: no whole vector, element by element",
     8, 1, 2, [T + 8], [S[0]], "ELEMENTS 0 2 0"),
    ("double, every pointer one element off, n == the line head",
     8, 1, 15, [T + 8], [S[0] + 8, S[1] + 8], "ALIGNED 1 7 0"),
    ("... n == the 16-byte head: nothing left for vectors",
     8, 1, 1, [T + 8], [S[0] + 8, S[1] + 8], "ELEMENTS 0 1 0"),
    ("short, target 112 bytes into its line, n just past the line head",
     2, 1, 9, [T + 112], [S[0] + 112], "ALIGNED 8 0 1"),
    ("... n at the line head: phase 0 needs no head",
     2, 1, 8, [T + 112], [S[0] + 112], "ALIGNED 0 1 0"),
    ("long double 8 bytes off: neither vector kind",
     16, 0, 100, [T + 8], [S[0] + 8], "ELEMENTS 0 100 0"),
    ("long double, one source 8 bytes off: no unaligned loads for it",
     16, 0, 100, [T], [S[0], S[1] + 8], "ELEMENTS 0 100 0"),
    ("double complex, one source 8 bytes off",
     16, 1, 100, [T], [S[0], S[1] + 8], "SHIFT 0 100 0"),
    ("float, two outputs at one offset within their lines: the line head",
     4, 1, 1000, [T + 20, T + 0x100 + 20], [S[0] + 4, S[1] + 4], "ALIGNED 27 243 1"),
    ("float, two outputs 16 bytes apart within a line: the 16-byte head",
     4, 1, 1000, [T + 20, T + 0x100 + 36], [S[0] + 4, S[1] + 4], "ALIGNED 3 249 1"),
    ("float, outputs at two 16-byte phases",
     4, 1, 1000, [T, T + 0x100 + 4], [S[0], S[1]], "ELEMENTS 0 1000 0"),
    ("float, a target off its element size",
     4, 1, 1000, [T + 2], [S[0] + 2], "ELEMENTS 0 1000 0"),
    ("no outputs, sources aligned",
     4, 1, 1000, [], [S[0], S[1]], "ALIGNED 0 250 0"),
    ("no outputs, one source off: nothing to align to",
     4, 1, 1000, [], [S[0], S[1] + 4], "ELEMENTS 0 1000 0"),
]


# The two grid caps of the launch layer (launch_plan.h streaming_grid and
# coresident_cap). FNV-1a over every grid of the sweep, recorded from the two
# function bodies these replaced -- grid_for of combine_kernels.h and
# coresident_grid of fused.hip, their device queries turned into arguments --
# run through this same enumeration before they were deleted; the new
# functions gave the same grid on every case.
CAP_CASES = 5632
CAP_DIGEST = "8d705bf8d63b622b"

# ceil(units / per_pass), at least 1, at most cus x blocks_per_cu
STREAMING = [  # (units, per_pass, cus, blocks_per_cu) -> grid
    ((0, 1024, 256, 8), 1),
    ((1024, 1024, 256, 8), 1),
    ((1025, 1024, 256, 8), 2),
    ((2**40, 1024, 256, 1), 256),
    ((2**40, 1024, 304, 2), 608),
]
# per_cu = max(min(occupancy, 6) - 1, 1); cap = max(per_cu x cus / max(share, 1), 1); max(min(want, cap), 1)
RESIDENT = [  # (occupancy, cus, share, want) -> grid
    ((8, 256, 1, 10**6), 1280),
    ((8, 256, 9, 10**6), 142),      # 1280 / 9
    ((3, 256, 2, 10**6), 256),      # 2 x 256 / 2
    ((1, 256, 1, 10**6), 256),      # the margin never reaches zero
    ((0, 256, 1, 10**6), 256),      # a failed query counts as one
    ((6, 4, 64, 10**6), 1),
    ((8, 256, 0, 5), 5),            # share 0 treated as 1
    ((8, 256, 1, 0), 1),
]


def test_grid_caps_named_cases(exe):
    cases = [("stream", a, want) for a, want in STREAMING] + [("resident", a, want) for a, want in RESIDENT]
    out = subprocess.run([exe, "caps"] + [":".join([kind] + [str(v) for v in a]) for kind, a, _ in cases],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.split()
    assert len(got) == len(cases), out.stdout
    for (kind, a, want), g in zip(cases, got):
        assert int(g) == want, (kind, a)


def test_grid_caps_sweep_keeps_the_invariants_and_the_recorded_grids(exe):
    out = subprocess.run([exe, "capsweep"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{CAP_CASES} cases" in out.stdout, out.stdout
    assert "0 violations" in out.stdout, out.stdout
    assert f"digest {CAP_DIGEST}," in out.stdout, out.stdout


def test_named_cases(exe):
    args = [f"{es}:{sh}:{n}:{','.join(map(str, outs)) or '-'}:{','.join(map(str, srcs))}"
            for _, es, sh, n, outs, srcs, _ in NAMED]
    out = subprocess.run([exe, "plan"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(NAMED), out.stdout
    for (what, *_, want), line in zip(NAMED, got):
        assert line == want, what
