"""GPU: shmem_iput / shmem_iget through the public calls, on PE processes
sharing the test GPU (tests/iputget_worker.py).

Expected values are numpy indexing of the inputs, computed by each PE:
    target[k * tst] = source[k * sst]        k < nelems
Every target is pre-filled with a sentinel byte and compared WHOLE, gaps and
tail included; the source is compared afterwards too. PEs put to (me + 1) % N
and check after a barrier, get from (me + N - 1) % N, and put to / get from
their own number.
"""
import json
import os
import subprocess
import sys

import pytest

from _pes import launch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(ROOT, "osss-gasnet_amd", "lib")
pytestmark = pytest.mark.gpu

SIZES = [1, 2, 4, 8, 16]
STRIDES = [(1, 1), (1, 3), (3, 1), (2, 5)]
NELEMS = [0, 1, 5, 257, 4099]
SYM = ["device", "host"]
LOC = ["device", "host", "pageable"]


def run_pes(npes, cases, tmp_path, extra_env=None, timeout=300):
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"cases": cases}))
    env = {"SHMEM_DEVICE_HEAP_SIZE": "96M", "SHMEM_DEVICE_SCRATCH_SIZE": "384K",
           "SHMEM_SYMMETRIC_HEAP_SIZE": "64M", "SHMEM_BARRIER_TIMEOUT": "120", "SHMEM_PEER_ACQUIRE": "1"}
    env.update(extra_env or {})
    for rec in launch(npes, [sys.executable, os.path.join(HERE, "iputget_worker.py"), str(spec)], gpu=True,
                      timeout=timeout, env=env).records():
        assert rec["checked"] == len(cases) and not rec["failures"], rec


def case(cid, op, es, n, tst, sst, sym, loc, to="next"):
    return {"id": cid, "op": op, "es": es, "n": n, "tst": tst, "sst": sst, "sym": sym, "loc": loc, "to": to,
            "seed": 7000 + cid}


def full_matrix():
    """every element size x strides x nelems x symmetric side x local side, put
    and get; one 40000-element case per size, side pair and direction (with
    the 384 KiB of scratch the staged paths of the larger sizes take several
    pieces); puts and gets to the PE's own number"""
    cases = []
    for es in SIZES:
        for op in ("iput", "iget"):
            for sym in SYM:
                for loc in LOC:
                    for tst, sst in STRIDES:
                        for n in NELEMS:
                            cases.append(case(len(cases), op, es, n, tst, sst, sym, loc))
                    cases.append(case(len(cases), op, es, 40000, 2, 5, sym, loc))
                    for tst, sst in ((2, 5), (1, 3), (1, 1)):
                        cases.append(case(len(cases), op, es, 257, tst, sst, sym, loc, to="self"))
    return cases


@pytest.mark.multipe
@pytest.mark.parametrize("npes", [2, 4])
def test_iput_iget_matrix(tmp_path, npes):
    """Element sizes 1, 2, 4, 8, 16 x strides (1,1) (1,3) (3,1) (2,5) x nelems
    0, 1, 5, 257, 4099 (and 40000) x the symmetric side in the device heap and
    the host heap x the local side in device memory, shmem_malloc'd host
    memory and pageable memory."""
    run_pes(npes, full_matrix(), tmp_path)


@pytest.mark.multipe
def test_iput_branch_of_a_target_on_another_gpu(tmp_path):
    """SHMEM_TEST_IPUT_REMOTE_GPU=1 sends the puts to device-heap targets down
    the branch of a target on another GPU: packed into scratch by the kernel
    (or on the host), placed by the runtime's 2-D copy. One 40000-element put
    of 16-byte elements takes several pieces."""
    cases = []
    for es in SIZES:
        for loc in LOC:
            for tst, sst in STRIDES:
                for n in NELEMS:
                    cases.append(case(len(cases), "iput", es, n, tst, sst, "device", loc))
            cases.append(case(len(cases), "iput", es, 257, 2, 5, "device", loc, to="self"))
    for loc in LOC:
        cases.append(case(len(cases), "iput", 16, 40000, 2, 5, "device", loc))
    run_pes(2, cases, tmp_path, extra_env={"SHMEM_TEST_IPUT_REMOTE_GPU": "1"})


# ---------------------------------------------------------------------------
# callers
# ---------------------------------------------------------------------------
def build_c(tmp_path, source, name):
    exe = str(tmp_path / name)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), source, "-L", LIBDIR,
                    "-lshmem_reduce", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    return exe


def oshrun(exe, npes):
    env = dict(os.environ, SHMEM_DEVICE_HEAP_SIZE="16M", SHMEM_DEVICE_SCRATCH_SIZE="3M", SHMEM_BARRIER_TIMEOUT="120")
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "oshrun"), "-np", str(npes), "--same-device",
                           exe], env=env, capture_output=True, text=True, timeout=120)


@pytest.mark.multipe
def test_c_example_two_pes(tmp_path):
    exe = build_c(tmp_path, os.path.join(ROOT, "examples", "iput_example.c"), "iput_example")
    r = oshrun(exe, 2)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": PASS") == 2, r.stdout


@pytest.mark.multipe
def test_fortran_style_caller_two_pes(tmp_path):
    """shmem_iput4_, shmem_character_iget_ and shmem_iget128_ with every
    argument by reference"""
    exe = build_c(tmp_path, os.path.join(HERE, "native", "iputget_fortran_stub.c"), "iputget_fortran_stub")
    r = oshrun(exe, 2)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": PASS") == 2, r.stdout
