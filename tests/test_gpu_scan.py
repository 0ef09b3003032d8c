"""GPU: the scan collectives (include/shmemx.h shmemx_<T>_<op>_inscan /
_exscan) on PE processes sharing the test GPU (tests/_scan_worker.py), every
target bit for bit against tests/_scan_ref.py: both forms, the device heap, in
place, host arrays and partially overlapping buffers, a sub-set of the PEs,
every (type, op) pair, the schedules by name, rounds, host barriers, the
direct schedule against the shard schedule, torch tensors and the C example.
The workers also check that pSync and pWrk are never written and that exscan
leaves member 0's target alone."""
import json
import os
import subprocess
import sys
import uuid

import pytest

import _scan_ref as S
from _pes import launch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(ROOT, "osss-gasnet_amd", "lib")
pytestmark = [pytest.mark.gpu, pytest.mark.multipe]

EIGHT_TYPES = ("double", "float", "int", "longlong", "longdouble", "complexf", "half", "bfloat16")


def run_pes(npes, cases, tmp_path, extra_env=None, timeout=300):
    spec = tmp_path / f"spec_{uuid.uuid4().hex[:6]}.json"
    spec.write_text(json.dumps({"cases": cases}))
    env = {"SHMEM_DEVICE_HEAP_SIZE": "96M", "SHMEM_DEVICE_SCRATCH_SIZE": "384K",
           "SHMEM_SYMMETRIC_HEAP_SIZE": "64M", "SHMEM_BARRIER_TIMEOUT": "120", "SHMEM_PEER_ACQUIRE": "1"}
    env.update(extra_env or {})
    recs = launch(npes, [sys.executable, os.path.join(HERE, "_scan_worker.py"), str(spec)], gpu=True,
                  timeout=timeout, env=env).records()
    for rec in recs:
        assert rec["checked"] == len(cases) and not rec["failures"], rec
    return recs


def case(cases, op, dtype, n, aset, mode="dev", excl=False, **kw):
    c = {"id": len(cases), "op": op, "dtype": dtype, "n": n, "set": list(aset), "mode": mode, "excl": excl,
         "seed": 6000 + len(cases)}
    c.update(kw)
    cases.append(c)
    return c


def ops_of(dtype):
    return [op for op, t in S.PAIRS if t == dtype]


def matrix(npes):
    cases = []
    full = (0, 0, npes)
    for excl in (False, True):
        for n in (0, 1, 257, 40000):
            for mode in ("dev", "inplace", "host", "overlap_up", "overlap_down"):
                case(cases, "sum", "double", n, full, mode, excl)
        for dtype in EIGHT_TYPES:
            for op in ops_of(dtype):
                case(cases, op, dtype, 257, full, "dev", excl)
        case(cases, "max", "float", 40000, full, "inplace", excl)
        case(cases, "sum", "bfloat16", 40000, full, "dev", excl)
        if npes == 4:
            for n in (1, 257, 40000):
                case(cases, "sum", "float", n, (1, 1, 2), "dev", excl)
                case(cases, "min", "double", n, (1, 1, 2), "inplace", excl)
    return cases


def expected_schedule(c, wait_slow):
    size = c["set"][2]
    if c["n"] == 0:
        return "barrier-only"
    if c["mode"] == "host":
        return "scan-staged"
    if size == 1:
        return "scan-local"
    return "scan-p2p-host" if wait_slow else "scan-p2p"


def check_schedules(recs, cases, expect=expected_schedule):
    for pe, rec in enumerate(recs):
        for cid, sched in rec["schedules"].items():
            c = cases[int(cid)]
            assert sched == expect(c, rec["wait_slow"]), (pe, c, sched)


@pytest.mark.parametrize("npes", [1, 2, 3, 4, 5, 9])
def test_both_forms_every_mode(tmp_path, npes):
    """inscan and exscan x n 0, 1, 257, 40000 x device heap, in place, host
    arrays, overlapping either way (double sum); every op of eight types; at 4
    PEs the active set (1, 1, 2); the schedule of every call"""
    cases = matrix(npes)
    recs = run_pes(npes, cases, tmp_path, extra_env={"SHMEM_DEVICE_HEAP_SIZE": "32M"} if npes > 5 else None)
    check_schedules(recs, cases)
    assert all(len(r["schedules"]) > 0 for r in recs)


def test_all_52_pairs_three_pes(tmp_path):
    cases = []
    for op, dtype in S.PAIRS:
        for excl in (False, True):
            case(cases, op, dtype, 1000, (0, 0, 3), "dev", excl)
            case(cases, op, dtype, 257, (0, 0, 3), "inplace", excl)
    assert len(cases) == 52 * 4
    check_schedules(run_pes(3, cases, tmp_path), cases)


def some_cases():
    cases = []
    for excl in (False, True):
        for op, dtype in (("sum", "double"), ("prod", "complexf"), ("max", "float"), ("sum", "bfloat16"),
                          ("xor", "longlong"), ("sum", "longdouble")):
            case(cases, op, dtype, 40000 if dtype != "longdouble" else 3000, (0, 0, 3), "dev", excl)
        case(cases, "sum", "float", 40000, (0, 0, 3), "inplace", excl)
        case(cases, "sum", "double", 40000, (0, 0, 3), "overlap_up", excl)
    return cases


def test_version_area_too_small_for_one_round(tmp_path):
    """SHMEM_DEVICE_ORDER_SIZE at its minimum (128 KiB: 64 KiB per channel, two
    slots of 32 KiB at 3 PEs, of which 512 + 4096 bytes are alignment and
    stagger): one round takes 3 x 28160 bytes, so 40000 elements of 4 or 8
    bytes run in rounds and 40000 of 2 bytes or 3000 long doubles do not"""
    cases = some_cases()
    recs = run_pes(3, cases, tmp_path, extra_env={"SHMEM_DEVICE_ORDER_SIZE": "128K"})
    round_bytes = ((64 << 10) // 2 - 512 - 4096) // 256 * 256 * 3
    assert round_bytes == 84480

    def expect(c, slow):
        es = S.NP[c["dtype"]]().itemsize
        nbytes = c["n"] * es
        if c["mode"].startswith("overlap") or (c["mode"] == "inplace" and c["excl"]):
            # through scratch buffer C in chunks of SHMEM_DEVICE_SCRATCH_SIZE / 3 = 128 KiB, each a
            # schedule of its own; the call reports its last one: the lowest chunk when the target
            # lies above the source (walked top down), else the remainder at the top
            chunk = (384 << 10) // 3
            nbytes = min(chunk, nbytes) if c["mode"] == "overlap_up" else nbytes - (nbytes - 1) // chunk * chunk
        return "scan-p2p-rounds" if nbytes > round_bytes else "scan-p2p"

    check_schedules(recs, cases, expect)
    assert {expect(c, False) for c in cases} == {"scan-p2p-rounds", "scan-p2p"}


def test_host_barrier_form(tmp_path):
    """no signal regions (SHMEM_TEST_IPC_FAIL=sig, as test_gpu_multipe.py): host barriers"""
    cases = some_cases()
    recs = run_pes(3, cases, tmp_path, extra_env={"SHMEM_TEST_IPC_FAIL": "sig"})
    check_schedules(recs, cases, lambda c, slow: "scan-p2p-host")


def test_direct_schedule_matches_the_shard_schedule(tmp_path):
    """SHMEM_SCAN_DIRECT=1 (a testing aid): every member folds its prefix of
    the whole arrays; the same bits as the shard schedule on the same inputs"""
    cases = some_cases()
    shard = run_pes(3, cases, tmp_path)
    check_schedules(shard, cases)
    direct = run_pes(3, cases, tmp_path, extra_env={"SHMEM_SCAN_DIRECT": "1"})
    check_schedules(direct, cases, lambda c, slow: "scan-direct")
    for a, b in zip(shard, direct):
        assert a["digests"] == b["digests"] and len(a["digests"]) == len(cases)


def test_algorithm_requests_and_debug_exchange(tmp_path):
    """EXACT and RCCL requests run the scan schedule and give the same bits;
    SHMEM_DEBUG=1 exchanges the arguments first"""
    cases = []
    for alg in ("auto", "p2p", "exact", "rccl"):
        for excl in (False, True):
            c = case(cases, "sum", "float", 4099, (0, 0, 2), "dev", excl, algorithm=alg)
            c["seed"] = 31     # the same inputs under every request
    recs = run_pes(2, cases, tmp_path, extra_env={"SHMEM_DEBUG": "1"})
    check_schedules(recs, cases)
    for rec in recs:
        for excl in (0, 1):
            assert len({rec["digests"][str(i)] for i in range(excl, len(cases), 2)}) == 1


def test_scan_tensors(tmp_path):
    cases = []
    for tdt in ("float32", "bfloat16"):
        for excl in (False, True):
            cases.append({"id": len(cases), "torch": tdt, "op": "sum", "n": 4099, "excl": excl,
                          "seed": 7300 + len(cases)})
    recs = run_pes(2, cases, tmp_path, extra_env={"SHMEM_DEVICE_SCRATCH_SIZE": "3M"})
    for rec in recs:
        assert set(rec["schedules"].values()) == {"scan-p2p"}, rec


def test_c_example_three_pes(tmp_path):
    exe = str(tmp_path / "scan_example")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "scan_example.c"), "-L", LIBDIR, "-lshmem_reduce",
                    f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    env = dict(os.environ, SHMEM_DEVICE_HEAP_SIZE="16M", SHMEM_DEVICE_SCRATCH_SIZE="3M", SHMEM_BARRIER_TIMEOUT="120")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "oshrun"), "-np", "3", "--same-device", exe],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": PASS") == 3, r.stdout
