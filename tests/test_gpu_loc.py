"""GPU: the value-and-location collectives (include/shmemx.h
shmemx_<T>_maxloc_to_all / _minloc_to_all) on PE processes sharing the test GPU
(tests/_loc_worker.py), every member's target and target_loc bit for bit
against tests/_loc_ref.py -- and so equal to each other's: both operators,
n 0, 1, 257, 40000, out of place and in place, explicit and NULL source_loc,
all 16 (type, op) pairs, sub-sets of the PEs, the schedule of every call, and
torch tensors. The workers also check that the sources stay as they were, that
nothing past a target is written, and that the inputs exercised every rule."""
import json
import os
import sys
import uuid

import pytest

import _loc_ref as L
from _pes import launch

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = [pytest.mark.gpu, pytest.mark.multipe]


def run_pes(npes, cases, tmp_path, extra_env=None, timeout=300, require_rules=False):
    spec = tmp_path / f"spec_{uuid.uuid4().hex[:6]}.json"
    spec.write_text(json.dumps({"cases": cases, "require_rules": require_rules}))
    env = {"SHMEM_DEVICE_HEAP_SIZE": "96M", "SHMEM_DEVICE_SCRATCH_SIZE": "384K",
           "SHMEM_SYMMETRIC_HEAP_SIZE": "64M", "SHMEM_BARRIER_TIMEOUT": "120", "SHMEM_PEER_ACQUIRE": "1"}
    env.update(extra_env or {})
    recs = launch(npes, [sys.executable, os.path.join(HERE, "_loc_worker.py"), str(spec)], gpu=True,
                  timeout=timeout, env=env).records()
    for rec in recs:
        assert rec["checked"] == len(cases) and not rec["failures"], rec
    return recs


def case(cases, op, dtype, n, aset, inplace=False, explicit=True):
    cases.append({"id": len(cases), "op": op, "dtype": dtype, "n": n, "set": list(aset), "inplace": inplace,
                  "explicit": explicit, "seed": 8000 + len(cases)})


def matrix(npes):
    cases = []
    full = (0, 0, npes)
    for op in L.OPS:
        for n in (0, 1, 257, 40000):
            for inplace in (False, True):
                for explicit in (True, False):
                    case(cases, op, "float", n, full, inplace, explicit)
        for dtype in L.DTYPES:
            case(cases, op, dtype, 257, full)
        case(cases, op, "int", 40000, full)
        case(cases, op, "bfloat16", 40000, full, inplace=True)
        case(cases, op, "double", 40000, full, explicit=False)
        if npes == 4:
            for aset in ((1, 1, 2), (0, 1, 2)):
                for n in (1, 257, 40000):
                    case(cases, op, "half", n, aset)
                    case(cases, op, "long", n, aset, inplace=True)
    return cases


def expected_schedule(c):
    if c["n"] == 0:
        return "barrier-only"
    return "loc-local" if c["set"][2] == 1 else "loc-p2p"


def check(recs, cases, npes):
    member_digests = {}
    for pe, rec in enumerate(recs):
        for cid, sched in rec["schedules"].items():
            c = cases[int(cid)]
            assert sched == expected_schedule(c), (pe, c, sched)
            if c["n"]:
                # the fold kernel, or none on a member whose shard is empty; the first member's never is
                k = rec["kernels"][cid]
                assert "mi355k::loc_fold_" in k or (k == "" and pe != c["set"][0]), (pe, c, k)
        for cid, d in rec["digests"].items():
            member_digests.setdefault(cid, set()).add(d)
    # every member holds the same pair (each also equals the model, checked by the worker)
    assert all(len(d) == 1 for d in member_digests.values()), member_digests
    assert len(member_digests) == len(cases)


@pytest.mark.parametrize("npes", [1, 2, 3, 4, 5, 9])
def test_both_operators_every_form(tmp_path, npes):
    cases = matrix(npes)
    recs = run_pes(npes, cases, tmp_path, extra_env={"SHMEM_DEVICE_HEAP_SIZE": "32M"} if npes > 5 else None,
                   require_rules=npes >= 2)
    check(recs, cases, npes)
    assert all(len(r["schedules"]) > 0 for r in recs)


def test_loc_to_all_tensors(tmp_path):
    cases = []
    for tdt in ("float32", "bfloat16", "int64"):
        for op in L.OPS:
            for explicit in (True, False):
                cases.append({"id": len(cases), "torch": tdt, "op": op, "n": 4099, "explicit": explicit,
                              "seed": 8300 + len(cases)})
    recs = run_pes(3, cases, tmp_path, extra_env={"SHMEM_DEVICE_SCRATCH_SIZE": "3M"})
    for rec in recs:
        assert set(rec["schedules"].values()) == {"loc-p2p"}, rec
