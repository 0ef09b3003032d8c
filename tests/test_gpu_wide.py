"""GPU: the wide-sum collectives (include/shmemx.h shmemx_<T>_wsum_to_all /
_wsum_to_all_float) on PE processes sharing the test GPU
(tests/_wide_worker.py), every member's target bit for bit against
tests/_wide_ref.py -- and so equal to each other's, which the digests check
again: both types and both outputs, n 0, 1, 257, 40000, out of place and in
place, sub-sets of the PEs, the schedule and the kernel of every call, the same
bits under SHMEM_REDUCE_ORDER=pe_start, torch tensors, and the calls the Python
layer refuses. The workers also check that the sources stay as they were and
that nothing past a target is written. tests/test_wide_ref.py asserts on the
CPU that these inputs exercise every class of the model and differ from the
stepwise 16-bit fold on 5 % of the elements or more."""
import json
import os
import sys
import uuid

import pytest

import _wide_ref as W
from _pes import launch

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = [pytest.mark.gpu, pytest.mark.multipe]


def run_pes(npes, cases, tmp_path, extra_env=None, timeout=300):
    spec = tmp_path / f"spec_{uuid.uuid4().hex[:6]}.json"
    spec.write_text(json.dumps({"cases": cases}))
    env = {"SHMEM_DEVICE_HEAP_SIZE": "32M", "SHMEM_DEVICE_SCRATCH_SIZE": "384K",
           "SHMEM_SYMMETRIC_HEAP_SIZE": "64M", "SHMEM_BARRIER_TIMEOUT": "120", "SHMEM_PEER_ACQUIRE": "1"}
    env.update(extra_env or {})
    recs = launch(npes, [sys.executable, os.path.join(HERE, "_wide_worker.py"), str(spec)], gpu=True,
                  timeout=timeout, env=env).records()
    for rec in recs:
        assert rec["checked"] == len(cases) and not rec["failures"], rec
    return recs


def case(cases, dtype, out_float, n, aset, inplace=False):
    cases.append({"id": len(cases), "dtype": dtype, "float": out_float, "n": n, "set": list(aset),
                  "inplace": inplace, "seed": W.SEEDS[len(cases) % 2]})


def matrix(npes):
    cases = []
    full = (0, 0, npes)
    for dtype in W.TYPES:
        for n in (0, 1, 257, 40000):
            case(cases, dtype, False, n, full)
            case(cases, dtype, True, n, full)
            case(cases, dtype, False, n, full, inplace=True)
        if npes == 4:
            for aset in ((1, 1, 2), (0, 1, 2)):
                for n in (1, 257, 40000):
                    case(cases, dtype, False, n, aset)
                    case(cases, dtype, True, n, aset)
                    case(cases, dtype, False, n, aset, inplace=True)
    return cases


def expected_schedule(c):
    if c["n"] == 0:
        return "barrier-only"
    return "wide-local" if c["set"][2] == 1 else "wide-p2p"


def check(recs, cases):
    member_digests = {}
    for pe, rec in enumerate(recs):
        for cid, sched in rec["schedules"].items():
            c = cases[int(cid)]
            assert sched == expected_schedule(c), (pe, c, sched)
            if c["n"]:
                # the fold kernel, or none on a member whose shard is empty; the first member's never is
                k = rec["kernels"][cid]
                assert "mi355k::wide_fold_" in k or (k == "" and pe != c["set"][0]), (pe, c, k)
                if c["n"] >= 8 * c["set"][2] * 128:     # every shard whole units on heap-aligned arrays
                    assert "mi355k::wide_fold_vec" in k, (pe, c, k)
        for cid, d in rec["digests"].items():
            member_digests.setdefault(cid, set()).add(d)
    # every member holds the same bits (each also equals the model, checked by the worker)
    assert all(len(d) == 1 for d in member_digests.values()), member_digests
    assert len(member_digests) == len(cases)
    return {cid: next(iter(d)) for cid, d in member_digests.items()}


@pytest.mark.parametrize("npes", [1, 2, 3, 4, 5, 9])
def test_both_types_both_outputs_every_form(tmp_path, npes):
    cases = matrix(npes)
    recs = run_pes(npes, cases, tmp_path)
    check(recs, cases)
    assert all(len(r["schedules"]) > 0 for r in recs)


def test_the_same_bits_whatever_the_reduce_order_says(tmp_path):
    """3 members: the stepwise sums' members disagree here under the default
    order; the wide sum's digests are the same in both settings"""
    cases = []
    for dtype in W.TYPES:
        for n in (257, 40000):
            case(cases, dtype, False, n, (0, 0, 3))
            case(cases, dtype, True, n, (0, 0, 3))
    default = check(run_pes(3, cases, tmp_path), cases)
    pe_start = check(run_pes(3, cases, tmp_path, extra_env={"SHMEM_REDUCE_ORDER": "pe_start"}), cases)
    assert default == pe_start


def test_wsum_tensors_and_what_it_refuses(tmp_path):
    cases = []
    for tdt in ("float16", "bfloat16"):
        for out_float in (False, True):
            cases.append({"id": len(cases), "torch": tdt, "float": out_float, "n": 4099, "seed": W.SEEDS[len(cases) % 2]})
    cases.append({"id": len(cases), "rejects": True})
    recs = run_pes(3, cases, tmp_path, extra_env={"SHMEM_DEVICE_SCRATCH_SIZE": "3M"})
    for rec in recs:
        assert [rec["schedules"][str(i)] for i in range(5)] == ["wide-p2p"] * 4 + ["refused"], rec
    digests = [{rec["digests"][str(i)] for rec in recs} for i in range(4)]
    assert all(len(d) == 1 for d in digests), digests
