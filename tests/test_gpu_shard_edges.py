"""GPU: empty and partial shards in the multi-launch shard schedule
(reduce.c), in each of its three flavours: device-flag barriers, host barriers
(SHMEM_TEST_IPC_FAIL=sig) and stream-ordered calls.

Shards start on 256-byte boundaries, so with four members a shard of doubles
is 32 elements: at n = 1, 33, 40 and 97 one to three members own an empty
shard (nothing to fold, nothing for the others to gather from them) and one
owns a partial one. The fused path is off (SHMEM_FUSED_MAX_BYTES=0), which the
reported schedule names confirm. Reductions: sum double (every member's order,
through the version areas) and xor long (the plain fold), against
oracle.reduce_pe. Scans: sum double as inscan and exscan against _scan_ref.py;
_scan_worker.py compares the whole target, sentinel tail included, so exscan's
member 0, which receives nothing, must still hold its sentinel. A two-member
float sum with NaNs of different payloads in both sources (the NaN golden
family, from a column where both operands are NaNs) at n = 1 -- member 1's
shard is empty: the NaN-word clear -- and n = 65, each call twice in a row so
both parities of the NaN word are used. Everything bit for bit.
"""
import os

import numpy as np
import pytest

import oracle
import test_gpu_scan as scan
from _compare import assert_match
from test_gpu_multipe import check, run_pes
from test_gpu_stream import check_stream, stream_case

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = [pytest.mark.gpu, pytest.mark.multipe]

NS = (1, 33, 40, 97)
FULL = [[0, 0, 4]]
PAIRS = [[0, 0, 2], [2, 0, 2]]     # two two-member sets at once
NAN_AT = 16                        # golden_nan_sum_float in_0: both operands NaNs at columns 16 and 16 + 64
MULTI_LAUNCH = {"SHMEM_FUSED_MAX_BYTES": "0"}
HOST_BARRIERS = dict(MULTI_LAUNCH, SHMEM_TEST_IPC_FAIL="sig")


def nan_inputs(n):
    x = np.load(os.path.join(HERE, "golden", "golden_nan_sum_float.npz"))["in_0"][:, NAN_AT:NAN_AT + n]
    bits = np.ascontiguousarray(x).view(np.uint32)
    both = np.isnan(x).all(axis=0) & (bits[0] != bits[1])
    assert both[0] and both[(n - 1) // 64 * 64], "the fixture column no longer holds two different NaNs"
    return [np.ascontiguousarray(r) for r in x]


def nan_case(cid, n, **kw):
    c = {"id": cid, "op": "sum", "dtype": "float", "n": n, "sets": PAIRS, "seed": 0, "golden": 0,
         "family": "nan_", "golden_at": NAN_AT}
    c.update(kw)
    return c


def blocking_cases():
    cases = []
    for n in NS:
        for op, dtype in (("sum", "double"), ("xor", "long")):
            cases.append({"id": len(cases), "op": op, "dtype": dtype, "n": n, "sets": FULL, "mode": "dev",
                          "algorithm": "p2p", "seed": 8100 + len(cases)})
    plain = list(cases)
    for n in (1, 65):
        for _ in range(2):     # twice in a row: both parities of the NaN word
            cases.append(nan_case(len(cases), n, mode="dev", algorithm="p2p"))
    return cases, plain


def check_blocking(results, cases, plain, schedule):
    check(results, plain)
    for c in cases:
        for pe in range(4):
            assert str(results[pe][f"{c['id']}_schedule"][0]) == schedule, (c, pe)
        if "golden" not in c:
            continue
        xs = nan_inputs(c["n"])
        for pe in range(4):
            assert_match(results[pe][str(c["id"])], oracle.reduce_pe("sum", "float", xs, pe % 2), "sum", "float",
                         strict=True, ctx=f"case {c['id']} two members n {c['n']} PE {pe}:")


def test_reductions_device_flags_and_on_stream(tmp_path):
    """one job: the blocking calls (device-flag barriers), then chains of two
    stream-ordered calls of the same reductions"""
    cases, plain = blocking_cases()
    streams = []
    for n in NS:
        for op, dtype in (("sum", "double"), ("xor", "long")):
            streams.append(stream_case(len(cases) + len(streams), op, dtype, n, FULL, chain=2))
    pairs = [nan_case(len(cases) + len(streams) + i, n, kind="stream", chain=2) for i, n in enumerate((1, 65))]
    results = run_pes(4, cases + streams + pairs, tmp_path, extra_env=MULTI_LAUNCH)
    check_blocking(results, cases, plain, "p2p")
    check_stream(results, streams)
    for c in streams + pairs:
        for pe in range(4):
            assert str(results[pe][f"{c['id']}_schedule"][0]) == "stream-p2p", (c, pe)
    for c in pairs:
        xs = nan_inputs(c["n"])
        for step in (1, 2):     # step 2 folds the members' step-1 results, which differ in payload
            xs = [oracle.reduce_pe("sum", "float", xs, i) for i in range(2)]
            for pe in range(4):
                assert_match(results[pe][f"{c['id']}_{step}"], xs[pe % 2], "sum", "float", strict=True,
                             ctx=f"case {c['id']} two members on a stream, n {c['n']} step {step} PE {pe}:")


def test_reductions_host_barriers(tmp_path):
    cases, plain = blocking_cases()
    check_blocking(run_pes(4, cases, tmp_path, extra_env=HOST_BARRIERS), cases, plain, "p2p-host")


@pytest.mark.parametrize("env,schedule", [(None, "scan-p2p"), ({"SHMEM_TEST_IPC_FAIL": "sig"}, "scan-p2p-host")],
                         ids=["device-flags", "host-barriers"])
def test_scans(tmp_path, env, schedule):
    cases = []
    for n in NS:
        for excl in (False, True):
            scan.case(cases, "sum", "double", n, (0, 0, 4), "dev", excl)
    recs = scan.run_pes(4, cases, tmp_path, extra_env=env)
    scan.check_schedules(recs, cases, lambda c, slow: schedule)
    assert all(len(r["schedules"]) == len(cases) for r in recs)
