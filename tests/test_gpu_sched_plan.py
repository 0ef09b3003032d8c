"""GPU: the library runs what the planner's check program says it plans.
3 PEs on the test GPU with small thresholds set explicitly (fused up to
16 KiB, one-shot up to 4 KiB, version areas of 64 KiB per channel, so an
ordered round is 3 x 28160 bytes); calls whose sizes ARE the plan's boundaries
-- n x es = 4 KiB, one element more, 16 KiB, one element more, one element
more than a round, and n = 2 (one shard empty) -- blocking and on a stream, in
place and not, for double sum, float max, bfloat16 sum and long long and, plus
one inscan and one exscan. Every result is compared bit for bit with the
oracle (tests/test_gpu_multipe.py check, tests/test_gpu_stream_matrix.py
check_cases) or the model (the 16-bit and scan workers check themselves), and
every schedule the library reports with what tests/native/sched_plan_check.c's
`plan` mode prints for the same request under the job's settings: the
expectation is the planner's own (osss-gasnet_amd/csrc/sched_plan.h compiled
for the host), not a restatement here. The workers' buffers come from
shmemx_malloc_device, so the requests' offsets are 16-byte aligned ones."""
import pytest

import test_gpu_half
import test_gpu_multipe
import test_gpu_scan
from test_gpu_stream import stream_case
from test_gpu_stream_matrix import check_cases
from test_sched_plan import build

pytestmark = [pytest.mark.gpu, pytest.mark.multipe]

FUSED_MAX, ONESHOT_MAX, ORDER_CHUNK, SCRATCH_CHUNK = 16 << 10, 4 << 10, 64 << 10, 128 << 10
JOB_ENV = {"SHMEM_FUSED_MAX_BYTES": "16K", "SHMEM_ONESHOT_MAX_BYTES": "4K", "SHMEM_DEVICE_ORDER_SIZE": "128K"}
# the same job as the planner's settings (the workers' jobs have SHMEM_DEVICE_SCRATCH_SIZE=384K: three buffers)
SETTINGS = [f"fused_max={FUSED_MAX}", f"oneshot_max={ONESHOT_MAX}", f"order_chunk={ORDER_CHUNK}",
            f"scratch_chunk={SCRATCH_CHUNK}", "npes=3", "order=reference", "algorithm=auto"]
ROUND_BYTES = (ORDER_CHUNK // 2 - 512 - 4096) // 256 * 256 * 3
FULL3 = [[0, 0, 3]]
ES = {"double": 8, "float": 4, "bfloat16": 2, "longlong": 8}
SRC, DST = 1 << 20, 1 << 24   # stand-ins for the workers' aligned, disjoint buffers


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory)


def planned(exe, calls, extra=()):
    """The schedule name the planner gives each (coll, entry, op, dtype, n, inplace)."""
    import subprocess
    reqs = [f"{coll}:{entry}:{op}:{dtype}:3:1:{SRC if inplace else DST}:{SRC}:{n}"
            for coll, entry, op, dtype, n, inplace in calls]
    out = subprocess.run([exe, "plan"] + SETTINGS + list(extra) + reqs, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    names = [line.split()[0] for line in out.stdout.splitlines()]
    assert len(names) == len(calls) and "error" not in names, out.stdout
    return names


def boundary(dtype, what):
    es = ES[dtype]
    return {"oneshot": ONESHOT_MAX // es, "oneshot+1": ONESHOT_MAX // es + 1, "fused": FUSED_MAX // es,
            "fused+1": FUSED_MAX // es + 1, "round+1": ROUND_BYTES // es + 1, "two": 2}[what]


# (op, dtype, boundary, in place) of the blocking and of the stream calls
BLOCKING = [("sum", "double", "oneshot", False), ("sum", "double", "oneshot", True),
            ("sum", "double", "oneshot+1", False), ("sum", "double", "fused", False),
            ("sum", "double", "fused+1", False), ("sum", "double", "round+1", True),
            ("max", "float", "fused+1", True), ("max", "float", "round+1", False),
            ("and", "longlong", "oneshot", False), ("and", "longlong", "round+1", False),
            ("and", "longlong", "two", False)]
STREAM = [("sum", "double", "oneshot", False), ("sum", "double", "oneshot+1", False),
          ("sum", "double", "fused+1", True), ("sum", "double", "round+1", False),
          ("max", "float", "oneshot", True), ("and", "longlong", "fused+1", False),
          ("sum", "bfloat16", "oneshot", False), ("sum", "bfloat16", "round+1", True)]
HALF_BLOCKING = [("sum", "bfloat16", "oneshot", False), ("sum", "bfloat16", "fused+1", True),
                 ("sum", "bfloat16", "round+1", False), ("sum", "bfloat16", "two", False)]
SCANS = [("inscan", "sum", "double", "round+1", True), ("exscan", "sum", "double", "oneshot+1", False)]


def test_reported_schedules_are_the_planners(tmp_path, exe):
    # the reference's types, blocking and on a stream: one job of tests/pe_worker.py
    cases = [{"id": i, "op": op, "dtype": dtype, "n": boundary(dtype, what), "sets": FULL3,
              "mode": "inplace" if inplace else "dev", "seed": 900 + i} for i, (op, dtype, what, inplace) in
             enumerate(BLOCKING)]
    want = planned(exe, [("reduce", "blocking", op, dtype, boundary(dtype, what), inplace)
                         for op, dtype, what, inplace in BLOCKING])
    streamed = [stream_case(100 + i, op, dtype, boundary(dtype, what), FULL3, chain=1, inplace=inplace,
                            thresholds=[FUSED_MAX, ONESHOT_MAX]) for i, (op, dtype, what, inplace) in enumerate(STREAM)]
    for c, name in zip(streamed, planned(exe, [("reduce", "stream", op, dtype, boundary(dtype, what), inplace)
                                               for op, dtype, what, inplace in STREAM])):
        c["expect"] = name
    (tmp_path / "a").mkdir()
    results = test_gpu_multipe.run_pes(3, cases + streamed, tmp_path / "a", extra_env=JOB_ENV)
    test_gpu_multipe.check(results, cases)
    seen = {}
    for c, name in zip(cases, want):
        for pe in range(3):
            assert str(results[pe][f"{c['id']}_schedule"][0]) == name, (c, pe)
        seen[name] = seen.get(name, 0) + 1
    check_cases(results, streamed, seen)

    # bfloat16 blocking: tests/_half_worker.py, which holds every target to the model
    cases = []
    for op, dtype, what, inplace in HALF_BLOCKING:
        test_gpu_half.case(cases, op, dtype, boundary(dtype, what), (0, 0, 3), "inplace" if inplace else "dev")
    want = planned(exe, [("reduce", "blocking", op, dtype, boundary(dtype, what), inplace)
                         for op, dtype, what, inplace in HALF_BLOCKING])
    (tmp_path / "b").mkdir()
    for rec in test_gpu_half.run_pes(3, cases, tmp_path / "b", extra_env=JOB_ENV):
        assert [rec["schedules"][str(c["id"])] for c in cases] == want, rec["schedules"]
    for name in want:
        seen[name] = seen.get(name, 0) + 1

    # the scans: tests/_scan_worker.py, which holds every target to tests/_scan_ref.py
    cases = []
    for coll, op, dtype, what, inplace in SCANS:
        test_gpu_scan.case(cases, op, dtype, boundary(dtype, what), (0, 0, 3), "inplace" if inplace else "dev",
                           coll == "exscan")
    (tmp_path / "c").mkdir()
    for rec in test_gpu_scan.run_pes(3, cases, tmp_path / "c", extra_env=JOB_ENV):
        want = planned(exe, [(coll, "blocking", op, dtype, boundary(dtype, what), inplace)
                             for coll, op, dtype, what, inplace in SCANS], [f"dev_wait_slow={int(rec['wait_slow'])}"])
        assert [rec["schedules"][str(c["id"])] for c in cases] == want, rec["schedules"]
    for name in want:
        seen[name] = seen.get(name, 0) + 1
    print("schedules: " + ", ".join(f"{k} x {v}" for k, v in sorted(seen.items())))
    # the boundaries are real ones: both sides of each were run
    assert {"fused-oneshot", "fused-twoshot", "p2p", "p2p-rounds", "stream-fused-oneshot", "stream-fused-twoshot",
            "stream-p2p", "stream-p2p-rounds"} <= set(seen), seen
