"""GPU: put / get and the pull collectives broadcast, fcollect and collect of
csrc/coll.c at every byte phase, edge and route, against the byte-exact model
of tests/_datamove_ref.py (whole guarded images of every buffer a call may
touch: result, both guards, the unchanged source, the root's target).

Each job's PEs run tests/_datamove_worker.py, which also reads the launch
layer's record after every call: the tests assert, case by case, the route
(put / get: copy kernel, its shifted form, hipMemcpy, memmove, no-op) or the
schedule (collectives: fused_pull, copy kernel between device barriers, host
barriers, none)
the model names, and that each setting reaches its full set of routes.

All PEs of a test job share one GPU, so put_bytes' branch for a target on
another GPU (the runtime's P2P copy) cannot be reached here; nothing fakes it.

The jobs are marked `multipe` (they start before this process initialises
HIP); the in-process test runs as PE 0 of 1 on the `shm` fixture.
"""
import json
import os
import sys
import time

import pytest

import _datamove_ref as ref
from _pes import launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# every other route leaves the marker
KERNEL_OF = {"copy": "copy", "shift": "shift", "fused_pull": "fused_pull", "host_wait": "signal"}
DEFAULT_CHUNK = 256 << 20      # SHMEM_DEVICE_SCRATCH_SIZE's default of 768M, in three chunks
CHUNK_3M = 1 << 20
CHUNK_PAIR = (CHUNK_3M - 8, CHUNK_3M, CHUNK_3M + 8)   # just below, at and just above a scratch chunk


def run_job(tmp_path, npes, spec, env, timeout=150):
    path = tmp_path / "spec.json"
    path.write_text(json.dumps(spec))
    e = {"SHMEM_BARRIER_TIMEOUT": "60", "SHMEM_WAIT_TIMEOUT": "60", "SHMEM_DEVICE_HEAP_SIZE": "512M"}
    e.update(env)
    job = launch(npes, [sys.executable, os.path.join(HERE, "_datamove_worker.py"), str(path)], gpu=True,
                 timeout=timeout, env=e)
    return job.records(), job.elapsed


def group(c):
    if c["op"] in ("put", "get"):
        return f"{c['op']} {c['sym']}/{c['loc']} {c['peer']}"
    return c["op"]


def check(label, recs, batches, npes, env, elapsed=None):
    """no image differs; every call ran the kernel its modelled route names;
    returns {group: set of routes} over all PEs"""
    model, seen, wrong = ref.Mover(), {}, []
    for rec in recs:
        assert rec["failures"] == [], (label, rec["failures"][:10])
        count = {}
        for cases, kernels in zip(batches, rec["kernels"]):
            for c in cases:
                if str(c["id"]) not in kernels:
                    continue      # not in the case's active sets
                route = model.route(c, rec["pe"], npes, env)
                seen.setdefault(group(c), set()).add(route)
                count[route] = count.get(route, 0) + 1
                if kernels[str(c["id"])] != KERNEL_OF.get(route, "marker"):
                    wrong.append((rec["pe"], c, route, kernels[str(c["id"])]))
        print(f"datamove-routes | {label} | PE {rec['pe']} | " + " ".join(f"{k} {v}" for k, v in sorted(count.items())))
    if elapsed is not None:
        print(f"datamove-routes | {label} | {sum(len(b) for b in batches)} cases | job {elapsed:.1f} s")
    assert not wrong, (label, len(wrong), wrong[:5])
    return seen


KERNELS = {"copy", "shift", "noop"}
PUTGET_ROUTES = {
    "put dev/dev next": KERNELS, "put dev/host next": KERNELS, "put dev/page next": {"memcpy", "noop"},
    "put host/dev next": {"memcpy", "noop"}, "put host/page next": {"memmove", "noop"},
    "get dev/dev next": KERNELS, "get dev/hip next": KERNELS, "get dev/host next": {"memcpy", "noop"},
    "get dev/page next": {"memcpy", "noop"}, "get host/dev next": {"memcpy", "noop"},
    "get host/page next": {"memmove", "noop"},
    "put dev/dev self": KERNELS, "get dev/dev self": KERNELS, "put dev/dev same": {"noop"}, "get dev/dev same": {"noop"},
}


@pytest.mark.multipe
@pytest.mark.parametrize("npes", [2, 3])
def test_put_get_every_route(tmp_path, npes):
    """Every size at every phase pair between device-heap objects of
    neighbouring PEs, and the route sub-table for every other kind of local
    and symmetric memory; self-targeted calls at other and at the same
    address."""
    cases = ref.gpu_putget_tables()
    env = {"gpu": True, "fused_max": 65536, "scratch_chunk": CHUNK_3M}
    recs, elapsed = run_job(tmp_path, npes, {"batches": [cases]},
                            {"SHMEM_FUSED_MAX_BYTES": "64K", "SHMEM_DEVICE_SCRATCH_SIZE": "3M"})
    seen = check(f"put/get {npes} PEs", recs, [cases], npes, env, elapsed)
    assert seen == PUTGET_ROUTES, seen


def test_self_targeted_calls_and_every_entry_point_in_process(shm):
    """PE 0 of 1: self-targeted put / get (other addresses: the copy kernel;
    the same address: nothing), and each of the 24 contiguous put / get
    symbols at 0, 1 and 5 elements one element off a 16-byte boundary, between
    heap objects and from / into hipMalloc memory: the element size each
    symbol multiplies by, sizeof (long double) included."""
    cases = ref.gpu_inprocess_tables()
    import _datamove_worker
    t0 = time.perf_counter()
    rec = _datamove_worker.run(shm, {"batches": [cases]}, True)
    env = {"gpu": True, "fused_max": rec["fused_max"], "scratch_chunk": CHUNK_3M}
    seen = check("in process", [rec], [cases], 1, env, time.perf_counter() - t0)
    # one element off a 16-byte boundary on both sides: the phases agree
    assert seen == {"put dev/dev self": KERNELS, "get dev/dev self": KERNELS, "put dev/dev same": {"noop"},
                    "get dev/dev same": {"noop"}, "put dev/hip self": {"copy", "noop"},
                    "get dev/hip self": {"copy", "noop"}}, seen
    assert {c["fn"] for c in cases if c["nelems"] == 5} >= set(ref.ENTRY_POINTS)


SETTINGS = {
    "fused_64k": ({"SHMEM_FUSED_MAX_BYTES": "64K"}, 65536, DEFAULT_CHUNK, {"fused_pull", "copy", "shift", "none"}),
    "barrier_copy_barrier": ({"SHMEM_FUSED_MAX_BYTES": "0"}, 0, DEFAULT_CHUNK, {"copy", "shift", "none"}),
    "scratch_chunk": ({"SHMEM_FUSED_MAX_BYTES": "2M", "SHMEM_DEVICE_SCRATCH_SIZE": "3M"}, 2 << 20, CHUNK_3M,
                      {"fused_pull", "copy", "shift", "none"}),
}


def limit_checks(label, recs, cases, fused_max, chunk):
    """the two conditions of fused_pull_ok at their boundaries, straight from
    the records: at the limit fused_pull, one element above it not"""
    lim = min(fused_max, chunk)
    at = above = 0
    for c in cases:
        if c["op"] == "collect" or c["sym"] != "dev":
            continue
        for rec in recs:
            k = rec["kernels"][0].get(str(c["id"]))
            s = ref.my_set(c, rec["pe"])
            if k is None or s[2] < 2:
                continue
            es = c["bits"] // 8
            total = c["n"] * es * (s[2] if c["op"] == "fcollect" else 1)
            step = es * (s[2] if c["op"] == "fcollect" else 1)
            step = max(step, 8)
            if lim - step < total <= lim:
                at += 1
                assert k == "fused_pull", (label, c, rec["pe"], k)
            elif lim < total <= lim + step:
                above += 1
                assert k != "fused_pull", (label, c, rec["pe"], k)
    print(f"datamove-routes | {label} | at the limit of {lim} bytes: {at} calls fused_pull, one element above: {above} not")
    assert at > 0 and above > 0, (label, at, above)


@pytest.mark.multipe
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_collectives_four_pes(tmp_path, setting):
    """The collective tables on 4 PEs: every count at every pair of phases,
    every root, active set and kind of target. fused_64k: fused_pull up to
    SHMEM_FUSED_MAX_BYTES, the copy kernel one element above;
    barrier_copy_barrier: the limit at 0, the copy kernel between device
    barriers; scratch_chunk: one size below and one above a scratch chunk of
    1 MiB under a limit of 2 MiB. 4,096 bytes +- one element is the edge of
    one block's share of fused_pull."""
    env_vars, fused_max, chunk, routes = SETTINGS[setting]
    if setting == "scratch_chunk":
        cases = ref.collective_table(ref.Ids(), 4, fused_max, extra_bytes=CHUNK_PAIR, limits=False)
    else:
        cases = ref.collective_table(ref.Ids(), 4, 65536)
    recs, elapsed = run_job(tmp_path, 4, {"batches": [cases]}, env_vars)
    for rec in recs:
        assert rec["fused_max"] == fused_max, rec["fused_max"]
    env = {"gpu": True, "fused_max": fused_max, "scratch_chunk": chunk}
    seen = check(f"collectives {setting}", recs, [cases], 4, env, elapsed)
    for op in ("broadcast", "fcollect"):
        assert seen[op] == routes, (op, seen[op])
    assert seen["collect"] == {"copy", "shift", "host_wait"}, seen["collect"]
    if fused_max:
        limit_checks(setting, recs, cases, fused_max, chunk)


@pytest.mark.multipe
def test_collectives_eight_pes_and_a_second_trip(tmp_path):
    """The tables once on 8 PEs under the default limit of 2 MiB, then an
    fcollect sized from the grid the launch layer reports for a fused_pull of
    about 1 MiB: one element per member above 4,096 bytes x that grid, so
    every block makes a second trip."""
    fused_max = 2 << 20
    cases = ref.collective_table(ref.Ids(), 8, fused_max, limits=False)
    recs, elapsed = run_job(tmp_path, 8, {"batches": [cases], "second_trip": True}, {"SHMEM_FUSED_MAX_BYTES": "2M"})
    env = {"gpu": True, "fused_max": fused_max, "scratch_chunk": DEFAULT_CHUNK}
    seen = check("collectives 8 PEs", recs, [cases], 8, env, elapsed)
    assert seen["broadcast"] == {"fused_pull", "none"} and seen["fcollect"] == {"fused_pull", "copy", "shift", "none"}, seen
    trips = [rec["second_trip"] for rec in recs]
    print(f"datamove-routes | second trip | grid {trips[0]['grid']} x 4096 B < {trips[0]['total']} B | {trips[0]['kernels']}")
    for t in trips:
        assert t["kernels"] == ["fused_pull", "fused_pull"] and t["grid"] == trips[0]["grid"], t
        assert t["grid"][0] * 4096 < t["total"] <= fused_max, t


@pytest.mark.multipe
def test_mixed_sequence_four_pes(tmp_path):
    """100 calls drawn from all tables with a fixed seed, back to back in one
    batch with no barrier of the test's own between them, every image checked
    at the end: the pair counts of the signal region and the ordering of the
    copy-out behind fused_pull."""
    cases = ref.mixed_sequence(4, 65536)
    recs, elapsed = run_job(tmp_path, 4, {"batches": [cases]}, {"SHMEM_FUSED_MAX_BYTES": "64K"})
    env = {"gpu": True, "fused_max": 65536, "scratch_chunk": DEFAULT_CHUNK}
    seen = check("mixed sequence", recs, [cases], 4, env, elapsed)
    assert {"put", "get", "broadcast", "fcollect", "collect"} <= {g.split()[0] for g in seen}, seen
