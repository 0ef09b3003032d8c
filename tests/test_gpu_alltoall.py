"""GPU: shmem_alltoall32/64, shmem_alltoalls32/64 and the strided pull kernel.

Expected results are the specification's formula, computed here with numpy
(m, i: indices in the active set):
    target_on_m[(i*nelems + k) * dst] = source_on_i[(m*nelems + k) * sst]
Every target is pre-filled with -7; a test compares the WHOLE target read
back, so the gaps between strided elements and the elements past the last
block must still hold the sentinel.

The kernel tests run in one process of their own on torch-allocated buffers
(tests/_strided_pull_worker.py); the collective tests start PE processes
sharing the test GPU (tests/alltoall_worker.py), as tests/test_gpu_multipe.py
does.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _pes import launch
from alltoall_worker import SENTINEL, source_of
from test_gpu_multipe import members

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(ROOT, "osss-gasnet_amd", "lib")
pytestmark = pytest.mark.gpu

STRIDES_HOST_TEST = [(1, 1), (1, 3), (3, 1), (2, 5)]


# ---------------------------------------------------------------------------
# the kernel, on torch-allocated buffers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernel_results():
    """tests/_strided_pull_worker.py, run once: a process of its own that
    loads the library beside torch WITHOUT shmem_init. (This pytest process
    holds the session's initialised library, whose exit handler finalizes it;
    with torch's GPU context in the same process the interpreter aborted in
    free() at exit, after every check had passed. The kernel layer needs no
    runtime, so its checks run where only torch owns the GPU's teardown.)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_strided_pull_worker.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("nseg", [1, 3, 64])
@pytest.mark.parametrize("es", [4, 8])
def test_strided_pull_kernel(kernel_results, es, nseg):
    """Strides (1,1) (1,2) (2,1) (1,3) (3,1) (2,5) (7,7) (33,1) (1,33) x
    nelems 0, 1, 3, 5, 257, 4099, bases one element off alignment."""
    failures = kernel_results["matrix"][f"{es}-{nseg}"]
    assert not failures, failures


def passes_rule(gx, nelems):
    """at least two full grid passes and a partial one, whatever the kernel's
    per-lane unroll (4 at most); from the grid the library reported"""
    return gx > 0 and nelems > 2 * 4 * 256 * gx


@pytest.mark.parametrize("es,nseg", [(4, 64), (8, 64), (8, 1)])
def test_strided_pull_kernel_past_one_pass(kernel_results, es, nseg):
    """Strides (1,2) (1,3) (2,1) (3,1) (2,3) (3,2) at 9 * 1024 * gx + 1024 + 37
    elements per segment, gx read back from the library: every block takes
    several trips round its tile loop and the last one is partial."""
    failures = kernel_results["passes"][f"{es}-{nseg}"]
    info = kernel_results["passes_info"][f"{es}-{nseg}"]
    print(f"grid-pass | strided_pull es {es} x{nseg} | (strides, gx, gy, nelems) {info}")
    assert not failures, failures
    assert len(info) == 6 and all(passes_rule(gx, n) and gy == nseg for _, gx, gy, n in info), info


def test_strided_pull_rejects_bad_arguments(kernel_results):
    rec = kernel_results["bad_arguments"]
    assert all(rc != 0 for rc in rec["rcs"]) and rec["untouched"], rec


def test_strided_pull_offsets_past_4_gib(kernel_results):
    rec = kernel_results["past_4_gib"]
    assert rec["rcs"] == [0, 0] and rec["last_byte_offset"] > 2**32, rec
    assert rec["gathered"] == [SENTINEL] + rec["vals"] + [SENTINEL] * 4, rec
    assert rec["scattered"] == rec["vals"] and rec["source_after"] == rec["vals"], rec


# ---------------------------------------------------------------------------
# the collectives, on PE processes sharing the GPU
# ---------------------------------------------------------------------------
def run_a2a(npes, cases, tmp_path, extra_env=None, timeout=300, offset=0):
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"cases": cases, "offset": offset}))
    env = {"SHMEM_DEVICE_HEAP_SIZE": "96M", "SHMEM_DEVICE_SCRATCH_SIZE": "384K",
           "SHMEM_SYMMETRIC_HEAP_SIZE": "64M", "SHMEM_BARRIER_TIMEOUT": "120", "SHMEM_PEER_ACQUIRE": "1"}
    env.update(extra_env or {})
    launch(npes, [sys.executable, os.path.join(HERE, "alltoall_worker.py"), str(spec), str(tmp_path)], gpu=True,
           timeout=timeout, env=env).ok()
    return [np.load(tmp_path / f"pe{pe}.npz") for pe in range(npes)]


def case(cid, kind, bits, n, sets, dst=1, sst=1, target="device", source="device", seed=None, report_grid=False):
    big = max(s[2] for s in sets)
    if kind in ("alltoall", "alltoalls"):
        slen = (big * n - 1) * sst + 1 if n else 0
        tlen = ((big * n - 1) * dst + 1 if n else 0) + 5
    elif kind == "fcollect":
        slen, tlen = n, big * n + 5
    else:
        slen, tlen = n, n + 5
    return {"id": cid, "kind": kind, "bits": bits, "n": n, "sets": sets, "dst": dst, "sst": sst, "target": target,
            "source": source, "seed": 5000 + cid if seed is None else seed, "slen": slen, "tlen": tlen,
            "report_grid": report_grid}


@functools.lru_cache(maxsize=None)
def cached_source(pe, n, bits, seed):
    x = source_of(pe, n, bits, seed)
    x.setflags(write=False)
    return x


def expected(c, pe):
    """what PE pe's target holds after case c (None: pe is in none of its sets)"""
    for s in c["sets"]:
        mem = members(*s)
        if pe not in mem:
            continue
        n, bits = c["n"], c["bits"]
        dt = np.int32 if bits == 32 else np.int64
        want = np.full(c["tlen"], SENTINEL, dtype=dt)
        m = mem.index(pe)
        k = np.arange(n)
        srcs = [cached_source(q, c["slen"], bits, c["seed"]) for q in mem]
        if c["kind"] in ("alltoall", "alltoalls"):
            for i, x in enumerate(srcs):
                want[(i * n + k) * c["dst"]] = x[(m * n + k) * c["sst"]]
        elif c["kind"] == "fcollect":
            want[:len(mem) * n] = np.concatenate(srcs) if n else []
        else:
            want[:n] = np.sum(srcs, axis=0, dtype=np.int32)
        return want
    return None


def check(results, cases):
    for c in cases:
        for pe in range(len(results)):
            want = expected(c, pe)
            if want is None:
                assert str(c["id"]) not in results[pe]
                continue
            got = results[pe][str(c["id"])]
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (f"case {c} PE {pe}: {bad.size} elements differ, first at {bad[0]}: "
                                   f"got {got[bad[0]]}, want {want[bad[0]]}")


FOUR_SETS = [[[0, 0, 4]], [[0, 1, 2], [1, 1, 2]], [[1, 0, 3]], [[2, 0, 1], [3, 0, 1]]]


@pytest.mark.multipe
@pytest.mark.parametrize("fused", ["default", "0"], ids=["fused", "copy-kernel"])
def test_alltoall_four_pes(tmp_path, fused, kernel_results):
    """Small contiguous calls run as one fused pull launch by default;
    SHMEM_FUSED_MAX_BYTES=0 sends every one through barrier + copy kernel +
    barrier. The strided calls run barrier + strided kernel + barrier either
    way (a host target: staged through scratch, 384 KiB here, so the larger
    cases take several passes). With the default thresholds, two more strided
    calls into device memory large enough for every block of the 4-segment
    launch to pass several times over its share (sized from the grid the
    kernel process saw for 4 segments; each PE reports the grid it launched
    and the rule is asserted from that)."""
    cases, cid = [], 0
    pairs = []
    for bits in (32, 64):
        for n in (0, 1, 5, 257, 40000):
            for sets in FOUR_SETS:
                for tk in ("device", "host", "pageable", "mixed"):
                    cases.append(case(cid, "alltoall", bits, n, sets, target=tk)); cid += 1
        for dst, sst in STRIDES_HOST_TEST + [(33, 2)]:
            for tk in ("device", "pageable"):
                for n in (0, 1, 5, 257, 4099):
                    cases.append(case(cid, "alltoalls", bits, n, [[0, 0, 4]], dst, sst, target=tk)); cid += 1
                for sets in FOUR_SETS[1:]:
                    cases.append(case(cid, "alltoalls", bits, 257, sets, dst, sst, target=tk)); cid += 1
        # a block larger than the scratch chunk, into host memory
        cases.append(case(cid, "alltoalls", bits, 40000, [[0, 0, 4]], 2, 3, target="pageable")); cid += 1
        cases.append(case(cid, "alltoalls", bits, 40000, [[0, 0, 4]], 3, 1, target="host")); cid += 1
        # alltoalls with strides (1,1) is alltoall: the same bytes from the same sources
        for n in (5, 40000):
            for tk in ("device", "mixed"):
                a = case(cid, "alltoall", bits, n, [[0, 0, 4]], target=tk, seed=77 + n); cid += 1
                b = case(cid, "alltoalls", bits, n, [[0, 0, 4]], 1, 1, target=tk, seed=77 + n); cid += 1
                cases += [a, b]
                pairs.append((a["id"], b["id"]))
    extra = {} if fused == "default" else {"SHMEM_FUSED_MAX_BYTES": fused}
    large = []
    if fused == "default":   # the strided calls take the same path either way: once is enough
        for dst, sst in ((2, 3), (1, 3)):
            gx = kernel_results["grid_of_four_segments"][f"{dst},{sst}"]
            large.append(case(cid, "alltoalls", 32, 9 * 1024 * gx + 1024 + 37, [[0, 0, 4]], dst, sst,
                              report_grid=True, seed=4242)); cid += 1   # one seed: the PEs' sources are shared
        cases += large
        heap = sum(max(c[k] * c["bits"] // 8 for c in cases) for k in ("slen", "tlen"))
        extra["SHMEM_DEVICE_HEAP_SIZE"] = f"{heap // 2**20 + 32}M"
    res = run_a2a(4, cases, tmp_path, extra_env=extra)
    check(res, cases)
    for c in large:
        for pe in range(4):
            gx, gy = (int(v) for v in res[pe][f"grid{c['id']}"])
            print(f"grid-pass | alltoalls32 ({c['dst']},{c['sst']}) PE {pe} | {gx} x {gy} | nelems {c['n']}")
            assert gy == 4 and passes_rule(gx, c["n"]), (c["id"], pe, gx, gy, c["n"])
    cached_source.cache_clear()
    for a, b in pairs:
        for pe in range(4):
            assert (res[pe][str(a)] == res[pe][str(b)]).all()


@pytest.mark.multipe
def test_closing_device_barrier_leaves_the_strided_launch_on_record(tmp_path):
    """The device barrier launches bare: it records nothing. After a strided
    alltoalls32 on 2 PEs -- device barrier, strided kernel, device barrier --
    the kernel layer's last launch is still the strided kernel, name and grid:
    5,000 elements per block at 1,024 per kernel block are 5 blocks in x (far
    below the cap of 8 per CU), one row per member in y. (Had the barrier
    recorded itself, the all-to-all tests' pass rule above would read 1 x 1.)"""
    c = case(0, "alltoalls", 32, 5000, [[0, 0, 2]], 2, 3, report_grid=True)
    res = run_a2a(2, [c], tmp_path)
    check(res, [c])
    for pe in range(2):
        kernel, grid = str(res[pe]["kernel0"][0]), tuple(int(v) for v in res[pe]["grid0"])
        print(f"barrier-record | alltoalls32 (2,3) PE {pe} | {kernel[:70]} | {grid}")
        assert "strided_pull" in kernel and "device_barrier" not in kernel, (pe, kernel)
        assert grid == (5, 2), (pe, grid)
    cached_source.cache_clear()


@pytest.mark.multipe
def test_alltoall_four_pes_off_alignment(tmp_path):
    """Source and target 4 bytes into their allocations: the vector sides
    peel a head, the copy kernel takes its co-aligned path."""
    cases, cid = [], 0
    for dst, sst in [(1, 1), (1, 3), (3, 1), (2, 5)]:
        for n in (5, 257, 4099):
            for tk in ("device", "pageable"):
                cases.append(case(cid, "alltoalls", 32, n, [[0, 0, 4]], dst, sst, target=tk)); cid += 1
    res = run_a2a(4, cases, tmp_path, offset=4)
    check(res, cases)


@pytest.mark.multipe
def test_alltoall_eight_pes(tmp_path):
    """8 PE processes: alltoall64 below and above the fused limit, and the
    strided form over two interleaved sets of 4."""
    cases = [case(0, "alltoall", 64, 100, [[0, 0, 8]]),
             case(1, "alltoall", 64, 40000, [[0, 0, 8]]),
             case(2, "alltoalls", 32, 1000, [[0, 1, 4], [1, 1, 4]], 2, 3),
             case(3, "alltoall", 32, 7, [[0, 1, 4], [1, 1, 4]], target="mixed")]
    res = run_a2a(8, cases, tmp_path)
    check(res, cases)


@pytest.mark.multipe
def test_alltoall_host_heap_source_into_device_target(tmp_path):
    """3 PEs, sources in shmem_malloc's host heap, targets in device memory
    (copies per block; the strided form packs on the host and spreads with
    the strided kernel), and into pageable memory (host loops)."""
    cases, cid = [], 0
    for bits in (32, 64):
        for n in (0, 5, 300):
            for tk in ("device", "pageable"):
                cases.append(case(cid, "alltoall", bits, n, [[0, 0, 3]], source="host", target=tk)); cid += 1
                for dst, sst in [(1, 3), (3, 1), (2, 5)]:
                    cases.append(case(cid, "alltoalls", bits, n, [[0, 0, 3]], dst, sst, source="host", target=tk))
                    cid += 1
        cases.append(case(cid, "alltoalls", bits, 33, [[1, 0, 2]], 2, 2, source="host")); cid += 1
        # more than the 128 KiB scratch chunk per block
        cases.append(case(cid, "alltoalls", bits, 40000, [[0, 0, 3]], 2, 3, source="host")); cid += 1
    res = run_a2a(3, cases, tmp_path)
    check(res, cases)


@pytest.mark.multipe
def test_alltoall_in_a_random_sequence_of_collectives(tmp_path):
    """100 back-to-back calls on 4 PEs: alltoall, alltoalls, fcollect and int
    sum reductions over random sets and sizes. Every kind advances the same
    per-pair barrier counts, so a miscount deadlocks (inside the barrier
    timeout) or lets a PE read a source too early."""
    rng = np.random.default_rng(20240607)
    cases = []
    set_choices = [[[0, 0, 4]], [[0, 1, 2], [1, 1, 2]], [[1, 0, 3]], [[0, 0, 2], [2, 0, 2]], [[0, 0, 3]]]
    for cid in range(100):
        kind = str(rng.choice(["alltoall", "alltoalls", "fcollect", "sum"]))
        sets = set_choices[int(rng.integers(len(set_choices)))]
        bits = 32 if kind == "sum" else int(rng.choice([32, 64]))
        n = int(rng.choice([0, 1, 50, 900, 20000])) if kind != "sum" else int(rng.choice([1, 50, 900, 20000]))
        dst, sst = (int(rng.integers(1, 4)), int(rng.integers(1, 4))) if kind == "alltoalls" else (1, 1)
        tk = str(rng.choice(["device", "device", "mixed", "host"])) if kind in ("alltoall", "alltoalls") else "device"
        cases.append(case(cid, kind, bits, n, sets, dst, sst, target=tk))
    res = run_a2a(4, cases, tmp_path)
    check(res, cases)


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
    exe = build_c(tmp_path, os.path.join(ROOT, "examples", "alltoall_example.c"), "alltoall_example")
    r = oshrun(exe, 2)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": PASS") == 2, r.stdout


@pytest.mark.multipe
def test_fortran_style_caller_two_pes(tmp_path):
    """shmem_alltoalls64_ with every argument by reference and an INTEGER pSync"""
    exe = build_c(tmp_path, os.path.join(HERE, "native", "alltoalls_fortran_stub.c"), "alltoalls_fortran_stub")
    r = oshrun(exe, 2)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": PASS") == 2, r.stdout


@pytest.mark.multipe
def test_alltoall_tensors_two_pes():
    """Shmem.alltoall_tensors on float32 and int64 tensors against torch
    indexing of the inputs (tests/_alltoall_torch_worker.py)."""
    env = dict(SHMEM_DEVICE_HEAP_SIZE="64M", SHMEM_DEVICE_SCRATCH_SIZE="3M", SHMEM_BARRIER_TIMEOUT="120",
               SHMEM_PEER_ACQUIRE="1")
    for rec in launch(2, [sys.executable, os.path.join(HERE, "_alltoall_torch_worker.py")], gpu=True, timeout=120,
                      env=env).records():
        assert rec["ok"] and rec["checked"] == 5, rec
