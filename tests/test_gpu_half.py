"""GPU: the half and bfloat16 reductions (include/shmemx.h), bit for bit against
the model (tests/_half_ref.py) on the whole target, sentinel-filled tails and
guards included.

  the kernels directly   mi355_combine / mi355_combine_orders in this process
  multi-PE               the public calls on PE processes sharing the test GPU
                         (tests/_half_worker.py)
  torch                  to_all_tensors on caching-allocator tensors, heap_tensor
                         with the stream-ordered call
  the C example          examples/bf16_example.c at 2 PEs
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _half_ref as R
from _pes import launch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(ROOT, "osss-gasnet_amd", "lib")
pytestmark = pytest.mark.gpu

GUARD = 64            # bytes of sentinel on both sides of every target
SENT = 0xA5
LANES = 256           # kBlock
NSRC = [1, 2, 3, 8, 9]    # 9: past one launch's sources
SIZES = [0, 1, 7, 8, 9, 71, 4099]
# (name, target byte offset, source k's byte offset)
LAYOUTS = [
    ("aligned", 0, lambda k: 0),
    ("target off by one element", 2, lambda k: 0),
    ("all off by one element", 2, lambda k: 2),
    ("sources at three phases", 0, lambda k: (0, 4, 10)[k % 3]),
]


class Arena:
    """one device allocation carved into slots of `stride` bytes"""

    def __init__(self, shm, nbytes):
        self.shm, self.nbytes = shm, nbytes
        self.base = shm.malloc_device(nbytes)
        assert self.base and self.base % 256 == 0, self.base

    def slots(self, k, stride):
        assert k * stride <= self.nbytes, (k, stride)
        return [self.base + i * stride for i in range(k)]


@pytest.fixture(scope="module")
def arena(shm):
    a = Arena(shm, 160 << 20)
    yield a
    shm.sync()
    shm.free_device(a.base)


_INPUTS = {}


def inputs(dtype, nsrc, n):
    """sources and every member's expected fold, computed once per (type, count, size)"""
    key = (dtype, nsrc, n)
    if key not in _INPUTS:
        _INPUTS[key] = R.sources(dtype, nsrc, n, 9000 + 131 * nsrc + n % 1009)
    return _INPUTS[key]


def stride_for(n):
    return (2 * GUARD + 32 + 2 * n + 255) // 256 * 256


def upload_sources(shm, slots, srcs, src_off):
    ptrs = []
    for k, (slot, x) in enumerate(zip(slots, srcs)):
        p = slot + GUARD + src_off(k)
        if x.size:
            shm.put(p, x)
        ptrs.append(p)
    return ptrs


def poison(shm, slot, nbytes):
    shm.put(slot, np.full(nbytes, SENT, dtype=np.uint8))


def read_target(shm, slot, off, n, what, below_is_source=False):
    raw = shm.get(slot, GUARD + off + 2 * n + GUARD, np.uint8)
    lo = GUARD + off
    if not below_is_source:
        assert (raw[:lo] == SENT).all(), f"{what}: bytes below the target were written"
    assert (raw[lo + 2 * n:] == SENT).all(), f"{what}: bytes above the target were written"
    return raw[lo:lo + 2 * n].copy().view(np.uint16)


def assert_bits(got, want, what):
    if (got == want).all():
        return
    bad = np.nonzero(got != want)[0]
    i = int(bad[0])
    raise AssertionError(f"{what}: {bad.size} of {want.size} elements differ, first at {i}: "
                         f"got {int(got[i]):#06x}, want {int(want[i]):#06x}")


def combine_case(shm, arena, op, dtype, nsrc, n, layout, inplace):
    name, dst_off, src_off = layout
    what = f"combine {dtype} {op} nsrc {nsrc} n {n} {name}{' in place' if inplace else ''}"
    srcs = inputs(dtype, nsrc, n)
    stride = stride_for(n)
    slots = arena.slots(nsrc + 1, stride)
    for s in slots:
        poison(shm, s, stride)
    ptrs = upload_sources(shm, slots[:nsrc], srcs, src_off)
    if inplace:
        tslot, toff = slots[0], src_off(0)
    else:
        tslot, toff = slots[nsrc], dst_off
    rc = shm.combine(op, dtype, tslot + GUARD + toff, ptrs, n)
    assert rc == 0, (what, rc)
    shm.sync()
    got = read_target(shm, tslot, toff, n, what)
    assert_bits(got, R.left_fold(op, dtype, srcs), what)


def orders_case(shm, arena, op, dtype, nsrc, n, layout, inplace):
    name, dst_off, src_off = layout
    what = f"orders {dtype} {op} nsrc {nsrc} n {n} {name}{' in place' if inplace else ''}"
    srcs = inputs(dtype, nsrc, n)
    stride = stride_for(n)
    slots = arena.slots(2 * nsrc, stride)
    for s in slots:
        poison(shm, s, stride)
    ptrs = upload_sources(shm, slots[:nsrc], srcs, src_off)
    # in place: dsts[q] == srcs[q] (beyond 8 sources only one fold may be)
    alias = [inplace and (nsrc <= 8 or q == nsrc // 2) for q in range(nsrc)]
    where = [(slots[q], src_off(q)) if alias[q] else (slots[nsrc + q], dst_off) for q in range(nsrc)]
    dsts = [s + GUARD + o for s, o in where]
    rc = shm.combine_orders(op, dtype, dsts, ptrs, n)
    assert rc == 0, (what, rc)
    shm.sync()
    for q in range(nsrc):
        got = read_target(shm, where[q][0], where[q][1], n, f"{what} member {q}")
        assert_bits(got, R.fold(op, dtype, srcs, q), f"{what} member {q}")


@pytest.mark.parametrize("dtype", R.TYPES)
@pytest.mark.parametrize("op", R.OPS)
def test_combine_kernels(shm, arena, op, dtype):
    """mi355_combine: 1, 2, 3, 8 and 9 sources x n 0 .. 4099 x the four
    layouts, and in place (dst == srcs[0]) at every size"""
    for nsrc in NSRC:
        for n in SIZES:
            for layout in LAYOUTS:
                combine_case(shm, arena, op, dtype, nsrc, n, layout, False)
            combine_case(shm, arena, op, dtype, nsrc, n, LAYOUTS[0], True)
            combine_case(shm, arena, op, dtype, nsrc, n, LAYOUTS[2], True)


@pytest.mark.parametrize("dtype", R.TYPES)
@pytest.mark.parametrize("op", R.OPS)
def test_combine_orders_kernels(shm, arena, op, dtype):
    """mi355_combine_orders: every member's fold, the same matrix, and in
    place (dsts[q] == srcs[q])"""
    for nsrc in NSRC:
        for n in SIZES:
            for layout in LAYOUTS:
                orders_case(shm, arena, op, dtype, nsrc, n, layout, False)
            orders_case(shm, arena, op, dtype, nsrc, n, LAYOUTS[0], True)


def test_special_table_meets_itself(shm, arena):
    """the inputs the matrix above runs on: at n = 4099 every ordered pair of
    the 64 special patterns meets in sources 0 and 1, and the model's members
    differ (so an order mistake cannot pass)"""
    for dtype in R.TYPES:
        srcs = inputs(dtype, 3, 4099)
        assert len(set(zip(srcs[0][:4096].tolist(), srcs[1][:4096].tolist()))) == 4096
        assert (R.fold("sum", dtype, srcs, 0) != R.fold("sum", dtype, srcs, 2)).any()
        assert (R.fold("min", dtype, srcs[:2], 0) != R.fold("min", dtype, srcs[:2], 1)).any()


@pytest.mark.parametrize("dtype", R.TYPES)
@pytest.mark.parametrize("which", ["combine", "orders"])
def test_beyond_one_grid_pass(shm, arena, which, dtype):
    """Two sources, a size that takes the grid-stride loop past its first
    pass and ends on a partial vector: sized from the grid the library
    reports (more than two passes of the deepest unroll, 4 vectors per lane)."""
    cap_bytes = 36 << 20
    slots = arena.slots(4, cap_bytes + 4096)
    probe_n = cap_bytes // 2
    ptrs = [slots[0] + GUARD, slots[1] + GUARD]
    if which == "combine":
        assert shm.combine("sum", dtype, slots[2] + GUARD, ptrs, probe_n) == 0
    else:
        assert shm.combine_orders("sum", dtype, [slots[2] + GUARD, slots[3] + GUARD], ptrs, probe_n) == 0
    shm.sync()
    gx, _ = shm.last_launch_grid()
    assert gx > 0
    nvec = 9 * LANES * gx + LANES + 37
    n = nvec * 8 + 3
    assert nvec > 2 * 4 * LANES * gx and 2 * n + 2 * GUARD <= cap_bytes, (gx, n)
    srcs = inputs(dtype, 2, n)
    for s in slots:
        poison(shm, s, 2 * GUARD + 2 * n)
    ptrs = upload_sources(shm, slots[:2], srcs, lambda k: 0)
    if which == "combine":
        assert shm.combine("sum", dtype, slots[2] + GUARD, ptrs, n) == 0
        shm.sync()
        assert shm.last_launch_grid()[0] == gx
        assert_bits(read_target(shm, slots[2], 0, n, "fold"), R.left_fold("sum", dtype, srcs), "fold past one pass")
    else:
        assert shm.combine_orders("sum", dtype, [slots[2] + GUARD, slots[3] + GUARD], ptrs, n) == 0
        shm.sync()
        assert shm.last_launch_grid()[0] == gx
        # two members: a + b == b + a in every bit (canonical NaN), so both folds are the left fold
        for q in range(2):
            assert_bits(read_target(shm, slots[2 + q], 0, n, f"member {q}"), R.fold("sum", dtype, srcs, q),
                        f"every-member fold past one pass, member {q}")
    _INPUTS.pop((dtype, 2, n), None)


# ---------------------------------------------------------------------------
# multi-PE, the public calls
# ---------------------------------------------------------------------------
def run_pes(npes, cases, tmp_path, extra_env=None, timeout=300):
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"cases": cases}))
    env = {"SHMEM_DEVICE_HEAP_SIZE": "96M", "SHMEM_DEVICE_SCRATCH_SIZE": "384K",
           "SHMEM_SYMMETRIC_HEAP_SIZE": "64M", "SHMEM_BARRIER_TIMEOUT": "120", "SHMEM_PEER_ACQUIRE": "1"}
    env.update(extra_env or {})
    recs = launch(npes, [sys.executable, os.path.join(HERE, "_half_worker.py"), str(spec)], gpu=True,
                  timeout=timeout, env=env).records()
    for rec in recs:
        assert rec["checked"] == len(cases) and not rec["failures"], rec
    return recs


def case(cases, op, dtype, n, aset, mode="dev", **kw):
    c = {"id": len(cases), "op": op, "dtype": dtype, "n": n, "set": list(aset), "mode": mode,
         "seed": 5000 + len(cases)}
    c.update(kw)
    cases.append(c)
    return c


def public_matrix(npes):
    cases = []
    full = (0, 0, npes)
    for dtype in R.TYPES:
        for op in R.OPS:
            for n in (1, 257, 40000):
                for order in ("reference", "pe_start"):
                    case(cases, op, dtype, n, full, "dev", order=order)
                case(cases, op, dtype, n, full, "inplace")
                case(cases, op, dtype, n, full, "dev", algorithm="exact")
            if npes == 4:
                for n in (1, 257, 40000):
                    case(cases, op, dtype, n, (1, 1, 2), "dev")
                    case(cases, op, dtype, n, (1, 1, 2), "inplace", order="pe_start")
        case(cases, "sum", dtype, 40000, full, "host")            # shmem_malloc arrays: the staged path
        case(cases, "sum", dtype, 40000, full, "dev", stream=True)
        case(cases, "max", dtype, 257, full, "inplace", stream=True)
        case(cases, "sum", dtype, 0, full, "dev")
    return cases


@pytest.mark.multipe
@pytest.mark.parametrize("npes", [2, 3, 4])
def test_public_calls(tmp_path, npes):
    """Both types x four ops x n 1, 257, 40000 x both result orders, in place,
    EXACT, (4 PEs) the active set 1, 1, 2, host arrays, the stream-ordered
    call. Small calls must not take the fused kernel (it has no 16-bit float
    instantiations)."""
    cases = public_matrix(npes)
    for rec in run_pes(npes, cases, tmp_path):
        for cid, sched in rec["schedules"].items():
            assert "fused" not in sched, (cases[int(cid)], sched)
            if cases[int(cid)].get("algorithm") == "exact":
                assert sched == "exact", (cases[int(cid)], sched)


@pytest.mark.multipe
def test_rccl_request_falls_back_to_p2p(tmp_path):
    """SHMEM_REDUCE_ALGORITHM=rccl: RCCL has no per-step-rounded fold, so the
    call runs the P2P schedule and delivers the model's bits"""
    cases = []
    for dtype in R.TYPES:
        case(cases, "sum", dtype, 40000, (0, 0, 2), "dev")
    for rec in run_pes(2, cases, tmp_path, extra_env={"SHMEM_REDUCE_ALGORITHM": "rccl"}):
        for cid, sched in rec["schedules"].items():
            assert sched != "rccl", (cases[int(cid)], sched)


@pytest.mark.multipe
def test_debug_exchange(tmp_path):
    """SHMEM_DEBUG=1: the members compare their arguments first; matching calls pass"""
    cases = []
    for dtype in R.TYPES:
        case(cases, "prod", dtype, 257, (0, 0, 2), "dev")
        case(cases, "min", dtype, 257, (0, 0, 2), "dev", stream=True)
    run_pes(2, cases, tmp_path, extra_env={"SHMEM_DEBUG": "1"})


@pytest.mark.multipe
def test_torch_tensors(tmp_path):
    """to_all_tensors on torch.bfloat16 / torch.float16 tensors from the
    caching allocator (the members map each other's allocations), and
    heap_tensor(n, torch.bfloat16) with the stream-ordered sum"""
    cases = []
    for tdt in ("bfloat16", "float16"):
        for op in ("sum", "max"):
            cases.append({"id": len(cases), "torch": tdt, "op": op, "n": 4099, "seed": 7100 + len(cases)})
    cases.append({"id": len(cases), "torch": "bfloat16", "op": "sum", "n": 4099, "heap": True, "seed": 7200})
    cases.append({"id": len(cases), "torch": "float16", "op": "sum", "n": 4099, "heap": True, "seed": 7201})
    for rec in run_pes(2, cases, tmp_path, extra_env={"SHMEM_DEVICE_SCRATCH_SIZE": "3M"}):
        assert rec["external_map_opened"] > 0, rec
        for cid, sched in rec["schedules"].items():
            assert sched.startswith("mapped-"), (cases[int(cid)], sched)


# ---------------------------------------------------------------------------
# the C example
# ---------------------------------------------------------------------------
@pytest.mark.multipe
def test_c_example_two_pes(tmp_path):
    exe = str(tmp_path / "bf16_example")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "bf16_example.c"), "-L", LIBDIR, "-lshmem_reduce",
                    f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    env = dict(os.environ, SHMEM_DEVICE_HEAP_SIZE="16M", SHMEM_DEVICE_SCRATCH_SIZE="3M", SHMEM_BARRIER_TIMEOUT="120")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "oshrun"), "-np", "2", "--same-device", exe],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": PASS") == 2, r.stdout
