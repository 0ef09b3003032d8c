"""CPU: remote atomics, shmem_wait_until and locks without a GPU.

The ABI (strong pshmem_ names, weak shmem_ names, the Fortran wrappers pinned
in tests/golden/fortran_atomic_names.txt, the prototypes against the
reference's headers where its tree is present), the accumulate kernel's
launch plan, and the host-heap paths on PE processes under
SHMEM_BOOTSTRAP_ONLY=1 (tests/atomic_worker.py: the same semantic tests the
GPU suite runs on the device heap). The library's wait limit is 20 s here, so
a broken wait ends as a named failure of a child, never as a hang.
"""
import json
import os
import re
import subprocess
import sys

import pytest

import shmem_reduce
import test_bootstrap
from _pes import launch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(ROOT, "osss-gasnet_amd", "lib")
REFERENCE = "/root/reference/src"

ALL5 = {"int": "int", "long": "long", "longlong": "long long", "float": "float", "double": "double"}
INT3 = {k: ALL5[k] for k in ("int", "long", "longlong")}
WAIT4 = {"short": "short", "int": "int", "long": "long", "longlong": "long long"}
C_NAMES = ([f"shmem_{t}_{op}" for op in ("swap", "fetch", "set") for t in ALL5]
           + [f"shmem_{t}_{op}" for op in ("cswap", "fadd", "finc", "add", "inc") for t in INT3]
           + [f"shmem_{t}_{op}" for op in ("wait", "wait_until") for t in WAIT4]
           + ["shmem_wait", "shmem_wait_until", "shmem_set_lock", "shmem_clear_lock", "shmem_test_lock",
              "shmem_fence", "shmem_quiet"])
SEMANTIC = ["tickets", "fadd_chain", "wrap", "swap", "cswap_election", "neighbours", "locks"]


def _nm():
    out = subprocess.check_output(["nm", "-D", "--defined-only", shmem_reduce.LIB_PATH], text=True)
    return {line.split()[-1]: line.split()[-2] for line in out.splitlines() if len(line.split()) >= 2}


def test_symbols_strong_and_weak():
    assert len(C_NAMES) == 15 + 15 + 8 + 7
    kinds = _nm()
    for n in C_NAMES:
        assert kinds.get("p" + n) == "T", "p" + n
        assert kinds.get(n) == "W", n
    for t in ALL5:
        assert kinds.get(f"shmemx_{t}_atomic_add_v") == "T", t
    for n in ("mi355_amo", "mi355_atomic_add_v", "mi355_atomic_add_v_plan"):
        assert kinds.get(n) == "T", n


def test_fortran_names_equal_the_pinned_list():
    """the wrappers the reference's src/fortran/fortran.c defines for swap,
    cswap, fadd, finc, add, inc, fetch, set, wait, wait_until, locks, fence
    and quiet: 34 names, each weak over its strong p-name"""
    pinned = open(os.path.join(HERE, "golden", "fortran_atomic_names.txt")).read().split()
    assert len(pinned) == 34 and pinned == sorted(set(pinned))
    kinds = _nm()
    fam = re.compile(r"^shmem_(\w+_)?(swap|cswap|fadd|finc|add|inc|fetch|set|wait|wait_until|set_lock|clear_lock|"
                     r"test_lock|fence|quiet)_$")
    got = sorted(n for n in kinds if fam.match(n))
    assert got == pinned
    for n in pinned:
        assert kinds[n] == "W" and kinds.get("p" + n) == "T", n


def _prototypes(text, prefix):
    """{name: prototype with single spaces} of the atomic / wait / lock / fence declarations in a header"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fam = (r"(?:\w+_)?(?:swap|cswap|fadd|finc|add|inc|fetch|set|wait|wait_until)|set_lock|clear_lock|test_lock|"
           r"fence|quiet")
    out = {}
    for m in re.finditer(r"^[ \t]*((?:void|int|long|float|double)[\w \t]*?\b" + prefix + r"shmem_(?:" + fam +
                         r")\s*\([^;{]*?\)[^;{]*?);", text, flags=re.M):
        proto = " ".join(m.group(1).split())
        name = re.search(r"\b(" + prefix + r"shmem_\w+)\s*\(", proto).group(1)
        out.setdefault(name, proto)
    return out


def test_prototypes_match_the_reference_and_compile(tmp_path):
    """Every new prototype, assigned to a function pointer of its stated type;
    the generic macros select the typed calls; and, where the reference tree
    is present, the prototypes equal its headers' text up to white space."""
    lines = ["#include <stddef.h>", '#include "shmem.h"', '#include "pshmem.h"', '#include "shmemx.h"',
             '#include "shmem_fortran.h"', '#include "mi355_reduce.h"']
    k = 0
    for p in ("", "p"):
        for t, ct in ALL5.items():
            lines.append(f"{ct} (*f{k}) ({ct} *, {ct}, int) = {p}shmem_{t}_swap;"); k += 1
            lines.append(f"{ct} (*f{k}) (const {ct} *, int) = {p}shmem_{t}_fetch;"); k += 1
            lines.append(f"void (*f{k}) ({ct} *, {ct}, int) = {p}shmem_{t}_set;"); k += 1
        for t, ct in INT3.items():
            lines.append(f"{ct} (*f{k}) ({ct} *, {ct}, {ct}, int) = {p}shmem_{t}_cswap;"); k += 1
            lines.append(f"{ct} (*f{k}) ({ct} *, {ct}, int) = {p}shmem_{t}_fadd;"); k += 1
            lines.append(f"{ct} (*f{k}) ({ct} *, int) = {p}shmem_{t}_finc;"); k += 1
            lines.append(f"void (*f{k}) ({ct} *, {ct}, int) = {p}shmem_{t}_add;"); k += 1
            lines.append(f"void (*f{k}) ({ct} *, int) = {p}shmem_{t}_inc;"); k += 1
        for t, ct in WAIT4.items():
            lines.append(f"void (*f{k}) (volatile {ct} *, int, {ct}) = {p}shmem_{t}_wait_until;"); k += 1
            lines.append(f"void (*f{k}) (volatile {ct} *, {ct}) = {p}shmem_{t}_wait;"); k += 1
        lines.append(f"void (*f{k}) (volatile long *) = {p}shmem_set_lock;"); k += 1
        lines.append(f"void (*f{k}) (volatile long *) = {p}shmem_clear_lock;"); k += 1
        lines.append(f"int (*f{k}) (volatile long *) = {p}shmem_test_lock;"); k += 1
        lines.append(f"void (*f{k}) (void) = {p}shmem_fence;"); k += 1
    assert k == 2 * (15 + 15 + 8 + 4)
    for t, ct in ALL5.items():
        lines.append(f"void (*x{t}) ({ct} *, const {ct} *, size_t, int) = shmemx_{t}_atomic_add_v;")
    lines += ["int (*fi) (int *, int *) = shmem_int4_finc_;", "long (*fs) (long *, long *, int *) = pshmem_int8_swap_;",
              "void (*fw) (int *, int *, int *) = shmem_wait_until_;", "int (*ft) (long *) = shmem_test_lock_;",
              "int (*amo) (int, int, void *, unsigned long long, unsigned long long, unsigned long long *, void *) = "
              "mi355_amo;",
              "int (*addv) (int, void *, const void *, size_t, void *) = mi355_atomic_add_v;",
              "int cmp[6] = {SHMEM_CMP_EQ, SHMEM_CMP_NE, SHMEM_CMP_GT, SHMEM_CMP_LE, SHMEM_CMP_LT, _SHMEM_CMP_GE};",
              "_Static_assert (SHMEM_CMP_EQ == 0 && SHMEM_CMP_GE == 5, \"the reference's values\");",
              "double generic (long *l, int *i, long long *q, float *f, double *d, short *s) {",
              "  double r = shmem_swap (f, 1.0f, 0); r += shmem_cswap (q, 1LL, 2LL, 0); r += shmem_fadd (l, 1L, 0);",
              "  r += shmem_finc (i, 0); shmem_add (q, 1LL, 0); shmem_inc (l, 0); r += shmem_fetch (d, 0);",
              "  shmem_set (d, 1.0, 0); shmem_wait (s, (short) 0); shmem_wait_until (i, SHMEM_CMP_GT, 0); return r; }"]
    src = tmp_path / "atomics.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "atomics.o")])
    if not os.path.isfile(os.path.join(REFERENCE, "shmem.h")):
        return   # no reference tree here: nothing to compare with
    for header, prefix in (("shmem.h", ""), ("pshmem.h", "p")):
        ours = _prototypes(open(os.path.join(ROOT, "include", header)).read(), prefix)
        theirs = _prototypes(open(os.path.join(REFERENCE, header)).read(), prefix)
        new = [n for n in ours if n != prefix + "shmem_quiet"]
        assert len(new) == 42, (header, sorted(new))
        for n in new:
            assert ours[n] == theirs.get(n), (header, n, ours[n], theirs.get(n))


def test_accumulate_plan():
    """grids at n = 0, 1, one wave, one block +- 1 and the first size beyond
    one grid pass; 256 lanes x 4 elements per block pass, 8 blocks per CU"""
    s = shmem_reduce.Shmem()
    per_block = 256 * 4
    for cus in (1, 4, 256):
        cap = 8 * cus
        assert s.atomic_add_v_plan(0, cus) == (0, 0)
        for n, grid in ((1, 1), (64, 1), (per_block - 1, 1), (per_block, 1), (per_block + 1, 2),
                        (cap * per_block - 1, cap), (cap * per_block, cap), (cap * per_block + 1, cap),
                        (3 * cap * per_block + 5, cap), (1 << 40, cap)):
            assert s.atomic_add_v_plan(n, cus) == (min(grid, cap), min(grid, cap) * per_block), (cus, n)
    assert s.atomic_add_v_plan(5000, 0) == (5, 5 * per_block)   # cus <= 0 counts as one CU


def run_workers(npes, heap, tests, tmp_path, gpu=False, timeout=120):
    d = tmp_path / f"job{npes}"
    d.mkdir()
    spec = d / "spec.json"
    spec.write_text(json.dumps({"heap": heap, "tests": tests, "dir": str(d)}))
    env = dict(SHMEM_BARRIER_TIMEOUT="60", SHMEM_WAIT_TIMEOUT="20")
    if gpu:
        env.update({"SHMEM_DEVICE_HEAP_SIZE": "160M", "SHMEM_DEVICE_SCRATCH_SIZE": "3M",
                    "SHMEM_SYMMETRIC_HEAP_SIZE": "16M", "SHMEM_PEER_ACQUIRE": "1"})
    for rec in launch(npes, [sys.executable, os.path.join(HERE, "atomic_worker.py"), str(spec)], gpu=gpu,
                      timeout=timeout, env=env).records():
        assert rec["checked"] == tests and not rec["failures"], rec


@pytest.mark.parametrize("npes", [1, 2, 4, 7])
def test_host_heap_semantics(tmp_path, npes):
    """tickets, the fadd chain, wrap-around, swap tokens, the cswap election,
    neighbours of a 32-bit target at 4 mod 8, and the lock-protected counter
    (64 rounds per PE) with test_lock, for int, long and long long"""
    run_workers(npes, "host", SEMANTIC, tmp_path)


def test_host_heap_wait_until(tmp_path):
    """six comparisons x short, int, long, long long, released by shmem_<T>_p
    and by an atomic set, 50 ms after the waiter went in"""
    run_workers(2, "host", ["wait_until"], tmp_path)


def build_c(tmp_path, source, name):
    exe = str(tmp_path / name)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), source, "-L", LIBDIR,
                    "-lshmem_reduce", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    return exe


def run_c_host(exe, npes):
    job = launch(npes, [exe, "host"], gpu=False, timeout=60,
                 env=dict(SHMEM_BARRIER_TIMEOUT="60", SHMEM_WAIT_TIMEOUT="20"))
    for rc, out in zip(job.rc, job.out):
        assert rc == 0 and ": PASS" in out, out


@pytest.mark.parametrize("npes", [1, 3])
def test_float_and_double_move_bit_patterns(tmp_path, npes):
    """set, fetch and swap carry a signalling-NaN payload, -0.0 and a
    subnormal bit for bit; the float sits at 4 mod 8 between sentinels"""
    run_c_host(build_c(tmp_path, os.path.join(HERE, "native", "atomic_bits.c"), "atomic_bits"), npes)


def test_c_example_on_the_host_heap(tmp_path):
    """examples/atomic_example.c (shmem_int_finc, shmem_set_lock,
    shmem_long_wait_until) on 4 PEs without a GPU"""
    run_c_host(build_c(tmp_path, os.path.join(ROOT, "examples", "atomic_example.c"), "atomic_example"), 4)


def _aborts(tmp_path, call, name, words):
    body = f"""
    p = shm.malloc(256); x = (ctypes.c_long * 4)()
    {call}
    print('returned')
    """
    rc, out = test_bootstrap.spawn(1, body, tmp_path, extra={"SHMEM_WAIT_TIMEOUT": "20"})[0]
    assert rc != 0 and "returned" not in out, out
    assert name in out and words in out, out


def test_target_outside_the_heaps_aborts_by_name(tmp_path):
    _aborts(tmp_path, "shm.atomic('fadd', 'long', ctypes.addressof(x), 0, value=1)", "shmem_long_fadd",
            "neither symmetric heap")


def test_pe_out_of_range_aborts_by_name(tmp_path):
    _aborts(tmp_path, "shm.atomic('swap', 'int', p, 1, value=1)", "shmem_int_swap", "outside 0..0")


def test_wait_on_a_private_variable_aborts_by_name(tmp_path):
    _aborts(tmp_path, "shm.wait_until('long', ctypes.addressof(x), 'ne', 0)", "shmem_long_wait_until",
            "neither symmetric heap")


def test_lock_outside_the_heaps_aborts_by_name(tmp_path):
    _aborts(tmp_path, "shm.set_lock(ctypes.addressof(x))", "shmem_set_lock", "neither symmetric heap")


def test_misaligned_target_aborts_by_name(tmp_path):
    _aborts(tmp_path, "shm.atomic('fetch', 'long', p + 4, 0)", "shmem_long_fetch", "not aligned")


def test_accumulate_on_the_host_heap(tmp_path):
    """shmemx_<T>_atomic_add_v with a host-heap target: 3 PEs add into PE 2's
    array at once; integers wrap, float and double sums of small integers
    are exact in any order. The arithmetic of the float and double add
    (rounding, underflow, overflow, zeros, Inf, NaN) is
    tests/test_fp_add_cases.py's and test_accumulate_float_semantics', rounded
    sums under contention test_accumulate_arrival_orders'."""
    body = """
    import numpy as np
    n = 3001
    for name, dt in (('int', np.int32), ('long', np.int64), ('longlong', np.int64), ('float', np.float32),
                     ('double', np.float64)):
        rng = np.random.default_rng(11)
        if np.issubdtype(dt, np.integer):
            base = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, n, dtype=dt, endpoint=True)
        else:
            base = rng.integers(-64, 64, n, endpoint=True).astype(dt)
        t = shm.malloc(n * base.itemsize)
        T = np.ctypeslib.as_array(ctypes.cast(t, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,))
        T[:] = base
        mine = (base * dt(me + 2)).astype(dt)
        shm.barrier_all()
        shm.atomic_add_v(name, t + base.itemsize, mine[1:].ctypes.data, n - 1, npes - 1)
        shm.barrier_all()
        want = base.copy()
        if me == npes - 1:
            for pe in range(npes):
                want[1:] = (want[1:] + (base * dt(pe + 2)).astype(dt)[1:]).astype(dt)
        assert (T.view(np.uint8) == want.view(np.uint8)).all(), name
        shm.barrier_all()
        shm.free(t)
    shm.finalize()
    print('ok')
    """
    for rc, out in test_bootstrap.spawn(3, body, tmp_path):
        assert rc == 0 and "ok" in out, out


def test_accumulate_float_semantics(tmp_path):
    """worker test accumulate_fp on the host heap: PE 0 alone adds the operand
    table of tests/_fp_add_cases.py into PE 1's target, from a pageable source
    and from one in the host heap; every non-NaN row against the exact model
    in every bit"""
    run_workers(2, "host", ["accumulate_fp"], tmp_path)


@pytest.mark.parametrize("npes", [2, 4])
def test_accumulate_arrival_orders(tmp_path, npes):
    """worker test accumulate_orders on the host heap: full-mantissa arrays
    from every PE at once; every element is the rounded sum in one of the
    npes! arrival orders"""
    run_workers(npes, "host", ["accumulate_orders"], tmp_path)
