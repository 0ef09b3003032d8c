"""GPU: remote atomics, waits, locks and the atomic accumulate on the device heap.

Multi-PE: tests/atomic_worker.py, the semantic tests of tests/test_atomic_cpu.py
repeated on device-heap objects by PE processes sharing the test GPU, plus a
device-heap and a host-heap counter updated alternately and the accumulate of
every PE's array into one PE's. The library's wait limit is 20 s in the
children: a broken wait ends as a named failure.

In-process (PE 0 of 1): the two kernels alone through their C ABI
(Shmem.amo_raw, Shmem.atomic_add_v_raw), and one Fortran wrapper per family.

Expected values: Python integers reduced modulo 2^32 / 2^64 for the single
operations; numpy for the accumulate -- wrapping integer sums, and for float
and double sources drawn from small integers (|x| <= 512 on top of |t| <= 64:
every partial sum is an integer below 2^12, exact in either format), so the
comparison is of bits, with no tolerance. The arithmetic of the float and
double add itself -- one global_atomic_add_f32 / _f64 per element in the
memory-side atomic unit -- is held to the exact model of
tests/_fp_add_cases.py on its operand table (ties, sticky bits, gradual
underflow, overflow, zeros, Inf, NaN): the kernel alone, the library paths
with one adder, and every arrival order's rounded sum with several.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _fp_add_cases as fp
import test_bootstrap
from test_atomic_cpu import HERE, ROOT, SEMANTIC, build_c, run_workers

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel elements on both sides of an accumulate target
NP = {"int": np.int32, "long": np.int64, "longlong": np.int64, "float": np.float32, "double": np.float64}


# ---------------------------------------------------------------------------
# PE processes sharing the GPU
# ---------------------------------------------------------------------------
@pytest.mark.multipe
@pytest.mark.parametrize("npes", [1, 2, 4, 8])
def test_device_heap_semantics(tmp_path, npes):
    run_workers(npes, "device", SEMANTIC + ["mixed"], tmp_path, gpu=True, timeout=240)


@pytest.mark.multipe
def test_device_heap_wait_until(tmp_path):
    run_workers(2, "device", ["wait_until"], tmp_path, gpu=True, timeout=240)


@pytest.mark.multipe
@pytest.mark.parametrize("npes", [2, 4, 8])
def test_accumulate_across_pes(tmp_path, npes):
    run_workers(npes, "device", ["accumulate"], tmp_path, gpu=True, timeout=300)


@pytest.mark.multipe
def test_accumulate_float_semantics_across_pes(tmp_path):
    """worker test accumulate_fp on the device heap: PE 0 alone adds the
    operand table into PE 1's target from a device source, a pageable host
    source and a torch tensor; every non-NaN row against the exact model in
    every bit"""
    run_workers(2, "device", ["accumulate_fp"], tmp_path, gpu=True, timeout=240)


@pytest.mark.multipe
@pytest.mark.parametrize("npes", [2, 4])
def test_accumulate_arrival_orders(tmp_path, npes):
    """worker test accumulate_orders on the device heap: full-mantissa arrays
    from every PE at once; every element is the rounded sum in one of the
    npes! arrival orders"""
    run_workers(npes, "device", ["accumulate_orders"], tmp_path, gpu=True, timeout=240)


def oshrun(exe, npes, *args):
    env = dict(os.environ, SHMEM_DEVICE_HEAP_SIZE="16M", SHMEM_DEVICE_SCRATCH_SIZE="3M", SHMEM_BARRIER_TIMEOUT="120",
               SHMEM_WAIT_TIMEOUT="20")
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "oshrun"), "-np", str(npes), "--same-device",
                           exe, *args], env=env, capture_output=True, text=True, timeout=120)


@pytest.mark.multipe
def test_c_example_four_pes(tmp_path):
    exe = build_c(tmp_path, os.path.join(ROOT, "examples", "atomic_example.c"), "atomic_example")
    r = oshrun(exe, 4)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": PASS") == 4, r.stdout


@pytest.mark.multipe
def test_float_and_double_move_bit_patterns_two_pes(tmp_path):
    exe = build_c(tmp_path, os.path.join(HERE, "native", "atomic_bits.c"), "atomic_bits")
    r = oshrun(exe, 2)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": PASS") == 2, r.stdout


def _aborts(tmp_path, call, name, words):
    """a child on the GPU exits through the library's fatal message: an ordinary error exit"""
    body = f"""
    d = shm.malloc_device(256); x = (ctypes.c_long * 4)()
    ext = ctypes.c_void_p()
    assert shm.lib.hipMalloc(ctypes.byref(ext), ctypes.c_size_t(256)) == 0
    {call}
    print('returned')
    """
    extra = {"SHMEM_BOOTSTRAP_ONLY": "", "SHMEM_DEVICE_HEAP_SIZE": "16M", "SHMEM_DEVICE_SCRATCH_SIZE": "3M",
             "SHMEM_WAIT_TIMEOUT": "20"}
    rc, out = test_bootstrap.spawn(1, body, tmp_path, extra=extra)[0]
    assert rc == 1 and "returned" not in out, out
    assert name in out and words in out, out


@pytest.mark.multipe
def test_external_device_buffer_aborts_by_name(tmp_path):
    _aborts(tmp_path, "shm.atomic('finc', 'int', ext.value, 0)", "shmem_int_finc", "neither symmetric heap")


@pytest.mark.multipe
def test_accumulate_into_an_external_buffer_aborts_by_name(tmp_path):
    _aborts(tmp_path, "shm.atomic_add_v('float', ext.value, d, 8, 0)", "shmemx_float_atomic_add_v",
            "neither symmetric heap")


@pytest.mark.multipe
def test_pe_out_of_range_aborts_by_name(tmp_path):
    _aborts(tmp_path, "shm.atomic('cswap', 'long', d, 3, value=1, cond=0)", "shmem_long_cswap", "outside 0..0")


# ---------------------------------------------------------------------------
# the kernels alone (this process, no peers)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slot(shm):
    """8 bytes of host-coherent, device-visible memory for mi355_amo's old value"""
    p = ctypes.c_void_p()
    assert shm.lib.hipHostMalloc(ctypes.byref(p), ctypes.c_size_t(64), ctypes.c_uint(0x2 | 0x40000000)) == 0
    yield p.value
    shm.lib.hipHostFree(p)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("op", ["swap", "cswap", "fadd", "fetch", "set"])
def test_amo_kernel_every_op_at_every_phase(shm, slot, op, width):
    """every op x width with the target at every `width`-aligned 4-byte phase
    of a 16-byte line: the slot holds the old value, the target the new one,
    the words around it their sentinels. cswap runs once with a matching and
    once with a differing cond; fadd wraps at the top of the width."""
    mask = (1 << (8 * width)) - 1
    line = shm.malloc_device(256)
    SENT = 0xA5A5A5A5
    top = mask - 1                                 # fadd of 5 wraps
    for phase in range(0, 16, width):
        for cond_matches in ((True, False) if op == "cswap" else (True,)):
            words = np.full(64, SENT, np.uint32)
            init = top if op == "fadd" else 0x0123456789ABCDEF & mask
            words[16 + phase // 4: 16 + phase // 4 + width // 4] = np.array([init], np.uint64).view(np.uint32)[:width // 4]
            shm.put(line, words)
            value, cond = 0xFEDCBA9876543210 & mask if op != "fadd" else 5, (init if cond_matches else init ^ 1)
            ctypes.memset(slot, 0x77, 8)
            rc = shm.amo_raw(op, width, line + 64 + phase, value, cond, slot)
            assert rc == 0
            shm.sync()
            old = int(np.ctypeslib.as_array(ctypes.cast(slot, ctypes.POINTER(ctypes.c_uint64)), shape=(1,))[0])
            new = {"swap": value, "set": value, "fetch": init, "fadd": (init + value) & mask,
                   "cswap": value if cond_matches else init}[op]
            assert old == (0 if op == "set" else init), (op, width, phase, hex(old))
            got = shm.get(line, 64, np.uint32)
            words[16 + phase // 4: 16 + phase // 4 + width // 4] = np.array([new], np.uint64).view(np.uint32)[:width // 4]
            assert (got == words).all(), (op, width, phase, cond_matches, np.nonzero(got != words)[0])
    shm.free_device(line)


def test_amo_kernel_rejects_bad_arguments(shm, slot):
    d = shm.malloc_device(64)
    assert shm.amo_raw("swap", 2, d, 0, 0, slot) == -1
    assert shm.amo_raw("swap", 8, d + 4, 0, 0, slot) == -1
    assert shm.amo_raw("fetch", 4, None, 0, 0, slot) == -1
    assert shm.atomic_add_v_raw("short", d, d, 4) == -2
    assert shm.atomic_add_v_raw("double", d + 4, d, 1) == -1
    shm.sync()
    shm.free_device(d)


@pytest.fixture(scope="module")
def pass_elems(shm):
    """elements one pass of the saturated grid covers, from the grid the library reports"""
    d = shm.malloc_device(64 << 20)
    shm.put(d, np.zeros(16 << 20, np.int32))
    assert shm.atomic_add_v_raw("int", d, d + (32 << 20), 8 << 20) == 0
    shm.sync()
    gx, gy = shm.last_launch_grid()
    shm.free_device(d)
    assert gy == 1 and (gx, gx * 1024) == shm.atomic_add_v_plan(8 << 20, shm.device_cus())
    return gx * 1024


@pytest.fixture(scope="module")
def arena(shm, pass_elems):
    nbytes = 2 * ((3 * pass_elems + 5 + 2 * GUARD + 8) * 8 + 256)
    base = shm.malloc_device(nbytes)
    yield base, nbytes
    shm.free_device(base)


@pytest.mark.parametrize("dtype", ["int", "long", "longlong", "float", "double"])
def test_accumulate_kernel_alone(shm, arena, pass_elems, dtype):
    """n in {0, 1, 63, 64, 65, 255, 256, 257, pass - 1, pass + 1, 3 passes + 5}
    with target and source 1, 2 and 3 elements off a 16-byte boundary,
    independently (all nine pairs at the small sizes, three at the large
    ones); sentinels around the target and the source stay as they were.
    Float and double operands are small integers, every sum exact: what the
    add does when it rounds, underflows, overflows or meets a zero, an Inf or
    a NaN is test_accumulate_kernel_float_semantics'."""
    dt = NP[dtype]
    es = np.dtype(dt).itemsize
    base, nbytes = arena
    half = (nbytes // 2) & ~255
    rng = np.random.default_rng(99)
    small = [0, 1, 63, 64, 65, 255, 256, 257]
    large = [pass_elems - 1, pass_elems + 1, 3 * pass_elems + 5]
    cases = [(n, to, so) for n in small for to in (1, 2, 3) for so in (1, 2, 3)] + \
            [(n, to, so) for n in large for to, so in ((1, 3), (2, 2), (3, 1))]
    nmax = large[-1]
    if np.issubdtype(dt, np.integer):
        info = np.iinfo(dt)
        pool_t = rng.integers(info.min, info.max, nmax, dtype=dt, endpoint=True)
        pool_s = rng.integers(info.min, info.max, nmax, dtype=dt, endpoint=True)
        SENT = dt(0x5A5A5A5A)
    else:
        pool_t = rng.integers(-1024, 1024, nmax, endpoint=True).astype(dt)
        pool_s = rng.integers(-1024, 1024, nmax, endpoint=True).astype(dt)
        SENT = dt(-12345.0)
    for n, to, so in cases:
        tbuf = np.full(GUARD + to + n + GUARD, SENT, dt)
        sbuf = np.full(GUARD + so + n + GUARD, SENT, dt)
        tbuf[GUARD + to: GUARD + to + n] = pool_t[:n]
        sbuf[GUARD + so: GUARD + so + n] = pool_s[:n]
        assert GUARD * es % 16 == 0 and tbuf.nbytes <= half and sbuf.nbytes <= half
        shm.put(base, tbuf)
        shm.put(base + half, sbuf)
        rc = shm.atomic_add_v_raw(dtype, base + (GUARD + to) * es, base + half + (GUARD + so) * es, n)
        assert rc == 0, (n, to, so, rc)
        shm.sync()
        if n > pass_elems:
            assert shm.last_launch_grid()[0] * 1024 == pass_elems
        want = tbuf.copy()
        with np.errstate(over="ignore"):
            want[GUARD + to: GUARD + to + n] = (pool_t[:n] + pool_s[:n]).astype(dt)
        got = shm.get(base, tbuf.size, dt)
        bad = np.nonzero(got.view(np.uint8).reshape(tbuf.size, -1) != want.view(np.uint8).reshape(tbuf.size, -1))[0]
        assert bad.size == 0, (dtype, n, to, so, bad[:4] - GUARD - to, got[bad[:4]], want[bad[:4]])
        src_after = shm.get(base + half, sbuf.size, dt)
        assert (src_after.view(np.uint8) == sbuf.view(np.uint8)).all(), (dtype, n, to, so, "source changed")


@pytest.mark.parametrize("dtype", ["float", "double"])
def test_accumulate_kernel_float_semantics(shm, arena, dtype):
    """the operand table of tests/_fp_add_cases.py through the kernel alone,
    with target and source (0, 0), (1, 3) and (3, 1) elements off a 16-byte
    boundary, and once more in reversed row order (every class in other lanes
    and unroll slots): every non-NaN row equals one correctly rounded IEEE
    add -- nearest-even, gradual underflow, overflow to Inf, zero signs -- in
    every bit, every NaN row is a NaN; sentinels and source stay as they were.
    The table's length is the size: many blocks, all four unroll slots."""
    F = fp.FORMATS[dtype]
    dt, es = F.np_float, np.dtype(F.np_float).itemsize
    base, nbytes = arena
    half = (nbytes // 2) & ~255
    t, s = fp.cases(dtype)
    n = t.size
    assert n > 4 * 1024 and GUARD * es % 16 == 0 and base % 16 == 0 and half % 16 == 0
    fwd = np.arange(n)
    SENT = np.array([-12345.0], dt).view(F.np_uint)[0]
    for to, so, order in ((0, 0, fwd), (1, 3, fwd), (3, 1, fwd), (1, 3, fwd[::-1])):
        tbuf = np.full(GUARD + to + n + GUARD, SENT, F.np_uint)      # bit patterns: no NaN passes through a float move
        sbuf = np.full(GUARD + so + n + GUARD, SENT, F.np_uint)
        tbuf[GUARD + to: GUARD + to + n] = t.view(F.np_uint)[order]
        sbuf[GUARD + so: GUARD + so + n] = s.view(F.np_uint)[order]
        assert tbuf.nbytes <= half and sbuf.nbytes <= half
        shm.put(base, tbuf)
        shm.put(base + half, sbuf)
        rc = shm.atomic_add_v_raw(dtype, base + (GUARD + to) * es, base + half + (GUARD + so) * es, n)
        assert rc == 0, (dtype, to, so, rc)
        shm.sync()
        got = shm.get(base, tbuf.size, F.np_uint)
        where = f"kernel alone, target +{to}, source +{so}, rows {'reversed' if order[0] else 'in order'}"
        msg = fp.mismatches(dtype, got[GUARD + to: GUARD + to + n], order=order, where=where)
        assert msg is None, msg
        assert (got[:GUARD + to] == SENT).all() and (got[GUARD + to + n:] == SENT).all(), (where, "sentinels changed")
        assert (shm.get(base + half, sbuf.size, F.np_uint) == sbuf).all(), (where, "source changed")


# ---------------------------------------------------------------------------
# Fortran wrappers: one per family through its C-visible symbol (1 PE)
# ---------------------------------------------------------------------------
def test_fortran_wrappers_one_per_family(shm):
    L = shm.lib
    i32, i64 = ctypes.c_int, ctypes.c_long
    ref = ctypes.byref
    d = shm.malloc_device(64)
    shm.put(d, np.array([10, 0, 0, 0], np.int64))
    pe = i32(0)
    vp = ctypes.c_void_p

    def f(name, res, *args):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = [vp] + [ctypes.c_void_p] * (len(args) - 1)
        return fn(*args)
    assert f("shmem_int8_swap_", i64, d, ref(i64(11)), ref(pe)) == 10
    assert f("shmem_int8_cswap_", i64, d, ref(i64(11)), ref(i64(12)), ref(pe)) == 11
    assert f("shmem_int8_fadd_", i64, d, ref(i64(-2)), ref(pe)) == 12
    assert f("shmem_int8_finc_", i64, d, ref(pe)) == 10
    f("shmem_int8_add_", None, d, ref(i64(4)), ref(pe))
    f("shmem_int8_inc_", None, d, ref(pe))
    assert f("shmem_int8_fetch_", i64, d, ref(pe)) == 16
    f("shmem_int8_set_", None, d, ref(i64(-9)), ref(pe))
    f("shmem_int8_wait_until_", None, d, ref(i32(4)), ref(i64(0)))          # SHMEM_CMP_LT
    f("shmem_int8_wait_", None, d, ref(i64(5)))
    assert f("shmem_int4_fetch_", i32, d, ref(pe)) == -9
    f("shmem_real8_set_", None, d + 16, ref(ctypes.c_double(-0.0)), ref(pe))
    assert f("shmem_real8_swap_", ctypes.c_double, d + 16, ref(ctypes.c_double(2.5)), ref(pe)) == 0.0
    assert f("shmem_real8_fetch_", ctypes.c_double, d + 16, ref(pe)) == 2.5
    lock = d + 8
    f("shmem_set_lock_", None, lock)
    assert f("shmem_test_lock_", i32, lock) != 0
    f("shmem_clear_lock_", None, lock)
    assert f("shmem_test_lock_", i32, lock) == 0
    f("shmem_clear_lock_", None, lock)
    L.shmem_fence_()
    L.shmem_quiet_()
    got = shm.get(d, 3, np.int64)
    assert got[0] == -9 and got[2] == np.array([2.5]).view(np.int64)[0], got
    shm.free_device(d)
