"""One PE of the atomics / waits / locks tests (tests/test_atomic_cpu.py on the
host heap without a GPU, tests/test_gpu_atomic.py on the device heap).

    python atomic_worker.py spec.json

spec: {"heap": "host" | "device", "tests": [names], "dir": scratch directory}.
Every test is a function test_<name>(heap); values a test must see from every
PE travel through files in the scratch directory between two barriers, so the
checks never use the calls under test to move their own evidence. The last
line printed is a JSON record {"checked": [...], "failures": [...]}.
"""
import ctypes
import json
import operator
import os
import sys
import time
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "osss-gasnet_amd"))
spec = json.load(open(sys.argv[1]))
if "accumulate" in spec["tests"] or ("accumulate_fp" in spec["tests"] and spec["heap"] == "device"):
    # torch brings a HIP runtime of its own: it has to be loaded before the
    # library, as in the other torch workers, so that one runtime serves both
    import torch  # noqa: E402,F401
import shmem_reduce  # noqa: E402

import _fp_add_cases as fp  # noqa: E402  (tests/, this script's directory)

shm = shmem_reduce.Shmem()
shm.init()
me, npes = shm.my_pe(), shm.n_pes()
DIR = spec["dir"]
INT_TYPES = {"int": np.int32, "long": np.int64, "longlong": np.int64}
WAIT_TYPES = {"short": np.int16, "int": np.int32, "long": np.int64, "longlong": np.int64}
_round = [0]


def alloc(heap, nbytes):
    p = shm.malloc_device(nbytes) if heap == "device" else shm.malloc(nbytes)
    assert p, (heap, nbytes)
    return p


def free(heap, p):
    (shm.free_device if heap == "device" else shm.free)(p)


def poke(heap, ptr, arr):
    arr = np.ascontiguousarray(arr)
    if heap == "device":
        shm.put(ptr, arr)
    else:
        ctypes.memmove(ptr, arr.ctypes.data, arr.nbytes)


def peek(heap, ptr, n, dt):
    if heap == "device":
        return shm.get(ptr, n, dt)
    out = np.empty(n, dtype=dt)
    ctypes.memmove(out.ctypes.data, ptr, out.nbytes)
    return out


def gather(values):
    """every PE's list of integers, as a list indexed by PE (through files, between barriers)"""
    _round[0] += 1
    path = os.path.join(DIR, f"r{_round[0]}_{{}}.json")
    with open(path.format(me) + ".tmp", "w") as f:
        json.dump([int(v) for v in values], f)
    os.rename(path.format(me) + ".tmp", path.format(me))
    shm.barrier_all()
    got = [json.load(open(path.format(pe))) for pe in range(npes)]
    shm.barrier_all()
    return got


def test_tickets(heap):
    K = 32
    for name, dt in INT_TYPES.items():
        for r in sorted({0, npes - 1}):
            c = alloc(heap, 8)
            poke(heap, c, np.zeros(1, dt))
            shm.barrier_all()
            mine = [shm.atomic("finc", name, c, r) for _ in range(K)]
            allv = gather(mine)
            flat = sorted(v for pe in allv for v in pe)
            assert flat == list(range(npes * K)), (name, r, flat[:8])
            assert mine == sorted(mine), (name, "tickets of one PE are not increasing", mine)
            assert shm.atomic("fetch", name, c, r) == npes * K, name
            shm.barrier_all()
            free(heap, c)


def test_fadd_chain(heap):
    """Signed distinct powers of two: every partial sum over any arrival order
    is different, so the (old, value) pairs sorted by old form one chain.
    At most 28 adds, so that the sums fit an int."""
    J = min(4, 28 // npes)
    for name, dt in INT_TYPES.items():
        c = alloc(heap, 8)
        init = 5
        poke(heap, c, np.full(1, init, dt))
        shm.barrier_all()
        r = npes - 1
        vals = [(-1) ** (me + j) * (1 << (1 + me * J + j)) for j in range(J)]
        olds = [shm.atomic("fadd", name, c, r, value=v) for v in vals]
        allv = gather(olds + vals)
        step = {}
        for pe in allv:
            for o, v in zip(pe[:J], pe[J:]):
                assert o not in step, (name, "two adds saw the same old value", o)
                step[o] = v
        cur = init
        for _ in range(npes * J):
            assert cur in step, (name, "chain broken at", cur, step)
            cur += step.pop(cur)
        assert not step
        assert shm.atomic("fetch", name, c, r) == cur, name
        shm.barrier_all()
        free(heap, c)


def test_wrap(heap):
    right = (me + 1) % npes
    for name, dt in INT_TYPES.items():
        info = np.iinfo(dt)
        c = alloc(heap, 8)
        poke(heap, c, np.full(1, info.max, dt))
        shm.barrier_all()
        old = shm.atomic("fadd", name, c, right, value=1)
        assert old == info.max, (name, old)
        shm.barrier_all()
        assert peek(heap, c, 1, dt)[0] == info.min, name
        assert shm.atomic("finc", name, c, right) == info.min, name
        shm.atomic("add", name, c, right, value=-2)
        shm.atomic("inc", name, c, right)
        shm.barrier_all()
        assert peek(heap, c, 1, dt)[0] == info.min, name    # min + 1 - 2 (wraps down to max) + 1 (and up again)
        shm.barrier_all()
        free(heap, c)


def test_swap(heap):
    J = 4
    for name, dt in INT_TYPES.items():
        c = alloc(heap, 8)
        init = -77
        poke(heap, c, np.full(1, init, dt))
        shm.barrier_all()
        tokens = [1000 * (me + 1) + j for j in range(J)]
        got = [shm.atomic("swap", name, c, 0, value=t) for t in tokens]
        allv = gather(got + tokens)
        final = shm.atomic("fetch", name, c, 0)
        returned = sorted([v for pe in allv for v in pe[:J]] + [final])
        given = sorted([v for pe in allv for v in pe[J:]] + [init])
        assert returned == given, (name, returned, given)
        shm.barrier_all()
        free(heap, c)


def test_cswap_election(heap):
    for name, dt in INT_TYPES.items():
        for r in sorted({0, npes - 1}):
            c = alloc(heap, 8)
            poke(heap, c, np.zeros(1, dt))
            shm.barrier_all()
            seen = shm.atomic("cswap", name, c, r, value=me + 1, cond=0)
            allv = [pe[0] for pe in gather([seen])]
            winners = [pe for pe, v in enumerate(allv) if v == 0]
            assert len(winners) == 1, (name, allv)
            w = winners[0] + 1
            assert all(v == w for pe, v in enumerate(allv) if pe != winners[0]), (name, allv)
            assert shm.atomic("fetch", name, c, r) == w, name
            shm.barrier_all()
            free(heap, c)


def test_neighbours(heap):
    """a 32-bit target at an address 4 mod 8 between sentinels"""
    right = (me + 1) % npes
    c = alloc(heap, 32)
    assert c % 8 == 0
    SENT = np.int32(0x5A5A5A5A)
    words = np.full(8, SENT, np.int32)
    words[1] = 10
    poke(heap, c, words)
    shm.barrier_all()
    assert shm.atomic("fadd", "int", c + 4, right, value=5) == 10
    assert shm.atomic("swap", "int", c + 4, right, value=-3) == 15
    assert shm.atomic("cswap", "int", c + 4, right, value=8, cond=-3) == -3
    shm.atomic("set", "int", c + 4, right, value=9)
    assert shm.atomic("fetch", "int", c + 4, right) == 9
    shm.barrier_all()
    got = peek(heap, c, 8, np.int32)
    words[1] = 9
    assert (got == words).all(), got
    shm.barrier_all()
    free(heap, c)


WAIT_CASES = [("eq", 0, -5, -5), ("ne", -7, -7, 5), ("gt", -10, 3, 5), ("le", 10, -5, -5), ("lt", 10, -1, -5),
              ("ge", -10, 5, 5)]   # cmp, initial value, cmp_value, released with


HOLDS = {"eq": operator.eq, "ne": operator.ne, "gt": operator.gt, "le": operator.le, "lt": operator.lt,
         "ge": operator.ge}


def test_wait_until(heap):
    """PE 1 waits on a variable at an address 2 mod 4 (short) / 4 mod 8 (int)
    between sentinels; PE 0 sleeps 50 ms, passes its clock through a second
    symmetric variable, then releases with shmem_<T>_p, and in a second round
    with an atomic set."""
    assert npes == 2
    stamp = shm.malloc(8)                       # a double in the host heap
    p_double = shm._typed_fn("shmem_double_p", None, [ctypes.c_void_p, ctypes.c_double, ctypes.c_int])
    for name, dt in WAIT_TYPES.items():
        es = np.dtype(dt).itemsize
        off = {2: 2, 4: 4, 8: 8}[es]
        SENT = np.iinfo(dt).max - 3
        p_fn = shm._typed_fn(f"shmem_{name}_p", None, [ctypes.c_void_p, shm._AMO_C[name], ctypes.c_int])
        for how in ("p", "set"):
            if how == "set" and name == "short":
                continue
            for cmp, init, want, rel in WAIT_CASES:
                v = alloc(heap, 32)
                cells = np.full(32 // es, SENT, dt)
                cells[off // es] = init
                poke(heap, v, cells)
                poke("host", stamp, np.zeros(1, np.float64))
                shm.barrier_all()
                if me == 0:
                    time.sleep(0.05)
                    p_double(stamp, time.monotonic(), 1)
                    if how == "p":
                        p_fn(v + off, rel, 1)
                    else:
                        shm.atomic("set", name, v + off, 1, value=rel)
                else:
                    t_in = time.monotonic()
                    shm.wait_until(name, v + off, cmp, want)
                    t_out = time.monotonic()
                    released = peek("host", stamp, 1, np.float64)[0]
                    got = peek(heap, v, 32 // es, dt)
                    assert got[off // es] == rel, (name, how, cmp, got)
                    assert HOLDS[cmp](int(got[off // es]), want), (name, how, cmp, got)
                    assert released > 0 and t_out >= released, (name, how, cmp, "returned before the release",
                                                                t_in, t_out, released)
                    cells[off // es] = rel
                    assert (got == cells).all(), (name, how, cmp, got)
                shm.barrier_all()
                free(heap, v)
    shm.free(stamp)


def test_locks(heap):
    K = 64
    lock = alloc(heap, 8)
    count = alloc(heap, 8)
    poke(heap, lock, np.zeros(1, np.int64))
    poke(heap, count, np.zeros(1, np.int64))
    shm.barrier_all()
    g = shm._typed_fn("shmem_long_g", ctypes.c_long, [ctypes.c_void_p, ctypes.c_int])
    p = shm._typed_fn("shmem_long_p", None, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int])
    for _ in range(K):
        shm.set_lock(lock)
        p(count, g(count, 0) + 1, 0)
        shm.clear_lock(lock)
    shm.barrier_all()
    assert g(count, 0) == npes * K, g(count, 0)
    shm.barrier_all()
    # test_lock: everyone tries at once, exactly one takes it; while it is held nobody else can
    mine = shm.test_lock(lock)
    allv = [pe[0] for pe in gather([mine])]
    assert sum(1 for v in allv if v == 0) == 1, allv
    again = 0 if mine == 0 else shm.test_lock(lock)
    assert mine == 0 or again != 0, (mine, again)
    shm.barrier_all()
    if mine == 0:
        shm.clear_lock(lock)
    shm.barrier_all()
    # released: the lock can be taken again, by set_lock too
    if me == npes - 1:
        assert shm.test_lock(lock) == 0
        shm.clear_lock(lock)
        shm.set_lock(lock)
        shm.clear_lock(lock)
    shm.barrier_all()
    free(heap, count)
    free(heap, lock)


def test_mixed(heap):
    """a device-heap counter and a host-heap counter updated alternately"""
    K = 16
    d, h = alloc("device", 8), alloc("host", 8)
    poke("device", d, np.zeros(1, np.int64))
    poke("host", h, np.zeros(1, np.int64))
    shm.barrier_all()
    r = npes - 1
    got_d, got_h = [], []
    for _ in range(K):
        got_d.append(shm.atomic("finc", "long", d, r))
        got_h.append(shm.atomic("finc", "long", h, r))
    allv = gather(got_d + got_h)
    want = list(range(npes * K))
    assert sorted(v for pe in allv for v in pe[:K]) == want
    assert sorted(v for pe in allv for v in pe[K:]) == want
    assert shm.atomic("fetch", "long", d, r) == npes * K and shm.atomic("fetch", "long", h, r) == npes * K
    shm.barrier_all()
    free("host", h)
    free("device", d)


ACC_TYPES = {"int": np.int32, "long": np.int64, "longlong": np.int64, "float": np.float32, "double": np.float64}


def acc_source(name, base, pe):
    """PE pe's source. Integers: the full-range base times an odd number,
    wrapping, so the sums wrap too. Floats: |base| <= 64 times pe + 1 <= 8, so
    |x| <= 512 and every partial sum of up to 8 of them on top of an initial
    |t| <= 64 stays below 2^12: exact in either format in any arrival order."""
    dt = ACC_TYPES[name]
    with np.errstate(over="ignore"):
        return (base * dt(2 * pe + 1)).astype(dt) if np.issubdtype(dt, np.integer) else (base * dt(pe + 1)).astype(dt)


def test_accumulate(heap):
    """every PE adds its own array into the last PE's, concurrently, between two
    barriers; n = one grid pass + 1; sources in device memory, in pageable
    host memory, and a torch tensor through the tensor form. Float and double
    sums of these small integers are exact: what the add does when it rounds,
    underflows, overflows or meets a zero, an Inf or a NaN is
    test_accumulate_fp's, and rounded sums under contention
    test_accumulate_orders'."""
    _, pass_elems = shm.atomic_add_v_plan(1 << 40, shm.device_cus())
    n = pass_elems + 1
    r = npes - 1
    for name, dt in ACC_TYPES.items():
        rng = np.random.default_rng(4242)            # the same arrays on every PE
        if np.issubdtype(dt, np.integer):
            info = np.iinfo(dt)
            base = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
            init = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        else:
            base = rng.integers(-64, 64, n, endpoint=True).astype(dt)
            init = rng.integers(-64, 64, n, endpoint=True).astype(dt)
        with np.errstate(over="ignore"):
            want = init.copy()
            for pe in range(npes):
                want = (want + acc_source(name, base, pe)).astype(dt)
        mine = acc_source(name, base, me)
        for kind in ("device", "host", "torch"):
            if kind == "torch" and name == "longlong":
                continue
            if kind == "torch":
                tt = shm.heap_tensor(n, getattr(torch, np.dtype(dt).name))
                target = tt.data_ptr()
            else:
                target = shm.malloc_device(n * mine.itemsize)
            shm.put(target, init)
            dsrc = None
            if kind == "device":
                dsrc = shm.malloc_device(n * mine.itemsize)
                shm.put(dsrc, mine)
            shm.barrier_all()
            if kind == "device":
                shm.atomic_add_v(name, target, dsrc, n, r)
            elif kind == "host":
                shm.atomic_add_v(name, target, mine.ctypes.data, n, r)
            else:
                shm.atomic_add_v_tensors(tt, torch.from_numpy(mine).cuda(), r)
            shm.barrier_all()
            got = shm.get(target, n, dt)
            expect = want if me == r else init
            bad = np.nonzero(got.view(np.uint8).reshape(n, -1) != expect.view(np.uint8).reshape(n, -1))[0]
            assert bad.size == 0, (name, kind, bad[:4], got[bad[:4]], expect[bad[:4]])
            if dsrc is not None:
                assert (shm.get(dsrc, n, dt).view(np.uint8) == mine.view(np.uint8)).all(), (name, "source changed")
            shm.barrier_all()
            if dsrc is not None:
                shm.free_device(dsrc)
            shm.free_device(target)


FP_GUARD = 64       # sentinel elements on both sides of the table's target: a multiple of 16 bytes
FP_SENT = -12345.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_accumulate_fp(heap):
    """PE 0 alone adds the operand table of tests/_fp_add_cases.py into PE 1's
    target, one element off a 16-byte boundary between sentinels: a single
    adder, so every non-NaN row has one right answer in every bit and every
    NaN row is a NaN. Device heap: a device source, a pageable host source
    (staged through scratch C) and a torch tensor. Host heap: a pageable
    source and one in the host heap, neither needing a device."""
    assert npes == 2
    for name in ("float", "double"):
        t, s = fp.cases(name)
        dt, n = t.dtype, t.size
        es = dt.itemsize
        lo, hi = FP_GUARD + 1, FP_GUARD + 1 + n
        for kind in (("device", "host", "torch") if heap == "device" else ("host", "heap")):
            buf = np.full(hi + FP_GUARD, FP_SENT, dt)
            _bits(buf[lo:hi])[:] = _bits(t)                      # bytes: no NaN passes through a float move
            if kind == "torch":
                tt = shm.heap_tensor(buf.size, getattr(torch, dt.name))
                base = tt.data_ptr()
            else:
                base = alloc(heap, buf.nbytes)
            assert base % 16 == 0
            poke(heap, base, buf)
            mine = s.copy()
            src = None
            if kind in ("device", "heap"):
                src = alloc(kind.replace("heap", "host"), n * es)
                poke(kind.replace("heap", "host"), src, mine)
            elif kind == "torch":
                src_t = torch.from_numpy(mine.copy()).cuda()
            shm.barrier_all()
            if me == 0:
                if kind == "torch":
                    shm.atomic_add_v_tensors(tt[lo:hi], src_t, 1)
                else:
                    shm.atomic_add_v(name, base + lo * es, src if src is not None else mine.ctypes.data, n, 1)
            shm.barrier_all()
            got = peek(heap, base, buf.size, dt)
            where = f"{heap} heap, {kind} source, PE {me}"
            assert (_bits(got[:lo]) == _bits(buf[:lo])).all() and (_bits(got[hi:]) == _bits(buf[hi:])).all(), \
                (name, where, "sentinels changed")
            if me == 1:
                msg = fp.mismatches(name, got[lo:hi], where=where)
                assert msg is None, msg
            else:
                assert (_bits(got) == _bits(buf)).all(), (name, where, "the adder's own copy changed")
            after = {"device": lambda: shm.get(src, n, dt), "heap": lambda: peek("host", src, n, dt),
                     "host": lambda: mine, "torch": lambda: src_t.cpu().numpy()}[kind]()
            assert (_bits(after) == _bits(s)).all(), (name, where, "source changed")
            shm.barrier_all()
            if src is not None:
                free(kind.replace("heap", "host"), src)
            free(heap, base)


def test_accumulate_orders(heap):
    """every PE adds its own full-mantissa array (magnitudes in [1, 256),
    random signs) into the last PE's target at once, between two barriers;
    n = 4,096 + 64. Every element must equal the sum in one of the npes!
    arrival orders, each rounded in the format on top of the initial value
    (tests/_fp_add_cases.py orders_case: no term can be absorbed, so a lost
    or doubled update equals none of them). Not vacuous: at least 25 % of
    the elements (2 PEs; the inputs give 27.7 %) or 75 % (4 PEs; 82.5 %)
    have two or more distinct legal results."""
    r = npes - 1
    for name in ("float", "double"):
        init, sources, legal, share = fp.orders_case(name, npes)
        assert share >= fp.ORDERS_MIN_SHARE[npes], (name, npes, share)
        dt, n = init.dtype, init.size
        target = alloc(heap, n * dt.itemsize)
        poke(heap, target, init)
        src = None
        if heap == "device":
            src = alloc("device", n * dt.itemsize)
            poke("device", src, sources[me])
        mine = sources[me].copy()
        shm.barrier_all()
        shm.atomic_add_v(name, target, src if src is not None else mine.ctypes.data, n, r)
        shm.barrier_all()
        got = peek(heap, target, n, dt)
        if me == r:
            bad = fp.illegal_elements(name, npes, got)
            u = legal.dtype
            assert bad.size == 0, (name, heap, f"{bad.size} of {n} elements equal the sum in no arrival order", bad[:4],
                                   [hex(v) for v in got.view(u)[bad[:4]]],
                                   [[hex(v) for v in legal[:, i]] for i in bad[:2]])
        else:
            assert (_bits(got) == _bits(init)).all(), (name, heap, "a target that nobody added into changed")
        shm.barrier_all()
        if src is not None:
            free("device", src)
        free(heap, target)


checked, failures = [], []
for t in spec["tests"]:
    try:
        globals()["test_" + t](spec["heap"])
        checked.append(t)
    except Exception:  # noqa: BLE001
        failures.append({"test": t, "trace": traceback.format_exc()[-2500:]})
        break   # the other PEs are no longer in step: stop here, the launcher reports it
if not failures:
    shm.barrier_all()
    shm.finalize()
print(json.dumps({"pe": me, "checked": checked, "failures": failures}))
sys.stdout.flush()
if failures:
    shm.lib.shmem_global_exit(1)   # the PEs waiting for this one at a barrier leave too
