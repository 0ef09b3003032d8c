"""CPU: shmem_iput / shmem_iget and shmem_<T>_p / _g without a GPU.

The ABI (strong pshmem_ names, weak shmem_ names, the 22 Fortran wrappers, the
strided kernel's entry point), the headers (every new prototype assigned to a
function pointer of its stated type), and the host-heap paths on 3 PE
processes under SHMEM_BOOTSTRAP_ONLY=1.

Expected results are numpy indexing of the inputs:
    target[k * tst] = source[k * sst]        k < nelems
Targets are pre-filled with a sentinel and compared whole, gaps and tail
included; the source is compared afterwards too.
"""
import os
import subprocess
import textwrap

import shmem_reduce
import test_bootstrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = {"char": "char", "short": "short", "int": "int", "long": "long", "longlong": "long long", "float": "float",
         "double": "double", "longdouble": "long double"}
STRIDED = [f"shmem_{t}_{op}" for op in ("iput", "iget") for t in TYPES] + \
          [f"shmem_{op}{b}" for op in ("iput", "iget") for b in (32, 64, 128)]
SINGLE = [f"shmem_{t}_{op}" for op in ("p", "g") for t in TYPES]
FORTRAN = [f"shmem_{k}_{op}_" for op in ("iput", "iget")
           for k in ("character", "double", "integer", "logical", "real", "complex")] + \
          [f"shmem_{op}{b}_" for op in ("iput", "iget") for b in (4, 8, 32, 64, 128)]


def test_symbols_strong_weak_fortran_and_kernel():
    assert len(STRIDED) == 22 and len(SINGLE) == 16 and len(FORTRAN) == 22
    out = subprocess.check_output(["nm", "-D", "--defined-only", shmem_reduce.LIB_PATH], text=True)
    kinds = {line.split()[-1]: line.split()[-2] for line in out.splitlines() if len(line.split()) >= 2}
    for n in STRIDED + SINGLE + FORTRAN:
        assert kinds.get("p" + n) == "T", "p" + n
        assert kinds.get(n) == "W", n
    assert kinds.get("mi355_strided_copy") == "T"
    assert kinds.get("mi355_strided_pull") == "T"


def test_headers_declare_every_prototype(tmp_path):
    lines = ["#include <stddef.h>", "#include <complex.h>", '#include "shmem.h"', '#include "pshmem.h"',
             '#include "shmem_fortran.h"', '#include "mi355_reduce.h"']
    k = 0
    for prefix in ("", "p"):
        for op in ("iput", "iget"):
            for t, ct in TYPES.items():
                lines.append(f"void (*f{k}) ({ct} *, const {ct} *, ptrdiff_t, ptrdiff_t, size_t, int) = "
                             f"{prefix}shmem_{t}_{op};"); k += 1
            for b in (32, 64, 128):
                lines.append(f"void (*f{k}) (void *, const void *, ptrdiff_t, ptrdiff_t, size_t, int) = "
                             f"{prefix}shmem_{op}{b};"); k += 1
        for t, ct in TYPES.items():
            lines.append(f"void (*f{k}) ({ct} *, {ct}, int) = {prefix}shmem_{t}_p;"); k += 1
            lines.append(f"{ct} (*f{k}) ({ct} *, int) = {prefix}shmem_{t}_g;"); k += 1
        for op in ("iput", "iget"):
            for kind, ct in (("character", "char"), ("double", "double"), ("integer", "int"), ("logical", "int"),
                             ("real", "int"), ("complex", "float _Complex")):
                lines.append(f"void (*f{k}) ({ct} *, const {ct} *, int *, int *, int *, int *) = "
                             f"{prefix}shmem_{kind}_{op}_;"); k += 1
            for b in (4, 8, 32, 64, 128):
                lines.append(f"void (*f{k}) (void *, const void *, int *, int *, int *, int *) = "
                             f"{prefix}shmem_{op}{b}_;"); k += 1
    lines.append("int (*kernel) (int, void *const *, const void *const *, ptrdiff_t, ptrdiff_t, size_t, int, void *) = "
                 "mi355_strided_copy;")
    assert k == 2 * (22 + 16 + 22)
    src = tmp_path / "iputget.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "iputget.o")])


HOST_BODY = """
import numpy as np
SENT = 0x5A
SIZES = [1, 2, 4, 8, 16]
STRIDES = [(1, 1), (1, 3), (3, 1), (2, 5)]
NELEMS = [0, 1, 5, 300]
SPAN = (300 * 5 + 8) * 16
def view(p, n):
    return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(n,))
def source_of(pe, salt):
    return np.random.default_rng(1000 * salt + pe).integers(0, 256, SPAN, dtype=np.uint8)
def expect(es, tst, sst, n, src):
    want = np.full(SPAN, SENT, dtype=np.uint8).reshape(-1, es)
    k = np.arange(n)
    want[k * tst] = src.reshape(-1, es)[k * sst]
    return want.reshape(-1)
sym_p, loc_p = shm.malloc(SPAN), shm.malloc(SPAN)   # the symmetric side; a local side (host memory as well)
SYM, LOC = view(sym_p, SPAN), view(loc_p, SPAN)
right, left = (me + 1) % npes, (me + npes - 1) % npes
checked = 0
salt = 0
for es in SIZES:
    for tst, sst in STRIDES:
        for n in NELEMS:
            salt += 1
            # iput: my local source into the next PE's symmetric target
            mine = source_of(me, salt)
            LOC[:] = mine
            SYM[:] = SENT
            shm.barrier_all()
            shm.iput(es, sym_p, loc_p, tst, sst, n, right)
            shm.barrier_all()
            want = expect(es, tst, sst, n, source_of(left, salt))
            assert (SYM == want).all(), ('iput', es, tst, sst, n, np.nonzero(SYM != want)[0][:8])
            assert (LOC == mine).all(), ('iput source', es, tst, sst, n)
            shm.barrier_all()
            # iget: the previous PE's symmetric source into my local target
            SYM[:] = mine
            LOC[:] = SENT
            shm.barrier_all()
            shm.iget(es, loc_p, sym_p, tst, sst, n, left)
            want = expect(es, tst, sst, n, source_of(left, salt))
            assert (LOC == want).all(), ('iget', es, tst, sst, n, np.nonzero(LOC != want)[0][:8])
            shm.barrier_all()
            assert (SYM == mine).all(), ('iget source', es, tst, sst, n)
            checked += 2
# a put and a get to this PE's own number: a local strided copy
SYM[:] = SENT
LOC[:] = source_of(me, 999)
shm.iput(2, sym_p, loc_p, 3, 2, 40, me)
assert (SYM == expect(2, 3, 2, 40, source_of(me, 999))).all()
LOC[:] = SENT
SYM[:] = source_of(me, 998)
shm.iget(16, loc_p, sym_p, 2, 3, 7, me)
assert (LOC == expect(16, 2, 3, 7, source_of(me, 998))).all()
shm.barrier_all()

# single elements: p to the next PE, g from the previous one
C = {'char': ctypes.c_char, 'short': ctypes.c_short, 'int': ctypes.c_int, 'long': ctypes.c_long,
     'longlong': ctypes.c_longlong, 'float': ctypes.c_float, 'double': ctypes.c_double,
     'longdouble': ctypes.c_longdouble}
def value_of(name, pe):
    if name == 'char':
        return bytes([65 + pe])
    if name in ('float', 'double', 'longdouble'):
        return 1.5 + pe * 0.25
    return -1000 * (pe + 1) + 7 if name != 'short' else -100 * (pe + 1)
def stored(name, v):
    # the bytes a C variable of that type holds: all of them, or the 10 value bytes of an x87 long double
    b = bytes(C[name](v))
    return b[:10] if name == 'longdouble' else b
singles = 0
for name, ct in C.items():
    nb = ctypes.sizeof(ct)
    p = getattr(shm.lib, f'shmem_{name}_p'); p.restype = None; p.argtypes = [ctypes.c_void_p, ct, ctypes.c_int]
    g = getattr(shm.lib, f'shmem_{name}_g'); g.restype = ct; g.argtypes = [ctypes.c_void_p, ctypes.c_int]
    SYM[:] = SENT
    shm.barrier_all()
    p(sym_p + 32, value_of(name, me), right)
    shm.barrier_all()
    keep = 10 if name == 'longdouble' else nb
    assert bytes(SYM[32:32 + keep]) == stored(name, value_of(name, left)), (name, bytes(SYM[32:32 + nb]))
    assert (SYM[:32] == SENT).all() and (SYM[32 + nb:] == SENT).all(), name
    got = g(sym_p + 32, right)     # what I put there
    assert stored(name, got) == stored(name, value_of(name, me)), (name, got)
    shm.barrier_all()
    singles += 1
shm.free(loc_p); shm.free(sym_p)
shm.finalize()
print('CHECKED', checked, singles)
"""


def test_host_heap_three_pes_without_gpu(tmp_path):
    """iput to the next PE and iget from the previous one on shmem_malloc
    memory: element sizes 1, 2, 4, 8, 16 x strides (1,1) (1,3) (3,1) (2,5) x
    nelems 0, 1, 5, 300; then p / g round trips of all eight types."""
    res = test_bootstrap.spawn(3, HOST_BODY, tmp_path)
    for rc, out in res:
        assert rc == 0, out
    for rc, out in res:
        assert out.split("CHECKED")[1].split() == [str(2 * 5 * 4 * 4), "8"], out


def _aborts(tmp_path, call, name, words):
    body = f"""
    p = shm.malloc(256); q = shm.malloc(256)
    {call}
    print('returned')
    """
    rc, out = test_bootstrap.spawn(1, body, tmp_path)[0]
    assert rc != 0 and "returned" not in out, out
    assert name in out and words in out, out


def test_zero_stride_aborts_with_the_calls_name(tmp_path):
    _aborts(tmp_path, "shm.iput(4, q, p, 0, 1, 1, 0)", "shmem_iput32", "at least 1")


def test_zero_source_stride_of_a_get_aborts(tmp_path):
    _aborts(tmp_path, "shm.iget(2, q, p, 1, 0, 1, 0)", "shmem_short_iget", "at least 1")


def test_pe_out_of_range_aborts_with_the_calls_name(tmp_path):
    _aborts(tmp_path, "shm.iget(16, q, p, 1, 2, 1, 1)", "shmem_iget128", "outside 0..0")


def test_pe_out_of_range_put_aborts(tmp_path):
    _aborts(tmp_path, "shm.iput(1, q, p, 2, 1, 0, -1)", "shmem_char_iput", "outside 0..0")
