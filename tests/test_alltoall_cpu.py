"""CPU: shmem_alltoall32/64 and shmem_alltoalls32/64 without a GPU.

The ABI (strong pshmem_ names, weak shmem_ names, the four Fortran wrappers,
the strided kernel's entry point), the header (constants and prototypes), the
host-heap path on 3 PE processes under SHMEM_BOOTSTRAP_ONLY=1, and the
argument check of Shmem.alltoall_tensors.

Expected results are the specification's formula, with m and i the indices in
the active set:
    target_on_m[(i*nelems + k) * dst] = source_on_i[(m*nelems + k) * sst]
Targets are pre-filled with -7 and every element the formula does not name
must still hold it.
"""
import os
import subprocess
import textwrap

import pytest

import shmem_reduce
import test_bootstrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["shmem_alltoall32", "shmem_alltoall64", "shmem_alltoalls32", "shmem_alltoalls64"]


def test_symbols_strong_weak_fortran_and_kernel():
    out = subprocess.check_output(["nm", "-D", "--defined-only", shmem_reduce.LIB_PATH], text=True)
    kinds = {line.split()[-1]: line.split()[-2] for line in out.splitlines() if len(line.split()) >= 2}
    for n in NAMES:
        assert kinds.get("p" + n) == "T", "p" + n
        assert kinds.get(n) == "W", n
        assert kinds.get(n + "_") == "W", n + "_"
        assert kinds.get("p" + n + "_") == "T", "p" + n + "_"
    assert kinds.get("mi355_strided_pull") == "T"


def test_header_declares_constants_and_prototypes(tmp_path):
    src = tmp_path / "a2a.c"
    src.write_text(textwrap.dedent("""
        #include <stddef.h>
        #include "shmem.h"
        long psync_a[SHMEM_ALLTOALL_SYNC_SIZE];
        long psync_s[SHMEM_ALLTOALLS_SYNC_SIZE];
        void (*f32) (void *, const void *, size_t, int, int, int, long *) = shmem_alltoall32;
        void (*f64) (void *, const void *, size_t, int, int, int, long *) = shmem_alltoall64;
        void (*s32) (void *, const void *, ptrdiff_t, ptrdiff_t, size_t, int, int, int, long *) = shmem_alltoalls32;
        void (*s64) (void *, const void *, ptrdiff_t, ptrdiff_t, size_t, int, int, int, long *) = shmem_alltoalls64;
        int sizes_match[(SHMEM_ALLTOALL_SYNC_SIZE == 128L / (sizeof (long) / sizeof (int))
                         && SHMEM_ALLTOALLS_SYNC_SIZE == SHMEM_ALLTOALL_SYNC_SIZE) ? 1 : -1];
    """))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "a2a.o")])


def test_fortran_include_has_both_sizes():
    text = open(os.path.join(ROOT, "include", "shmem.fh")).read()
    assert "      parameter (SHMEM_ALLTOALL_SYNC_SIZE = 128)\n" in text
    assert "      parameter (SHMEM_ALLTOALLS_SYNC_SIZE = 128)\n" in text


HOST_BODY = """
import numpy as np
L = shm.lib
SENT = -7
SETS = [(0, 0, 3), (1, 0, 2)]
STRIDES = [(1, 1), (1, 3), (3, 1), (2, 5)]
NELEMS = [0, 1, 5]
MAXN = 3 * 5
def arr(p, n, dt):
    return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,))
def source_of(pe, n, dt, salt):
    return (np.arange(n, dtype=np.int64) * 7 + 100003 * (pe + 1) + 1000003 * salt).astype(dt)
slen, tlen = MAXN * 5 + 8, MAXN * 3 + 8
src_p = shm.malloc(slen * 8)
tgt_p = shm.malloc(tlen * 8)
psync = np.full(128, -1, dtype=np.int64)
checked = 0
salt = 0
for bits, dt in ((32, np.int32), (64, np.int64)):
    S, T = arr(src_p, slen, dt), arr(tgt_p, tlen, dt)
    for start, logs, size in SETS:
        members = [start + k * (1 << logs) for k in range(size)]
        for nelems in NELEMS:
            for strided in (False, True):
                for dst, sst in (STRIDES if strided else [(1, 1)]):
                    salt += 1
                    S[:] = source_of(me, slen, dt, salt)
                    T[:] = SENT
                    shm.barrier_all()
                    if me in members:
                        if strided:
                            shm.alltoalls(bits, tgt_p, src_p, dst, sst, nelems, start, logs, size)
                        else:
                            shm.alltoall(bits, tgt_p, src_p, nelems, start, logs, size)
                        m = members.index(me)
                        want = np.full(tlen, SENT, dtype=dt)
                        for i, pe in enumerate(members):
                            theirs = source_of(pe, slen, dt, salt)
                            for k in range(nelems):
                                want[(i * nelems + k) * dst] = theirs[(m * nelems + k) * sst]
                        assert (T == want).all(), (bits, (start, logs, size), nelems, strided, dst, sst, T, want)
                        checked += 1
                    else:
                        assert (T == SENT).all()
                    shm.barrier_all()
assert (psync == -1).all()
shm.free(tgt_p); shm.free(src_p)
shm.finalize()
print('CHECKED', checked)
"""


def test_host_heap_three_pes_without_gpu(tmp_path):
    """alltoall32/64 and alltoalls32/64 on shmem_malloc memory, sets (0,0,3)
    and (1,0,2), nelems 0/1/5, strides (1,1) (1,3) (3,1) (2,5)."""
    res = test_bootstrap.spawn(3, HOST_BODY, tmp_path)
    for rc, out in res:
        assert rc == 0, out
    counts = sorted(int(out.split("CHECKED")[1]) for rc, out in res)
    per_set = 2 * 3 * (1 + 4)                     # widths x nelems x (plain + 4 stride pairs)
    assert counts == [per_set, 2 * per_set, 2 * per_set], counts


def test_bad_stride_aborts_with_message(tmp_path):
    body = """
    p = shm.malloc(64); q = shm.malloc(64)
    shm.alltoalls(32, q, p, 0, 1, 1, 0, 0, 1)
    print('returned')
    """
    rc, out = test_bootstrap.spawn(1, body, tmp_path)[0]
    assert rc != 0 and "returned" not in out
    assert "shmem_alltoalls32" in out and "at least 1" in out, out


class _FakeTensor:
    """what alltoall_tensors looks at before it touches the GPU"""

    def __init__(self, numel, element_size):
        self._n, self._es = numel, element_size

    def numel(self):
        return self._n

    def element_size(self):
        return self._es


def test_alltoall_tensors_rejects_blocks_not_multiple_of_4_bytes():
    shm = shmem_reduce.Shmem()
    # 2 blocks of 3 int16 = 6 bytes each
    with pytest.raises(ValueError, match="multiple of 4"):
        shm.alltoall_tensors(_FakeTensor(6, 2), _FakeTensor(6, 2), PE_size=2)
    # 3 blocks of 1 byte
    with pytest.raises(ValueError, match="multiple of 4"):
        shm.alltoall_tensors(_FakeTensor(3, 1), _FakeTensor(3, 1), PE_size=3)
    with pytest.raises(ValueError, match="same number of bytes"):
        shm.alltoall_tensors(_FakeTensor(8, 4), _FakeTensor(8, 8), PE_size=2)
    with pytest.raises(ValueError, match="do not divide"):
        shm.alltoall_tensors(_FakeTensor(7, 4), _FakeTensor(7, 4), PE_size=3)


def test_alltoall_trace_level_names_the_path(tmp_path):
    """SHMEM_LOG_LEVELS=alltoall: one line per call saying how it ran"""
    log = tmp_path / "trace.log"
    body = """
    p = shm.malloc(256); q = shm.malloc(256)
    shm.barrier_all()
    shm.alltoall(32, q, p, 4)
    shm.alltoalls(64, q, p, 2, 1, 3)
    shm.finalize()
    """
    res = test_bootstrap.spawn(2, body, tmp_path, extra={"SHMEM_LOG_LEVELS": "alltoall", "SHMEM_LOG_FILE": str(log)})
    for rc, out in res:
        assert rc == 0, out
    lines = log.read_text().splitlines()
    assert len(lines) == 4 and all(": ALLTOALL: " in ln and ln.endswith(", host") for ln in lines), lines
    assert sum("shmem_alltoall32: 2 x 4 elements of 4 bytes, strides 1/1" in ln for ln in lines) == 2, lines
    assert sum("shmem_alltoalls64: 2 x 3 elements of 8 bytes, strides 2/1" in ln for ln in lines) == 2, lines
