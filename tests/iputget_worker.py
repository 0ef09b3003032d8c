#!/usr/bin/env python3
"""One PE of a multi-PE strided put/get test (tests/test_gpu_iputget.py): runs
the cases of a spec in order, checks each against numpy indexing of the
inputs and prints one JSON line {"checked", "failures"}.

usage: iputget_worker.py SPEC.json   (identity from SHMEM_PE / SHMEM_NPES)

A case: {"id", "op": iput | iget, "es", "n", "tst", "sst", "sym": device |
host (where the symmetric side lives), "loc": device | host | pageable (the
local side: device heap, shmem_malloc'd host memory, numpy memory), "to": next
| self, "seed"}.
  iput  every PE puts its local source to PE (me + 1) % N (or itself); after
        a barrier it compares its WHOLE symmetric target (sentinel-filled
        before) with what PE (me - 1) % N's source gives, and its own source
        with what it was.
  iget  every PE gets from PE (me + N - 1) % N (or itself) into its
        sentinel-filled local target and compares the whole of it; after a
        barrier, its symmetric source with what it was.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "osss-gasnet_amd"))

import shmem_reduce  # noqa: E402

SENTINEL = 0x5A
TAIL = 5   # elements of the target past the last one written


def source_of(pe, seed, nbytes):
    return np.random.default_rng(seed * 1009 + pe).integers(0, 256, nbytes, dtype=np.uint8)


def spans(c):
    n, es = c["n"], c["es"]
    slen = ((n - 1) * c["sst"] + 1) * es if n else 0
    tlen = (((n - 1) * c["tst"] + 1) if n else 0) * es + TAIL * es
    return slen + 16, tlen


def expected(c, src):
    slen, tlen = spans(c)
    es, n = c["es"], c["n"]
    want = np.full(tlen, SENTINEL, dtype=np.uint8).reshape(-1, es)
    k = np.arange(n)
    want[k * c["tst"]] = src[:slen].reshape(-1, es)[k * c["sst"]]
    return want.reshape(-1)


class Buffers:
    def __init__(self, shm, nbytes):
        self.shm = shm
        self.ptr = {("sym", "device"): shm.malloc_device(nbytes), ("sym", "host"): shm.malloc(nbytes),
                    ("loc", "device"): shm.malloc_device(nbytes), ("loc", "host"): shm.malloc(nbytes)}
        assert all(self.ptr.values()), self.ptr
        self.pageable = np.empty(nbytes + 64, dtype=np.uint8)
        self.ptr[("loc", "pageable")] = self.pageable.ctypes.data + 16

    def write(self, key, data):
        if key[1] == "device":
            self.shm.put(self.ptr[key], data)
        else:
            ctypes.memmove(self.ptr[key], data.ctypes.data, data.nbytes)

    def read(self, key, nbytes):
        if key[1] == "device":
            return self.shm.get(self.ptr[key], nbytes, np.uint8)
        out = np.empty(nbytes, dtype=np.uint8)
        ctypes.memmove(out.ctypes.data, self.ptr[key], nbytes)
        return out

    def free(self):
        for (_, kind), p in self.ptr.items():
            if kind == "device":
                self.shm.free_device(p)
            elif kind == "host":
                self.shm.free(p)


def run_case(shm, c, me, npes, bufs, failures):
    slen, tlen = spans(c)
    sym, loc = ("sym", c["sym"]), ("loc", c["loc"])
    right, left = ((me + 1) % npes, (me + npes - 1) % npes) if c["to"] == "next" else (me, me)
    mine = source_of(me, c["seed"], slen)
    sentinel = np.full(tlen, SENTINEL, dtype=np.uint8)
    if c["op"] == "iput":
        bufs.write(loc, mine)
        bufs.write(sym, sentinel)
        shm.barrier_all()
        shm.iput(c["es"], bufs.ptr[sym], bufs.ptr[loc], c["tst"], c["sst"], c["n"], right)
        shm.barrier_all()
        got, src_after = bufs.read(sym, tlen), bufs.read(loc, slen)
    else:
        bufs.write(sym, mine)
        bufs.write(loc, sentinel)
        shm.barrier_all()
        shm.iget(c["es"], bufs.ptr[loc], bufs.ptr[sym], c["tst"], c["sst"], c["n"], left)
        got = bufs.read(loc, tlen)
        shm.barrier_all()
        src_after = bufs.read(sym, slen)
    want = expected(c, source_of(left, c["seed"], slen))
    if not (got == want).all():
        bad = np.nonzero(got != want)[0]
        failures.append(f"case {c} PE {me}: {bad.size} bytes differ, first at {int(bad[0])}: got {int(got[bad[0]])}, "
                        f"want {int(want[bad[0]])}")
    if not (src_after == mine).all():
        failures.append(f"case {c} PE {me}: the source changed")


def main():
    spec = json.load(open(sys.argv[1]))
    shm = shmem_reduce.Shmem()
    shm.init()
    me, npes = shm.my_pe(), shm.n_pes()
    cases = spec["cases"]
    bufs = Buffers(shm, max(max(spans(c)) for c in cases) + 64)
    failures = []
    for c in cases:
        run_case(shm, c, me, npes, bufs, failures)   # every case, failed or not: the barriers are collective
    shm.barrier_all()
    bufs.free()
    shm.finalize()
    print(json.dumps({"checked": len(cases), "failures": failures[:20]}), flush=True)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
