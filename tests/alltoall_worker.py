#!/usr/bin/env python3
"""One PE of a multi-PE all-to-all test (tests/test_gpu_alltoall.py): runs the
cases of a spec in order and saves what its target holds after each.

usage: alltoall_worker.py SPEC.json OUTDIR   (identity from SHMEM_PE / SHMEM_NPES)

A case: {"id", "kind": alltoall | alltoalls | fcollect | sum, "bits", "n",
"dst", "sst", "sets", "target": device | host | pageable | mixed, "source":
device | host, "seed", "slen", "tlen"}; slen / tlen are the elements of the
source filled and of the target read back (sentinel -7 first). "report_grid":
also save mi355_last_launch_grid after the call, as "grid<id>", and that
kernel's name, as "kernel<id>".
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

SENTINEL = -7


def members(start, logstride, size):
    return [start + i * (1 << logstride) for i in range(size)]


def source_of(pe, n, bits, seed):
    """PE pe's source array of a case (the test computes the same)."""
    rng = np.random.default_rng(seed * 1009 + pe)
    if bits == 32:
        return rng.integers(-2**20, 2**20, n, dtype=np.int32)
    return rng.integers(-2**62, 2**62, n, dtype=np.int64)


def run_case(shm, c, me, bufs, results):
    mine = None
    for s in c["sets"]:
        if me in members(*s):
            mine = s
    if mine is None:
        return
    bits, n = c["bits"], c["n"]
    dt = np.int32 if bits == 32 else np.int64
    slen, tlen = c["slen"], c["tlen"]
    kt = c.get("target", "device")
    if kt == "mixed":  # pageable host target on odd PEs, device on even ones
        kt = "pageable" if me % 2 else "device"
    pageable = np.empty(tlen * 8 + 64, dtype=np.uint8)
    tgt = {"device": bufs["db"], "host": bufs["hb"], "pageable": pageable.ctypes.data + 8}[kt]
    sentinel = np.full(tlen, SENTINEL, dtype=dt)
    if kt == "device":
        shm.put(tgt, sentinel)
    else:
        ctypes.memmove(tgt, sentinel.ctypes.data, sentinel.nbytes)
    x = source_of(me, slen, bits, c["seed"])
    if c.get("source", "device") == "host":
        src = bufs["ha"]
        ctypes.memmove(src, x.ctypes.data, x.nbytes)
    else:
        src = bufs["da"]
        if slen:
            shm.put(src, x)
    kind = c["kind"]
    if kind == "alltoall":
        shm.alltoall(bits, tgt, src, n, *mine)
    elif kind == "alltoalls":
        shm.alltoalls(bits, tgt, src, c["dst"], c["sst"], n, *mine)
    elif kind == "fcollect":
        f = getattr(shm.lib, f"shmem_fcollect{bits}")
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_int] * 3 + [ctypes.c_void_p]
        f(tgt, src, n, *mine, shm._psync_ptr)
    elif kind == "sum":
        shm.to_all("sum", "int", tgt, src, n, *mine)
    else:
        raise ValueError(kind)
    if c.get("report_grid"):
        # the grid of the strided kernel this PE just launched (the test's pass rule)
        results[f"grid{c['id']}"] = np.array(shm.last_launch_grid())
        results[f"kernel{c['id']}"] = np.array([shm.last_kernel_name()])
    if kt == "device":
        got = shm.get(tgt, tlen, dt)
    else:
        got = np.empty(tlen, dtype=dt)
        ctypes.memmove(got.ctypes.data, tgt, got.nbytes)
    results[str(c["id"])] = got


def main():
    spec = json.load(open(sys.argv[1]))
    outdir = sys.argv[2]
    shm = shmem_reduce.Shmem()
    shm.init()
    me = shm.my_pe()
    cases = spec["cases"]
    def most(key, where=lambda c: True):
        """bytes of the largest source (slen) or target (tlen) among the cases `where` picks"""
        return max([c[key] * c["bits"] // 8 for c in cases if where(c)] + [8]) + 64

    off = spec.get("offset", 0)  # bytes off the allocations' alignment, both symmetric
    # the host-heap buffers only as large as the cases that use them
    bufs = {"da": shm.malloc_device(most("slen")) + off, "db": shm.malloc_device(most("tlen")) + off,
            "ha": shm.malloc(most("slen", lambda c: c.get("source", "device") == "host")) + off,
            "hb": shm.malloc(most("tlen", lambda c: c.get("target", "device") == "host")) + off}
    assert all(v > off for v in bufs.values()), bufs
    results = {}
    for c in cases:
        run_case(shm, c, me, bufs, results)
    assert (shm._psync == shmem_reduce.SHMEM_SYNC_VALUE).all(), "pSync was written"
    shm.barrier_all()
    np.savez(os.path.join(outdir, f"pe{me}.npz"), **results)
    for k, dev in (("db", True), ("da", True), ("hb", False), ("ha", False)):
        (shm.free_device if dev else shm.free)(bufs[k] - off)
    shm.finalize()


if __name__ == "__main__":
    main()
