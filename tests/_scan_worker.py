#!/usr/bin/env python3
"""One PE of a multi-PE scan test (tests/test_gpu_scan.py): runs the cases of
a spec in order through shmemx_<T>_<op>_inscan / _exscan, compares its WHOLE
target (sentinel tail included) bit for bit with tests/_scan_ref.py and prints
one JSON line {"checked", "failures", "schedules", "digests", "wait_slow"}.

usage: _scan_worker.py SPEC.json   (identity from SHMEM_PE / SHMEM_NPES)

A case: {"id", "op", "dtype", "n", "set": [PE_start, logPE_stride, PE_size],
"excl": bool, "mode": dev | inplace | host | overlap_up | overlap_down, "seed",
"algorithm": auto | p2p | exact | rccl}. Member i's source is
_scan_ref.sources(op, dtype, PE_size, n, seed)[i] (with "inputs": exhaustive |
product, two members of a 16-bit float type: the first n of a and b of that
pair set of tests/_half_ref.py; with "inputs": "paths" and "spacing": member
i's array of tests/_inputs.py paths_source). overlap_up / overlap_down:
the target starts 16 elements above / below the source in one buffer. A
"torch" case {"id", "torch": float32 | bfloat16, "op", "n", "excl", "seed"}
runs Shmem.scan_tensors on heap_tensors over all PEs.
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "osss-gasnet_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import _half_ref  # noqa: E402
import _scan_ref as S  # noqa: E402
import oracle  # noqa: E402
import shmem_reduce  # noqa: E402

SENT = 0xA5
TAIL = 24     # elements of the target past the last one scanned
SHIFT = 16    # elements between target and source in the overlap modes
WRK = 4096    # bytes of pWrk handed in (never written)


def members(start, logstride, size):
    return [start + i * (1 << logstride) for i in range(size)]


def value_bytes(a, dtype):
    if dtype in S.HALF_TYPES:
        return np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return np.ascontiguousarray(oracle.as_value_bytes(a, dtype)).reshape(-1)


class Mem:
    """reads and writes of host (shmem_malloc) or device-heap memory"""

    def __init__(self, shm, host):
        self.shm, self.host = shm, host

    def write(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes == 0:
            return
        if self.host:
            ctypes.memmove(ptr, arr.ctypes.data, arr.nbytes)
        else:
            self.shm.put(ptr, arr)

    def read(self, ptr, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        if nbytes == 0:
            return out
        if self.host:
            ctypes.memmove(out.ctypes.data, ptr, nbytes)
        else:
            self.shm.lib.shmemx_memcpy(out.ctypes.data, ptr, nbytes)
        return out


def run_scan(shm, c, me, bufs, out):
    mem_pes = members(*c["set"])
    if me not in mem_pes:
        return
    j = mem_pes.index(me)
    op, dtype, n, excl, mode = c["op"], c["dtype"], c["n"], bool(c.get("excl")), c["mode"]
    es = np.dtype(S.NP[dtype]).itemsize
    if c.get("inputs") == "paths":   # the directed operand table (tests/_op_paths.py), by member index
        import _inputs
        srcs = [_inputs.paths_source(op, dtype, n, c["spacing"], i) for i in range(len(mem_pes))]
    elif "inputs" in c:  # the 16-bit floats' pair sets: a is member 0's source, b member 1's
        srcs = [s[:n] for s in _half_ref.pair_set(c["inputs"], dtype)]
    else:
        srcs = S.sources(op, dtype, len(mem_pes), n, c["seed"])
    x = srcs[j]
    m = Mem(shm, mode == "host")
    a, b = (bufs["ha"], bufs["hb"]) if mode == "host" else (bufs["da"], bufs["db"])
    if mode == "inplace":
        src = dst = a
    elif mode == "overlap_up":
        src, dst = a, a + SHIFT * es
    elif mode == "overlap_down":
        src, dst = a + SHIFT * es, a
    else:
        src, dst = a, b
    span = (n + TAIL + SHIFT) * es
    m.write(a, np.full(span, SENT, dtype=np.uint8))
    if mode in ("dev", "host"):
        m.write(b, np.full(span, SENT, dtype=np.uint8))
    m.write(src, x)
    before = m.read(dst, (n + TAIL) * es)     # what an untouched target holds
    shm.put(bufs["wrk"], np.full(WRK, SENT, dtype=np.uint8))
    psync = np.full(shmem_reduce.SHMEM_REDUCE_SYNC_SIZE, shmem_reduce.SHMEM_SYNC_VALUE, dtype=np.int64)
    shm.set_algorithm(c.get("algorithm", "auto"))
    shm.scan(op, dtype, dst, src, n, *c["set"], exclusive=excl, pWrk=bufs["wrk"], pSync=psync.ctypes.data)
    got = m.read(dst, (n + TAIL) * es)
    tag = f"case {c['id']} ({dtype} {op} {'exscan' if excl else 'inscan'} n {n} {mode} set {c['set']}) PE {me}"
    want = S.expected(op, dtype, srcs, j, excl)
    if isinstance(want, str):
        assert want == S.UNTOUCHED
        if not (got == before).all():
            out["failures"].append(f"{tag}: exscan wrote member 0's target")
        result = np.zeros(0, dtype=np.uint8)
    else:
        g = got[:n * es].view(S.NP[dtype])
        bad = S.differing(g, want, op, dtype)
        if len(bad):
            i = int(bad[0])
            out["failures"].append(f"{tag}: {len(bad)} of {n} elements differ, first at {i}: got "
                                   f"{g[i:i + 1].tobytes().hex()} want {np.ascontiguousarray(want)[i:i + 1].tobytes().hex()}")
        if not (got[n * es:] == before[n * es:]).all():
            out["failures"].append(f"{tag}: bytes past the target were written")
        result = value_bytes(g, dtype)
    if mode in ("dev", "host"):
        after = m.read(src, n * es)
        if not (after == np.ascontiguousarray(x).view(np.uint8).reshape(-1)).all():
            out["failures"].append(f"{tag}: the source changed")
    if not (psync == shmem_reduce.SHMEM_SYNC_VALUE).all():
        out["failures"].append(f"{tag}: pSync was written")
    if not (shm.get(bufs["wrk"], WRK, np.uint8) == SENT).all():
        out["failures"].append(f"{tag}: pWrk was written")
    out["schedules"][str(c["id"])] = shm.last_call_info()["schedule"]
    out["digests"][str(c["id"])] = hashlib.sha256(result.tobytes()).hexdigest()[:16]


def run_torch(shm, c, me, npes, out):
    import torch
    tdt = getattr(torch, c["torch"])
    dtype = shmem_reduce.TORCH_DTYPES[c["torch"]]
    n, op, excl = c["n"], c["op"], bool(c.get("excl"))
    srcs = S.sources(op, dtype, npes, n, c["seed"])
    x, y = shm.heap_tensor(n, tdt), shm.heap_tensor(n, tdt)
    bits = torch.int16 if dtype in S.HALF_TYPES else torch.int32
    dev = x.device
    x.view(bits).copy_(torch.from_numpy(np.ascontiguousarray(srcs[me]).view(np.int16 if bits == torch.int16 else np.int32).copy()).to(dev))
    y.view(bits).fill_(-1)
    torch.cuda.synchronize()
    shm.scan_tensors(op, y, x, exclusive=excl)
    got = y.view(bits).cpu().numpy()
    want = S.expected(op, dtype, srcs, me, excl)
    tag = f"case {c['id']} (torch {c['torch']} {op} excl {excl}) PE {me}"
    if isinstance(want, str):
        if not (got == -1).all():
            out["failures"].append(f"{tag}: exscan wrote member 0's tensor")
    else:
        bad = S.differing(got.view(S.NP[dtype]), want, op, dtype)
        if len(bad):
            out["failures"].append(f"{tag}: {len(bad)} of {n} elements differ, first at {int(bad[0])}")
    out["schedules"][str(c["id"])] = shm.last_call_info()["schedule"]
    shm.barrier_all()
    for t in (y, x):
        shm.free_device(t.data_ptr())


def main():
    cases = json.load(open(sys.argv[1]))["cases"]
    with_torch = any("torch" in c for c in cases)
    if with_torch:
        import torch   # first, as in every torch worker here: one HIP runtime in the process
    shm = shmem_reduce.Shmem()
    shm.init()
    me, npes = shm.my_pe(), shm.n_pes()
    if with_torch:
        torch.cuda.set_device(shm.lib.shmemx_device_id())
    nbytes = (max([c["n"] for c in cases if "torch" not in c] + [0]) + TAIL + SHIFT) * 16 + 64
    bufs = {"da": shm.malloc_device(nbytes), "db": shm.malloc_device(nbytes), "wrk": shm.malloc_device(WRK),
            "ha": shm.malloc(nbytes), "hb": shm.malloc(nbytes)}
    assert all(bufs.values()), bufs
    out = {"checked": 0, "failures": [], "schedules": {}, "digests": {}, "wait_slow": shm.device_wait_report()[0]}
    for c in cases:
        if "torch" in c:
            run_torch(shm, c, me, npes, out)
        else:
            run_scan(shm, c, me, bufs, out)
        out["checked"] += 1
    shm.barrier_all()
    shm.free(bufs["hb"])
    shm.free(bufs["ha"])
    for k in ("wrk", "db", "da"):
        shm.free_device(bufs[k])
    shm.finalize()
    out["failures"] = out["failures"][:20]
    print(json.dumps(out), flush=True)
    return 1 if out["failures"] else 0


if __name__ == "__main__":
    sys.exit(main())
