#!/usr/bin/env python3
"""One PE of a multi-PE 16-bit float reduction test (tests/test_gpu_half.py):
runs the cases of a spec in order through the public shmemx_half_* /
shmemx_bfloat16_* calls, compares its WHOLE target (sentinel-filled tail
included) bit for bit with the model (tests/_half_ref.py) and prints one JSON
line {"checked", "failures", "schedules"}.

usage: _half_worker.py SPEC.json   (identity from SHMEM_PE / SHMEM_NPES)

A case: {"id", "op", "dtype", "n", "set": [PE_start, logPE_stride, PE_size],
"mode": dev | inplace | host, "order": reference | pe_start, "algorithm":
auto | p2p | exact | rccl, "stream": bool, "seed"}. Member i's source is
_half_ref.sources(dtype, PE_size, n, seed)[i], or with "inputs": exhaustive |
product (two members) the first n of a (member 0) and b (member 1) of that
pair set (_half_ref.PAIR_SETS). A "torch" case: {"id", "torch":
float16 | bfloat16, "op", "n", "heap": bool, "seed"} reduces torch tensors over
all PEs -- from the caching allocator through to_all_tensors, or (heap) a
heap_tensor through the stream-ordered call.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "osss-gasnet_amd"))

import _half_ref as R  # noqa: E402
import shmem_reduce  # noqa: E402

SENT = 0xA5A5
TAIL = 24   # elements of the target past the last one reduced


def members(start, logstride, size):
    return [start + i * (1 << logstride) for i in range(size)]


def expected(c, dtype, srcs, me_index):
    if c.get("order", "reference") == "pe_start":
        return R.fold(c["op"], dtype, srcs, 0)
    return R.fold(c["op"], dtype, srcs, me_index)


def report(failures, c, me, got, want):
    if got.shape == want.shape and (got == want).all():
        return
    bad = np.nonzero(got != want)[0]
    i = int(bad[0])
    failures.append(f"case {c} PE {me}: {bad.size} of {want.size} elements differ, first at {i}: "
                    f"got {int(got[i]):#06x}, want {int(want[i]):#06x}")


def run_reduce(shm, c, me, bufs, failures, schedules):
    mem = members(*c["set"])
    if me not in mem:
        return
    op, dtype, n = c["op"], c["dtype"], c["n"]
    if "inputs" in c:
        assert len(mem) == 2, c
        srcs = [s[:n] for s in R.pair_set(c["inputs"], dtype)]
    else:
        srcs = R.sources(dtype, len(mem), n, c["seed"])
    x = srcs[mem.index(me)]
    mode = c["mode"]
    host = mode == "host"
    a, b = (bufs["ha"], bufs["hb"]) if host else (bufs["da"], bufs["db"])
    src, dst = (a, a) if mode == "inplace" else (a, b)
    sent = np.full(n + TAIL, SENT, dtype=np.uint16)

    def write(ptr, arr):
        if host:
            ctypes.memmove(ptr, arr.ctypes.data, arr.nbytes)
        else:
            shm.put(ptr, arr)

    write(dst, sent)
    if src != dst:
        write(src, sent)
    if n:
        write(src, x)
    # a case without "algorithm" runs what the job's environment selected
    shm.set_algorithm(c.get("algorithm", os.environ.get("SHMEM_REDUCE_ALGORITHM", "auto")))
    shm.set_order(c.get("order", "reference"))
    if c.get("stream"):
        st = shm.stream_create()
        shm.to_all_on_stream(op, dtype, dst, src, n, *c["set"], st)
        shm.stream_sync(st)
        shm.stream_destroy(st)
    else:
        shm.to_all(op, dtype, dst, src, n, *c["set"])
    if host:
        got = np.empty(n + TAIL, dtype=np.uint16)
        ctypes.memmove(got.ctypes.data, dst, got.nbytes)
    else:
        got = shm.get(dst, n + TAIL, np.uint16)
    want = np.concatenate([expected(c, dtype, srcs, mem.index(me)), sent[n:]])
    report(failures, c, me, got, want)
    if src != dst:   # the source is left alone
        if host:
            after = np.empty(n, dtype=np.uint16)
            ctypes.memmove(after.ctypes.data, src, after.nbytes)
        else:
            after = shm.get(src, n, np.uint16)
        if not (after == x).all():
            failures.append(f"case {c} PE {me}: the source changed")
    if n and not c.get("stream"):
        schedules[str(c["id"])] = shm.last_call_info()["schedule"]


def run_torch(shm, c, me, npes, failures, schedules):
    import torch
    tdt = getattr(torch, c["torch"])
    dtype = shmem_reduce.TORCH_DTYPES[c["torch"]]
    n, op = c["n"], c["op"]
    srcs = R.sources(dtype, npes, n, c["seed"])
    dev = f"cuda:{shm.lib.shmemx_device_id()}"
    mine = torch.from_numpy(srcs[me].view(np.int16).copy()).to(dev).view(tdt)
    shm.set_algorithm("auto")
    shm.set_order("reference")
    if c.get("heap"):
        x, out = shm.heap_tensor(n, tdt), shm.heap_tensor(n, tdt)
        if x.dtype != tdt or x.numel() != n:
            failures.append(f"case {c} PE {me}: heap_tensor gave {x.dtype} x {x.numel()}")
        x.copy_(mine)
        out.view(torch.int16).fill_(-1)
        torch.cuda.synchronize()
        st = shm.stream_create()
        shm.to_all_on_stream(op, dtype, out.data_ptr(), x.data_ptr(), n, 0, 0, npes, st)
        shm.stream_sync(st)
        shm.stream_destroy(st)
    else:
        x, out = mine, torch.empty(n, dtype=tdt, device=dev)
        out.view(torch.int16).fill_(-1)
        torch.cuda.synchronize()
        shm.to_all_tensors(op, out, x)
        schedules[str(c["id"])] = shm.last_call_info()["schedule"]
    got = out.view(torch.int16).cpu().numpy().view(np.uint16)
    report(failures, c, me, got, R.fold(op, dtype, srcs, me))
    if c.get("heap"):
        shm.barrier_all()
        for t in (out, x):
            shm.free_device(t.data_ptr())


def main():
    spec = json.load(open(sys.argv[1]))
    cases = spec["cases"]
    with_torch = any("torch" in c for c in cases)
    if with_torch:
        # torch first, as in every torch worker here: its wheel carries a HIP
        # runtime of its own, and the library must bind to that one copy, not
        # bring a second one into the process
        import torch
    shm = shmem_reduce.Shmem()
    shm.init()
    me, npes = shm.my_pe(), shm.n_pes()
    if with_torch:
        torch.cuda.set_device(shm.lib.shmemx_device_id())
    nbytes = (max(c["n"] for c in cases) + TAIL) * 2 + 64
    bufs = {"da": shm.malloc_device(nbytes), "db": shm.malloc_device(nbytes),
            "ha": shm.malloc(nbytes), "hb": shm.malloc(nbytes)}
    assert all(bufs.values()), bufs
    failures, schedules = [], {}
    for c in cases:
        if "torch" in c:
            run_torch(shm, c, me, npes, failures, schedules)
        else:
            run_reduce(shm, c, me, bufs, failures, schedules)
    shm.barrier_all()
    ext = shm.external_map_stats()
    shm.free(bufs["hb"])
    shm.free(bufs["ha"])
    shm.free_device(bufs["db"])
    shm.free_device(bufs["da"])
    shm.finalize()
    print(json.dumps({"checked": len(cases), "failures": failures[:20], "schedules": schedules,
                      "external_map_opened": ext[1]}), flush=True)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
