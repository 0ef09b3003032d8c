#!/usr/bin/env python3
"""One PE of a multi-PE wide-sum test (tests/test_gpu_wide.py): runs the cases
of a spec in order through shmemx_<T>_wsum_to_all / _wsum_to_all_float,
compares its WHOLE target (sentinel tail included) bit for bit with
tests/_wide_ref.py and prints one JSON line {"checked", "failures",
"schedules", "kernels", "digests"}.

usage: _wide_worker.py SPEC.json   (identity from SHMEM_PE / SHMEM_NPES)

A case: {"id", "dtype", "float": bool, "n", "set": [PE_start, logPE_stride,
PE_size], "inplace": bool, "seed"}. Member j's source is
_wide_ref.sources(dtype, PE_size, n, seed)[j]. A "torch" case {"id", "torch":
float16 | bfloat16, "float": bool, "n", "seed"} runs Shmem.wsum_tensors on
heap_tensors over all PEs; a {"id", "rejects": true} case checks the calls
wsum_tensors refuses, which never reach the library.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "osss-gasnet_amd")):
    sys.path.insert(0, p)

import _wide_ref as W  # noqa: E402
import shmem_reduce  # noqa: E402

SENT = 0xA5
TAIL = 24     # elements of the target past the last one reduced


def members(start, logstride, size):
    return [start + i * (1 << logstride) for i in range(size)]


def run_case(shm, c, me, bufs, out):
    mem_pes = members(*c["set"])
    if me not in mem_pes:
        return
    j = mem_pes.index(me)
    dtype, fo, n, inplace = c["dtype"], bool(c["float"]), c["n"], bool(c.get("inplace"))
    oes = 4 if fo else 2
    srcs = W.sources(dtype, *W.gpu_shape(len(mem_pes), n), c["seed"])
    for k in ("s", "t"):
        shm.put(bufs[k], np.full((n + TAIL) * 4, SENT, dtype=np.uint8))
    if n:
        shm.put(bufs["s"], srcs[j])
    t = bufs["s"] if inplace else bufs["t"]
    before = shm.get(t, (n + TAIL) * oes, np.uint8)
    shm.wsum(dtype, fo, t, bufs["s"], n, *c["set"])
    got = shm.get(t, (n + TAIL) * oes, np.uint8)
    tag = (f"case {c['id']} ({dtype} wsum{'_float' if fo else ''} n {n} {'in place' if inplace else 'out of place'} "
           f"set {c['set']}) PE {me}")
    want = W.result(dtype, fo, srcs)
    g = got[:n * oes].view(want.dtype)
    bad = np.flatnonzero(g != want)
    if len(bad):
        i = int(bad[0])
        out["failures"].append(f"{tag}: {len(bad)} of {n} elements differ, first at {i}: got {int(g[i]):#x} want "
                               f"{int(want[i]):#x}")
    if not (got[n * oes:] == before[n * oes:]).all():
        out["failures"].append(f"{tag}: bytes past the target were written")
    if not inplace and n and not (shm.get(bufs["s"], n + TAIL, np.uint16)[:n] == srcs[j]).all():
        out["failures"].append(f"{tag}: the source changed")
    if n and not (shm.get(bufs["s"], (n + TAIL) * 2, np.uint8)[n * 2:] == SENT).all():
        out["failures"].append(f"{tag}: bytes past the source were written")
    info = shm.last_call_info()
    out["schedules"][str(c["id"])] = info["schedule"]
    out["kernels"][str(c["id"])] = info["kernel"]
    if info["schedule"] == "wide-p2p" and n:
        lo, hi = shmem_reduce.shard_bounds(shm.lib, n, 2, len(mem_pes), j)
        if hi > lo and info["alg_bytes"] != (len(mem_pes) * 2 + oes) * (hi - lo):
            out["failures"].append(f"{tag}: alg_bytes {info['alg_bytes']} for a shard of {hi - lo}")
    out["digests"][str(c["id"])] = hashlib.sha256(g.tobytes()).hexdigest()[:16]


def run_torch(shm, c, me, npes, out):
    import torch
    tdt = getattr(torch, c["torch"])
    dtype = shmem_reduce.TORCH_DTYPES[c["torch"]]
    n, fo = c["n"], bool(c["float"])
    srcs = W.sources(dtype, *W.gpu_shape(npes, n), c["seed"])
    x = shm.heap_tensor(n, tdt)
    y = shm.heap_tensor(n, torch.float32 if fo else tdt)
    x.view(torch.int16).copy_(torch.from_numpy(srcs[me].view(np.int16).copy()).to(x.device))
    y.view(torch.int32 if fo else torch.int16).fill_(-1)
    torch.cuda.synchronize()
    shm.wsum_tensors(y, x)
    want = W.result(dtype, fo, srcs)
    got = y.view(torch.int32 if fo else torch.int16).cpu().numpy().view(want.dtype)
    tag = f"case {c['id']} (torch {c['torch']} -> {'float32' if fo else c['torch']}) PE {me}"
    bad = np.flatnonzero(got != want)
    if len(bad):
        out["failures"].append(f"{tag}: {len(bad)} of {n} elements differ, first at {int(bad[0])}")
    out["schedules"][str(c["id"])] = shm.last_call_info()["schedule"]
    out["digests"][str(c["id"])] = hashlib.sha256(got.tobytes()).hexdigest()[:16]
    if not fo:     # out is x: in place
        shm.barrier_all()
        shm.wsum_tensors(x, x)
        got = x.view(torch.int16).cpu().numpy().view(np.uint16)
        if not (got == want).all():
            out["failures"].append(f"{tag}: in place (out is x) differs")
    shm.barrier_all()
    for t in (y, x):
        shm.free_device(t.data_ptr())


def run_rejects(shm, c, me, out):
    """the calls wsum_tensors refuses; none reaches the library, so the PEs stay in step"""
    import torch
    n = 64
    dev = f"cuda:{shm.lib.shmemx_device_id()}"
    x = shm.heap_tensor(n, torch.bfloat16)
    f = shm.heap_tensor(n, torch.float32)
    before = shm.last_call_info()

    def refused(what, exc, call):
        try:
            call()
        except exc:
            return
        except Exception as e:       # noqa: BLE001
            out["failures"].append(f"case {c['id']} PE {me}: {what} raised {type(e).__name__}, not {exc.__name__}")
            return
        out["failures"].append(f"case {c['id']} PE {me}: {what} was not refused")

    # a tensor from torch's allocator, as the source and as the target
    refused("a torch-allocator x", ValueError, lambda: shm.wsum_tensors(f, torch.zeros(n, dtype=torch.bfloat16, device=dev)))
    refused("a torch-allocator out", ValueError, lambda: shm.wsum_tensors(torch.zeros(n, dtype=torch.float32, device=dev), x))
    # a float out that overlaps x: x's 16-bit elements viewed inside the float buffer
    inside = f.view(torch.bfloat16)[n // 2:n // 2 + n]
    refused("a float out that overlaps x", ValueError, lambda: shm.wsum_tensors(f, inside))
    refused("a 16-bit out that overlaps x without being x", ValueError,
            lambda: shm.wsum_tensors(f.view(torch.bfloat16)[:n], f.view(torch.bfloat16)[8:8 + n]))
    # wrong dtype pairs
    h = shm.heap_tensor(n, torch.float16)
    refused("bfloat16 into float16", TypeError, lambda: shm.wsum_tensors(h, x))
    refused("float32 sources", TypeError, lambda: shm.wsum_tensors(f, f))
    refused("bfloat16 into int32", TypeError, lambda: shm.wsum_tensors(f.view(torch.int32), x))
    refused("sizes that differ", ValueError, lambda: shm.wsum_tensors(f[:n - 1], x))
    if shm.last_call_info() != before:
        out["failures"].append(f"case {c['id']} PE {me}: a refused call reached the library")
    out["schedules"][str(c["id"])] = "refused"
    out["digests"][str(c["id"])] = "refused"
    shm.barrier_all()
    for t in (h, f, x):
        shm.free_device(t.data_ptr())


def main():
    spec = json.load(open(sys.argv[1]))
    cases = spec["cases"]
    with_torch = any("torch" in c or "rejects" in c for c in cases)
    if with_torch:
        import torch   # first, as in every torch worker here: one HIP runtime in the process
    shm = shmem_reduce.Shmem()
    shm.init()
    me, npes = shm.my_pe(), shm.n_pes()
    if with_torch:
        torch.cuda.set_device(shm.lib.shmemx_device_id())
    nbytes = (max([c["n"] for c in cases if "dtype" in c] + [0]) + TAIL) * 4 + 64
    bufs = {k: shm.malloc_device(nbytes) for k in ("s", "t")}
    assert all(bufs.values()), bufs
    out = {"checked": 0, "failures": [], "schedules": {}, "kernels": {}, "digests": {}}
    for c in cases:
        if "rejects" in c:
            run_rejects(shm, c, me, out)
        elif "torch" in c:
            run_torch(shm, c, me, npes, out)
        else:
            run_case(shm, c, me, bufs, out)
        out["checked"] += 1
    shm.barrier_all()
    for k in ("t", "s"):
        shm.free_device(bufs[k])
    shm.finalize()
    out["failures"] = out["failures"][:20]
    print(json.dumps(out), flush=True)
    return 1 if out["failures"] else 0


if __name__ == "__main__":
    sys.exit(main())
