#!/usr/bin/env python3
"""One PE of a multi-PE value-and-location test (tests/test_gpu_loc.py): runs
the cases of a spec in order through shmemx_<T>_maxloc_to_all / _minloc_to_all,
compares its WHOLE target and target_loc (sentinel tails included) bit for bit
with tests/_loc_ref.py and prints one JSON line {"checked", "failures",
"schedules", "digests", "rules"}.

usage: _loc_worker.py SPEC.json   (identity from SHMEM_PE / SHMEM_NPES)

A case: {"id", "op": max | min, "dtype", "n", "set": [PE_start, logPE_stride,
PE_size], "inplace": bool, "explicit": bool, "seed"}. Member j's arrays are
_loc_ref.inputs(dtype, PE_size, n, seed)[.][j]; with "explicit" false the call
passes source_loc = NULL. A "torch" case {"id", "torch": float32 | bfloat16 |
int64, "op", "n", "explicit", "seed"} runs Shmem.loc_to_all_tensors on
heap_tensors over all PEs.

"rules": per type class, how many (element, step) pairs of the explicit cases
exercised each rule of the model -- counted on the model alone. With
"require_rules" in the spec a zero count is a failure: the inputs would not
test what they are there for.
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

import _loc_ref as L  # noqa: E402
import shmem_reduce  # noqa: E402

SENT = 0xA5
TAIL = 24     # elements of each target past the last one reduced


def members(start, logstride, size):
    return [start + i * (1 << logstride) for i in range(size)]


def klass(dtype):
    return "float" if dtype in L.FLOATS else "int"


def run_case(shm, c, me, bufs, out):
    mem_pes = members(*c["set"])
    if me not in mem_pes:
        return
    j = mem_pes.index(me)
    op, dtype, n, inplace, explicit = c["op"], c["dtype"], c["n"], bool(c.get("inplace")), bool(c.get("explicit", True))
    st = np.dtype(L.STORE[dtype])
    es = st.itemsize
    vals, locs = L.inputs(dtype, len(mem_pes), n, c["seed"])
    for k in ("sv", "sl", "tv", "tl"):
        shm.put(bufs[k], np.full((n + TAIL) * 8, SENT, dtype=np.uint8))
    if n:
        shm.put(bufs["sv"], vals[j])
        shm.put(bufs["sl"], locs[j])
    # in place needs target_loc == source_loc, so the locations are explicit there
    tv, tl = (bufs["sv"], bufs["sl"]) if inplace else (bufs["tv"], bufs["tl"])
    before_v = shm.get(tv, (n + TAIL) * es, np.uint8)
    before_l = shm.get(tl, (n + TAIL) * 8, np.uint8)
    shm.loc_to_all(op, dtype, tv, tl, bufs["sv"], bufs["sl"] if explicit else None, n, *c["set"])
    got_v = shm.get(tv, (n + TAIL) * es, np.uint8)
    got_l = shm.get(tl, (n + TAIL) * 8, np.uint8)
    tag = (f"case {c['id']} ({dtype} {op}loc n {n} {'in place' if inplace else 'out of place'} "
           f"{'explicit' if explicit else 'NULL'} set {c['set']}) PE {me}")
    counts = out["rules"][klass(dtype)] if explicit else None
    want_v, want_l = L.fold(op, dtype, vals, locs if explicit else None, counts=counts)
    gv, gl = got_v[:n * es].view(st), got_l[:n * 8].view(np.int64)
    bad = np.flatnonzero((gv != want_v) | (gl != want_l))
    if len(bad):
        i = int(bad[0])
        out["failures"].append(f"{tag}: {len(bad)} of {n} pairs differ, first at {i}: got ({gv[i:i + 1].tobytes().hex()}, "
                               f"{int(gl[i])}) want ({want_v[i:i + 1].tobytes().hex()}, {int(want_l[i])})")
    if not ((got_v[n * es:] == before_v[n * es:]).all() and (got_l[n * 8:] == before_l[n * 8:]).all()):
        out["failures"].append(f"{tag}: bytes past a target were written")
    if not inplace:
        if n and not ((shm.get(bufs["sv"], n, st) == vals[j]).all() and
                      (shm.get(bufs["sl"], n, np.int64) == locs[j]).all()):
            out["failures"].append(f"{tag}: a source changed")
    info = shm.last_call_info()
    out["schedules"][str(c["id"])] = info["schedule"]
    out["kernels"][str(c["id"])] = info["kernel"]
    if info["schedule"].startswith("loc-p2p") and n:
        lo, hi = shmem_reduce.shard_bounds(shm.lib, n, es, len(mem_pes), j)
        if hi > lo and info["alg_bytes"] != (len(mem_pes) + 1) * (es + 8) * (hi - lo):
            out["failures"].append(f"{tag}: alg_bytes {info['alg_bytes']} for a shard of {hi - lo}")
    out["digests"][str(c["id"])] = hashlib.sha256(gv.tobytes() + gl.tobytes()).hexdigest()[:16]


def run_torch(shm, c, me, npes, out):
    import torch
    tdt = getattr(torch, c["torch"])
    dtype = shmem_reduce.TORCH_DTYPES[c["torch"]]
    n, op, explicit = c["n"], c["op"], bool(c.get("explicit", True))
    vals, locs = L.inputs(dtype, npes, n, c["seed"])
    x, y = shm.heap_tensor(n, tdt), shm.heap_tensor(n, tdt)
    xi, yi = shm.heap_tensor(n, torch.int64), shm.heap_tensor(n, torch.int64)
    bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]
    npbits = {2: np.int16, 4: np.int32, 8: np.int64}[x.element_size()]
    x.view(bits).copy_(torch.from_numpy(vals[me].view(npbits).copy()).to(x.device))
    xi.copy_(torch.from_numpy(locs[me].copy()).to(x.device))
    y.view(bits).fill_(-1)
    yi.fill_(-1)
    torch.cuda.synchronize()
    shm.loc_to_all_tensors(op, y, yi, x, xi if explicit else None)
    want_v, want_l = L.fold(op, dtype, vals, locs if explicit else None)
    got_v = y.view(bits).cpu().numpy().view(L.STORE[dtype])
    got_l = yi.cpu().numpy()
    tag = f"case {c['id']} (torch {c['torch']} {op}loc explicit {explicit}) PE {me}"
    bad = np.flatnonzero((got_v != want_v) | (got_l != want_l))
    if len(bad):
        out["failures"].append(f"{tag}: {len(bad)} of {n} pairs differ, first at {int(bad[0])}")
    out["schedules"][str(c["id"])] = shm.last_call_info()["schedule"]
    shm.barrier_all()
    for t in (yi, xi, y, x):
        shm.free_device(t.data_ptr())


def main():
    spec = json.load(open(sys.argv[1]))
    cases = spec["cases"]
    with_torch = any("torch" in c for c in cases)
    if with_torch:
        import torch   # first, as in every torch worker here: one HIP runtime in the process
    shm = shmem_reduce.Shmem()
    shm.init()
    me, npes = shm.my_pe(), shm.n_pes()
    if with_torch:
        torch.cuda.set_device(shm.lib.shmemx_device_id())
    nbytes = (max([c["n"] for c in cases if "torch" not in c] + [0]) + TAIL) * 8 + 64
    bufs = {k: shm.malloc_device(nbytes) for k in ("sv", "sl", "tv", "tl")}
    assert all(bufs.values()), bufs
    out = {"checked": 0, "failures": [], "schedules": {}, "kernels": {}, "digests": {},
           "rules": {"float": {}, "int": {}}}
    for c in cases:
        if "torch" in c:
            run_torch(shm, c, me, npes, out)
        else:
            run_case(shm, c, me, bufs, out)
        out["checked"] += 1
    shm.barrier_all()
    for k in ("tl", "tv", "sl", "sv"):
        shm.free_device(bufs[k])
    shm.finalize()
    if spec.get("require_rules"):
        for kl, names in (("float", L.RULES_FLOAT), ("int", L.RULES_INT)):
            for rule in names:
                if out["rules"][kl].get(rule, 0) == 0:
                    out["failures"].append(f"the inputs never exercised rule {rule} for the {kl} types: "
                                           f"{out['rules'][kl]}")
    out["failures"] = out["failures"][:20]
    print(json.dumps(out), flush=True)
    return 1 if out["failures"] else 0


if __name__ == "__main__":
    sys.exit(main())
