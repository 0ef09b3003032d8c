#!/usr/bin/env python3
"""One PE of a data-movement job (tests/_datamove_ref.py holds the model and
the tables): runs batches of put / get / broadcast / fcollect / collect cases
and prints one JSON record.

usage: _datamove_worker.py SPEC.json   (identity from SHMEM_PE / SHMEM_NPES)

SPEC: {"batches": [[case, ...], ...], "second_trip": bool}. A batch is run in
one go: every case owns a guarded slot in each arena it touches (one arena per
kind of memory and role), all slots are filled, one barrier, every call of the
batch back to back with no barrier of the worker's own between them, one
barrier, then each arena is read once, whole, and compared with the model's
image. On a GPU the launch layer's record (last_kernel_name) after every call
says which kernel moved the bytes; a marker kernel (a fetch atomic on this
PE's own word) launched just before the call is what the record still names
when the call launched nothing.

Record: {"pe", "gpu", "fused_max", "failures": [{"id", "pe", "where", "offset"}],
"kernels": [{id: "copy" | "shift" | "fused_pull" | "signal" (the wait kernel of
a host-barrier entry) | "marker" | name}, one per batch], "second_trip":
{"probe_grid", "grid", "total", "kernels", "case"} or null}.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "osss-gasnet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _datamove_ref as ref  # noqa: E402

_vp, _sz, _i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def kernel_class(name):
    for key, cls in (("copy_segments_shift", "shift"), ("copy_segments<", "copy"), ("fused_pull", "fused_pull"),
                     ("amo_one", "marker"), ("signal_only", "signal")):
        if key in name:
            return cls
    return name[:60]


class Arena:
    """`size` bytes of one kind of memory, starting on a 128-byte line"""

    def __init__(self, shm, hip, kind, size):
        self.shm, self.hip, self.kind, self.size = shm, hip, kind, size
        if kind == "dev":
            self.ptr = shm.malloc_device(size)
        elif kind == "host":
            self.ptr = shm.malloc(size)
        elif kind == "hip":
            p = _vp()
            assert hip.hipMalloc(ctypes.byref(p), _sz(size)) == 0
            self.ptr = p.value
        else:
            self.keep = np.empty(size + ref.LINE, dtype=np.uint8)   # plain pageable memory
            self.ptr = self.keep.ctypes.data + (-self.keep.ctypes.data) % ref.LINE
        assert self.ptr and self.ptr % ref.LINE == 0, (kind, self.ptr)

    def write(self, img):
        if self.kind in ("dev", "hip"):
            self.shm.put(self.ptr, img)
        else:
            ctypes.memmove(self.ptr, img.ctypes.data, img.nbytes)

    def read(self):
        if self.kind in ("dev", "hip"):
            return self.shm.get(self.ptr, self.size, np.uint8)
        out = np.empty(self.size, dtype=np.uint8)
        ctypes.memmove(out.ctypes.data, self.ptr, self.size)
        return out

    def free(self):
        if self.kind == "dev":
            self.shm.free_device(self.ptr)
        elif self.kind == "host":
            self.shm.free(self.ptr)
        elif self.kind == "hip":
            self.hip.hipFree(_vp(self.ptr))


def call(shm, c, me, npes, tptr, sptr):
    L = shm.lib
    if c["op"] in ("put", "get"):
        f = shm._typed_fn(c["fn"], None, [_vp, _vp, _sz, _i])
        f(tptr, sptr, c["nelems"], ref.peer_of(c, me, npes))
        return
    start, logstride, size = ref.my_set(c, me)
    if c["op"] == "broadcast":
        f = shm._typed_fn(f"shmem_broadcast{c['bits']}", None, [_vp, _vp, _sz, _i, _i, _i, _i, _vp])
        f(tptr, sptr, c["n"], c["root"] % size, start, logstride, size, shm._psync_ptr)
        return
    f = shm._typed_fn(f"shmem_{c['op']}{c['bits']}", None, [_vp, _vp, _sz, _i, _i, _i, _vp])
    n = c["n"] if c["op"] == "fcollect" else c["counts"][ref.members(start, logstride, size).index(me)]
    f(tptr, sptr, n, start, logstride, size, shm._psync_ptr)


def run_batch(shm, hip, cases, me, npes, gpu, marker=None, grids=None):
    """(failures, {id: kernel class}) of one batch on this PE"""
    sizes, at = ref.layout(cases, npes)
    arena = {name: Arena(shm, hip, name[1:], sizes[name]) for name in sorted(sizes)}   # collective: the same order everywhere
    want = {name: np.full(sizes[name], ref.SENT_T if name[0] == "T" else ref.SENT_S, dtype=np.uint8) for name in sizes}
    init = {name: w.copy() for name, w in want.items()}
    for c in cases:
        ta, sa = ref.arenas(c, me)
        nb = ref.slot_bytes(c, npes)
        wt, ws = ref.images(c, npes, me)
        so = at[(sa, c["id"])]
        init[sa][so:so + nb] = ws
        want[sa][so:so + nb] = ws
        if ta != sa:
            want[ta][at[(ta, c["id"])]:at[(ta, c["id"])] + nb] = wt
    for name, a in arena.items():
        a.write(init[name])
    shm.barrier_all()
    kernels = {}
    for c in cases:
        if c["op"] not in ("put", "get") and ref.my_set(c, me) is None:
            continue
        ta, sa = ref.arenas(c, me)
        tp, sp = ref.phases(c)
        tptr = arena[ta].ptr + at[(ta, c["id"])] + ref.GUARD + tp
        sptr = arena[sa].ptr + at[(sa, c["id"])] + ref.GUARD + sp
        if gpu:
            shm.atomic("fetch", "long", marker, me)
        call(shm, c, me, npes, tptr, sptr)
        if gpu:
            kernels[str(c["id"])] = kernel_class(shm.last_kernel_name())
            if grids is not None:
                grids[str(c["id"])] = list(shm.last_launch_grid())
    shm.barrier_all()
    failures = []
    got = {name: a.read() for name, a in arena.items()}
    for name in sizes:
        if (got[name] == want[name]).all():
            continue
        for c in cases:   # which case, and where
            ta, sa = ref.arenas(c, me)
            if name not in (ta, sa):
                continue
            nb = ref.slot_bytes(c, npes)
            to, so = at[(ta, c["id"])], at[(sa, c["id"])]
            d = ref.first_difference(c, npes, me, got.get(ta, want[ta])[to:to + nb], got.get(sa, want[sa])[so:so + nb],
                                     want[ta][to:to + nb], want[sa][so:so + nb])
            if d is not None and d not in failures:
                failures.append(d)
    for name in sorted(arena, reverse=True):
        arena[name].free()
    return failures, kernels


def second_trip(shm, hip, me, npes, marker):
    """An fcollect whose fused_pull blocks each make a second trip: the grid
    is read back from a first launch near the size wanted, and the case is
    sized one element above 4,096 bytes x that grid."""
    fused_max = shm.thresholds()[0]

    def fc(cid, total):
        return {"id": cid, "op": "fcollect", "bits": 64, "n": total // (8 * npes), "sets": [[0, 0, npes]], "toff": 8,
                "soff": 0, "sym": "dev", "tgt": "dev"}

    grids = {}
    probe = fc(0, min(fused_max, 1 << 20))
    failures, k0 = run_batch(shm, hip, [probe], me, npes, True, marker, grids)
    grid = grids["0"][0]
    case = fc(1, 4096 * grid + 8 * npes)
    f2, k1 = run_batch(shm, hip, [case], me, npes, True, marker, grids)
    return failures + f2, {"probe_grid": grids["0"], "grid": grids["1"], "total": case["n"] * 8 * npes,
                           "kernels": [k0["0"], k1["1"]], "case": case}


def run(shm, spec, gpu):
    me, npes = shm.my_pe(), shm.n_pes()
    hip = ctypes.CDLL("libamdhip64.so") if gpu else None
    marker = shm.malloc_device(256) if gpu else None
    rec = {"pe": me, "gpu": gpu, "fused_max": shm.thresholds()[0] if gpu else None, "failures": [], "kernels": [],
           "second_trip": None}
    for cases in spec["batches"]:
        failures, kernels = run_batch(shm, hip, cases, me, npes, gpu, marker)
        rec["failures"] += failures
        rec["kernels"].append(kernels)
    if spec.get("second_trip"):
        failures, rec["second_trip"] = second_trip(shm, hip, me, npes, marker)
        rec["failures"] += failures
    if gpu:
        shm.free_device(marker)
    return rec


def main():
    import shmem_reduce
    spec = json.load(open(sys.argv[1]))
    gpu = os.environ.get("SHMEM_BOOTSTRAP_ONLY") != "1"
    shm = shmem_reduce.Shmem()
    shm.init()
    rec = run(shm, spec, gpu)
    shm.finalize()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
