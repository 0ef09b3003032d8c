#!/usr/bin/env python3
"""All-to-all measurements with the PEs sharing one GPU (the
all-to-all section). Run one process per PE:

    tools/oshrun -np 4 --same-device python3 tools/alltoall_bench.py [--out FILE] [--legs a,b,c]

PE 0 writes one JSON file (default profiles/alltoall/one_gpu.json). No xGMI
link is involved: every "peer" source is this GPU's own memory.

Legs
  contig   shmem_alltoall64 against shmem_fcollect64, the same bytes into
           every PE (64 MiB): seconds per call on the host clock, between
           job-wide barriers, warm (one buffer pair) and cold (rotating over
           three pairs, 1.5 GiB of traffic between two uses of a buffer in a
           4-PE job); and the all-to-all's copy kernel alone
           (shmemx_kernel_timing: the launch's own start/stop stamps)
  strided  shmem_alltoalls64 at strides (dst, sst) (1,1) (1,2) (2,1) (2,2)
           (1,16), 16 MiB of elements into every PE: kernel time, useful
           bytes per second, the fraction of the (1,1) rate, and the share of
           each fetched or written 128-byte line that is useful
  small    4 KiB per peer block: one fused launch against barrier + copy
           kernel + barrier (the fused limit set to 0), microseconds per call
--legs fcollect runs only the fcollect half of `contig` (a library built from
a commit without all-to-all: SHMEM_REDUCE_LIBDIR); the committed file holds
that run of the parent commit under "parent_commit_fcollect".

Every figure is a median over `--reps` samples with min and max beside it;
the first `--warmup` calls of a leg are not counted.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "osss-gasnet_amd"))
import shmem_reduce  # noqa: E402

MIB = 1 << 20


def spread(xs, scale=1.0, digits=2):
    return {"median": round(statistics.median(xs) * scale, digits), "min": round(min(xs) * scale, digits),
            "max": round(max(xs) * scale, digits), "samples": len(xs)}


def host_times(shm, call, reps, warmup, inner=1):
    """seconds per call, each sample between two job-wide barriers"""
    for k in range(warmup):
        call(k)
    out = []
    for r in range(reps):
        shm.barrier_all()
        t0 = time.perf_counter()
        for k in range(inner):
            call(r * inner + k)
        shm.barrier_all()
        out.append((time.perf_counter() - t0) / inner)
    return out


def kernel_times(shm, call, reps, warmup):
    """milliseconds of the call's timed kernel(s), one sample per call"""
    for k in range(warmup):
        call(k)
    out = []
    for r in range(reps):
        shm.kernel_timing(True)
        call(r)
        launches, total_ms, _ = shm.kernel_timing_stats()
        shm.kernel_timing(False)
        if launches:
            out.append(total_ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alltoall", "one_gpu.json"))
    ap.add_argument("--legs", default="contig,strided,small")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    legs = args.legs.split(",")
    os.environ.setdefault("SHMEM_DEVICE_HEAP_SIZE", "1100M")
    os.environ.setdefault("SHMEM_DEVICE_SCRATCH_SIZE", "24M")
    os.environ.setdefault("SHMEM_THRESHOLD_CALIBRATE", "0")   # the default thresholds, not this run's timing
    shm = shmem_reduce.Shmem()
    shm.init()
    me, npes = shm.my_pe(), shm.n_pes()
    L = shm.lib
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.shmem_fcollect64.argtypes = [vp, vp, sz, i, i, i, vp]
    ps = shm._psync_ptr
    rec = {"npes": npes, "layout": "every PE on one GPU: no xGMI link in any figure", "reps": args.reps,
           "warmup": args.warmup, "library": os.path.relpath(shmem_reduce.LIB_PATH, ROOT), "kernel_code_hash": shmem_reduce.kernel_code_hash()}

    if "contig" in legs or "fcollect" in legs:
        total = 64 * MIB                      # bytes into every PE
        blk = total // npes                   # per peer block
        pairs = [(shm.malloc_device(total), shm.malloc_device(total)) for _ in range(3)]
        leg = {"bytes_into_each_pe": total, "block_bytes": blk}

        def fcollect(k, rot=False):
            s, t = pairs[k % 3 if rot else 0]
            L.shmem_fcollect64(t, s, blk // 8, 0, 0, npes, ps)

        def alltoall(k, rot=False):
            s, t = pairs[k % 3 if rot else 0]
            shm.alltoall(64, t, s, blk // 8)

        names = [("fcollect64", fcollect)] + ([("alltoall64", alltoall)] if "contig" in legs else [])
        for name, f in names:
            for mode, rot in (("warm", False), ("cold", True)):
                ts = host_times(shm, lambda k: f(k, rot), args.reps, args.warmup)
                leg[f"{name}_{mode}_us_per_call"] = spread(ts, 1e6, 1)
                leg[f"{name}_{mode}_GB_s_into_each_pe"] = round(total / statistics.median(ts) / 1e9, 1)
        if "contig" in legs:
            for mode, rot in (("warm", False), ("cold", True)):
                ks = kernel_times(shm, lambda k: alltoall(k, rot), args.reps, args.warmup)
                leg[f"alltoall64_{mode}_kernel_us"] = spread(ks, 1e3, 1)
                leg[f"alltoall64_{mode}_kernel_GB_s"] = round(total / (statistics.median(ks) * 1e-3) / 1e9, 1)
        rec["contig"] = leg
        for s, t in reversed(pairs):
            shm.free_device(t)
            shm.free_device(s)

    if "strided" in legs:
        useful = 16 * MIB
        n = useful // 8 // npes               # elements per peer block
        smax = 16
        src = shm.malloc_device(useful * smax)
        tgt = shm.malloc_device(useful * 2)
        leg = {"useful_bytes_into_each_pe": useful, "elem_bytes": 8, "nelems_per_block": n}
        base = None
        for dst, sst in [(1, 1), (1, 2), (2, 1), (2, 2), (1, 16)]:
            ks = kernel_times(shm, lambda k: shm.alltoalls(64, tgt, src, dst, sst, n), args.reps, args.warmup)
            med = statistics.median(ks) * 1e-3
            rate = useful / med / 1e9
            if base is None:
                base = rate
            per_line = 128 // 8
            leg[f"dst{dst}_sst{sst}"] = {
                "kernel_us": spread(ks, 1e3, 1), "useful_GB_s": round(rate, 1),
                "fraction_of_contiguous": round(rate / base, 3),
                "useful_share_of_read_lines": round(max(1.0 / sst, 1.0 / per_line), 4),
                "useful_share_of_written_lines": round(max(1.0 / dst, 1.0 / per_line), 4),
                "line_bytes_touched_GB_s": round(rate * (min(sst, per_line) + min(dst, per_line)), 1)}
        rec["strided"] = leg
        shm.free_device(tgt)
        shm.free_device(src)

    if "small" in legs:
        blk = 4096
        src = shm.malloc_device(blk * npes)
        tgt = shm.malloc_device(blk * npes)
        leg = {"block_bytes": blk}
        old = shm.set_fused_max(1 << 20)
        for name, limit in (("fused_one_launch", 1 << 20), ("barrier_copy_barrier", 0)):
            shm.set_fused_max(limit)
            shm.barrier_all()
            ts = host_times(shm, lambda k: shm.alltoall(64, tgt, src, blk // 8), args.reps, args.warmup, inner=200)
            leg[f"{name}_us_per_call"] = spread(ts, 1e6, 2)
        shm.set_fused_max(old)
        rec["small"] = leg
        shm.free_device(tgt)
        shm.free_device(src)

    shm.barrier_all()
    if me == 0:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps(rec), flush=True)
    shm.finalize()


if __name__ == "__main__":
    main()
