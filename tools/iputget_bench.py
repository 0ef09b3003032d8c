#!/usr/bin/env python3
"""Strided get measurements on one PE (the strided put/get
paragraph):

    python3 tools/iputget_bench.py [--out FILE]

shmem_iget of 16 MiB of useful bytes from this PE's own device heap into it,
element sizes 1, 2, 4, 8 and 16 bytes x strides (tst, sst) (1,2) (2,1) (2,2)
(1,16): the time of the strided kernel alone (shmemx_kernel_timing: the
launch's own start/stop stamps), useful bytes per second, and the fraction of
the contiguous copy of the same bytes (strides (1,1): mi355_copy_segments),
measured in the same run. A put to this PE runs the same kernel on the same
pointers, so the get stands for both. No xGMI link is involved.

Every figure is a median over `--reps` samples with min and max beside it; the
first `--warmup` calls of a row are not counted. Rows are taken in an
interleaved order (every row once per round) so that drift over the run
spreads over all of them. Every row reads and writes the start of the same
two buffers, so the rates are warm: the rows of strides up to 2 touch at most
64 MiB, inside the 256 MiB Infinity Cache; only the stride-16 source (256 MiB)
does not fit.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "osss-gasnet_amd"))
import shmem_reduce  # noqa: E402

MIB = 1 << 20
SIZES = [1, 2, 4, 8, 16]
STRIDES = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 16)]


def spread(xs, scale=1.0, digits=2):
    return {"median": round(statistics.median(xs) * scale, digits), "min": round(min(xs) * scale, digits),
            "max": round(max(xs) * scale, digits), "samples": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iputget", "one_gpu.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    os.environ.setdefault("SHMEM_DEVICE_HEAP_SIZE", "400M")
    os.environ.setdefault("SHMEM_DEVICE_SCRATCH_SIZE", "3M")
    os.environ.setdefault("SHMEM_THRESHOLD_CALIBRATE", "0")
    shm = shmem_reduce.Shmem()
    shm.init()
    useful = 16 * MIB
    src = shm.malloc_device(useful * 16)
    tgt = shm.malloc_device(useful * 2)
    rows = [(es, tst, sst) for es in SIZES for tst, sst in STRIDES]
    samples = {r: [] for r in rows}

    def timed(es, tst, sst):
        shm.kernel_timing(True)
        shm.iget(es, tgt, src, tst, sst, useful // es, 0)
        launches, total_ms, _ = shm.kernel_timing_stats()
        shm.kernel_timing(False)
        return total_ms if launches else None

    for rnd in range(args.warmup + args.reps):
        for r in rows:
            ms = timed(*r)
            if rnd >= args.warmup and ms is not None:
                samples[r].append(ms)

    rec = {"npes": 1, "layout": "one PE, source and target in its own device heap: no xGMI link in any figure",
           "useful_bytes": useful, "reps": args.reps, "warmup": args.warmup,
           "library": os.path.relpath(shmem_reduce.LIB_PATH, ROOT), "kernel_code_hash": shmem_reduce.kernel_code_hash(),
           "rows": {}}
    for es in SIZES:
        base = useful / (statistics.median(samples[(es, 1, 1)]) * 1e-3) / 1e9
        per_line = 128 // es
        for tst, sst in STRIDES:
            ks = samples[(es, tst, sst)]
            rate = useful / (statistics.median(ks) * 1e-3) / 1e9
            rec["rows"][f"es{es}_tst{tst}_sst{sst}"] = {
                "kernel": "mi355_copy_segments" if (tst, sst) == (1, 1) else "mi355_strided_copy",
                "nelems": useful // es, "kernel_us": spread(ks, 1e3, 1), "useful_GB_s": round(rate, 1),
                "fraction_of_contiguous": round(rate / base, 3),
                "line_bytes_touched_GB_s": round(rate * (min(sst, per_line) + min(tst, per_line)), 1),
                "elements_per_us": round(useful // es / (statistics.median(ks) * 1e3), 1)}
    shm.free_device(tgt)
    shm.free_device(src)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    shm.finalize()


if __name__ == "__main__":
    main()
