#!/usr/bin/env python3
"""The identity copy's sweep direction, A/B in one process and one build.

Times mi355_copy_segments on one 256 MiB segment (the headline's kernel,
copy_segments<4,1>) with the library's own event stamps
(mi355_time_next_launch), the direction pinned or left to the library
(mi355_copy_direction_next_launch). One process, no PE job.

Legs (REPS launches each, after WARM untimed ones in the leg's own order):
  a_ascending    the same pair every launch, every launch pinned ascending
  b_alternating  the same pair, unpinned: the library alternates
  c_descending   the same pair, every launch pinned descending
  d_cold_*       5 disjoint pairs taken in turn (bench.py rotating_leg's
                 layout: 2.5 GiB of footprint, every byte from HBM),
                 alternating and pinned ascending
(a) against (b) is the result; (c) shows what descending alone costs; (d)
that the HBM-only case does not change. The call_* entries time the blocking
call itself (shmem_double_sum_to_all on a 1-PE set, entry to return, the
interpreter's per-call cost included in every leg alike). Prints one JSON line.

usage: copy_direction_ab.py [MiB] [reps]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "osss-gasnet_amd"))
import shmem_reduce  # noqa: E402

PAIRS = 5
WARM = 20


def stats(us):
    a = np.asarray(us)
    return {"mean_us": round(float(a.mean()), 2), "median_us": round(float(np.median(a)), 2),
            "min_us": round(float(a.min()), 2), "max_us": round(float(a.max()), 2),
            "p10_us": round(float(np.percentile(a, 10)), 2), "p90_us": round(float(np.percentile(a, 90)), 2),
            "launches": len(us)}


def main():
    mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    S = mib << 20
    os.environ.setdefault("SHMEM_DEVICE_HEAP_SIZE", str(2 * PAIRS * S + (64 << 20)))
    os.environ.setdefault("SHMEM_DEVICE_SCRATCH_SIZE", "3M")
    shm = shmem_reduce.Shmem()
    shm.init()
    L = shm.lib
    L.mi355_time_next_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.mi355_time_next_launch.restype = None
    hip = ctypes.CDLL("libamdhip64.so")
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0

    x = np.random.default_rng(3).integers(0, 1 << 63, S // 8, dtype=np.int64)
    pairs = []
    for _ in range(PAIRS):
        s, d = shm.malloc_device(S), shm.malloc_device(S)
        assert s and d, "device heap too small (SHMEM_DEVICE_HEAP_SIZE)"
        shm.put(s, x)
        pairs.append((s, d))
    nb = (ctypes.c_size_t * 1)(S)

    def launch(pair, pin, timed):
        if timed:
            L.mi355_time_next_launch(e0, e1)
        if pin:
            L.mi355_copy_direction_next_launch(pin)
        rc = L.mi355_copy_segments((ctypes.c_void_p * 1)(pair[1]), (ctypes.c_void_p * 1)(pair[0]), nb, 1, None)
        assert rc == 0, rc
        if not timed:
            return None
        assert hip.hipEventSynchronize(e1) == 0
        ms = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1) == 0
        return ms.value * 1e3

    def leg(pin, npairs):
        for j in range(WARM):
            launch(pairs[j % npairs], pin, False)
        shm.sync()
        return stats([launch(pairs[j % npairs], pin, True) for j in range(reps)])

    def wall_leg(pin, npairs):
        """the blocking call itself, shmem_double_sum_to_all on a 1-PE set, entry to return"""
        def call(j):
            L.mi355_copy_direction_next_launch(pin)
            shm.to_all("sum", "double", pairs[j % npairs][1], pairs[j % npairs][0], S // 8, 0, 0, 1)
        for j in range(WARM):
            call(j)
        shm.sync()
        t0 = time.perf_counter()
        for j in range(reps):
            call(j)
        return {"us_per_call": round((time.perf_counter() - t0) / reps * 1e6, 2), "calls": reps}

    res = {"tool": "copy_direction_ab", "bytes_per_buffer": S, "kernel_code_sha": shmem_reduce.kernel_code_hash(),
           "a_ascending": leg(1, 1), "b_alternating": leg(0, 1), "c_descending": leg(-1, 1),
           "d_cold_alternating": leg(0, PAIRS), "d_cold_ascending": leg(1, PAIRS),
           # the warm legs once more, in the opposite order: drift over the run shows here
           "c_descending_again": leg(-1, 1), "b_alternating_again": leg(0, 1), "a_ascending_again": leg(1, 1)}
    # entry-to-return time of the blocking call, warm (one pair) and cold (5 pairs), each leg twice
    for rnd in ("", "_again"):
        for name, pin, npairs in (("warm_ascending", 1, 1), ("warm_alternating", 0, 1), ("cold_ascending", 1, PAIRS),
                                  ("cold_alternating", 0, PAIRS), ("cold_descending", -1, PAIRS)):
            res["call_" + name + rnd] = wall_leg(pin, npairs)
    bad = sum(int((shm.get(d, S // 8, np.int64) != x).sum()) for _, d in pairs)
    res["check"] = "every target equals its source" if bad == 0 else f"MISMATCH in {bad} words"
    print(json.dumps(res), flush=True)
    for s, d in pairs:
        shm.free_device(d)
        shm.free_device(s)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    shm.finalize()
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
