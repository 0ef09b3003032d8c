#!/usr/bin/env python3
"""The 16-bit float sums against the `short` sum at the same bytes and shapes
("16-bit floats"): one GPU, kernel time from HIP event
stamps on the library stream, median of `reps` launches, the whole set
repeated `repeats` times so the run-to-run spread shows.

  fold    mi355_combine, k = 2 and k = 8 sources of S bytes each
  orders  mi355_combine_orders, 8 members of S bytes each, every output
  call    the 1-PE <T>_sum_to_all of S bytes (target != source), host-timed

usage: half_bench.py [repeats] [reps]     one JSON line per figure
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

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
BIG = 256 << 20
os.environ.setdefault("SHMEM_DEVICE_HEAP_SIZE", str(10 * BIG + (64 << 20)))
os.environ.setdefault("SHMEM_DEVICE_SCRATCH_SIZE", "3M")
shm = shmem_reduce.Shmem()
shm.init()
hip = ctypes.CDLL("libamdhip64.so")
shm.lib.mi355_time_next_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
hip.hipEventCreate(ctypes.byref(e0))
hip.hipEventCreate(ctypes.byref(e1))
bufs = [shm.malloc_device(BIG) for _ in range(9)]
outs = [shm.malloc_device(32 << 20) for _ in range(8)]
# bit patterns 0x3000 .. 0x3FFF: finite normal numbers as half and as bfloat16
rng = np.random.default_rng(1)
fill = (rng.integers(0x3000, 0x4000, BIG // 2, dtype=np.uint16))
for b in bufs:
    shm.put(b, fill)


def timed(launch):
    for _ in range(3):
        launch()
    shm.sync()
    ts = []
    for _ in range(reps):
        shm.lib.mi355_time_next_launch(e0, e1)
        assert launch() == 0
        hip.hipEventSynchronize(e1)
        ms = ctypes.c_float()
        hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1)
        ts.append(ms.value)
    return float(np.median(ts)) * 1e3


for rep in range(repeats):
    for dtype in ("short", "half", "bfloat16"):
        for mib in (8, 256):          # warm (the sources fit the Infinity Cache) and from HBM
            S = mib << 20
            for k in (2, 8):
                us = timed(lambda: shm.combine("sum", dtype, bufs[0], bufs[1:1 + k], S // 2))
                print(json.dumps({"repeat": rep, "what": "fold", "dtype": dtype, "k": k, "MiB": mib,
                                  "us": round(us, 1), "GB_s": round((k + 1) * S / us / 1e3, 1)}), flush=True)
        for mib in (8, 32):
            S = mib << 20
            us = timed(lambda: shm.combine_orders("sum", dtype, outs, bufs[:8], S // 2))
            print(json.dumps({"repeat": rep, "what": "orders", "dtype": dtype, "k": 8, "MiB": mib,
                              "us": round(us, 1), "GB_s": round(16 * S / us / 1e3, 1)}), flush=True)
        n = BIG // 2
        ts = []
        for i in range(reps + 3):
            t0 = time.perf_counter()
            shm.to_all("sum", dtype, bufs[0], bufs[1], n, 0, 0, 1)
            ts.append(time.perf_counter() - t0)
        us = float(np.median(ts[3:])) * 1e6
        print(json.dumps({"repeat": rep, "what": "call", "dtype": dtype, "k": 1, "MiB": 256,
                          "us": round(us, 1), "GB_s": round(2 * BIG / us / 1e3, 1)}), flush=True)
shm.finalize()
