#!/usr/bin/env python3
"""Rate of the widening fold against the 16-bit fold it sits beside (one GPU).

    python tools/wide_bench.py [--mi 64] [--repeats 7] [--out file.json]

One process, one PE. For bfloat16 and half at 2 and 8 sources of `mi` Mi
elements each: mi355_combine_wide with the 16-bit output and with the float
output, and -- the yardstick, in the same run, on the same buffers --
mi355_combine's sum of the same type. Each launch is timed by an event pair
after 3 warm-ups; median, min and max of `repeats` launches in microseconds,
and the bytes moved (sources read once plus the output written) per second.
The 16-bit output moves the yardstick's bytes and is compared by time; the
float output writes twice the output bytes and is compared by bytes per second.

Prints one JSON record.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "osss-gasnet_amd"))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mi", type=int, default=64, help="Mi elements per source")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    n = args.mi << 20
    max_src = 8
    os.environ.setdefault("SHMEM_DEVICE_HEAP_SIZE", f"{(max_src * 2 + 4) * args.mi + 192}M")
    os.environ.setdefault("SHMEM_DEVICE_SCRATCH_SIZE", "3M")
    for k in ("SHMEM_PE", "SHMEM_NPES"):
        os.environ.pop(k, None)
    import numpy as np
    import shmem_reduce
    shm = shmem_reduce.Shmem()
    shm.init()
    vp = ctypes.c_void_p
    srcs = [shm.malloc_device(n * 2) for _ in range(max_src)]
    dst = shm.malloc_device(n * 4)
    assert all(srcs) and dst
    rng = np.random.default_rng(5)
    ev = [vp(), vp()]
    for e in ev:
        shm._hip("hipEventCreate", ctypes.byref(e))
    ms = ctypes.c_float()

    def timed(launch):
        out = []
        for i in range(3 + args.repeats):
            shm.lib.mi355_time_next_launch(ev[0], ev[1])
            assert launch() == 0
            shm.sync()
            shm._hip("hipEventElapsedTime", ctypes.byref(ms), ev[0], ev[1])
            if i >= 3:
                out.append(ms.value * 1e3)
        return spread(out)

    rec = {"gpu": shm.lib.shmemx_device_id(), "cus": shm.device_cus(), "elements": n, "repeats": args.repeats,
           "kernels": {}, "results": {}}
    for dtype, one, mant in (("bfloat16", 0x3F80, 7), ("half", 0x3C00, 10)):
        # finite values of both signs within a few binades of 1.0: no NaN, no overflow at 8 sources
        m = min(n, 4 << 20)
        e = rng.integers(-3, 4, m)
        block = ((one + (e << mant) + rng.integers(0, 1 << mant, m)) | (rng.integers(0, 2, m) << 15)).astype(np.uint16)
        for k, s in enumerate(srcs):     # one random block, rotated per source and repeated
            shm.put(s, np.resize(np.roll(block, 1237 * k), n))
        for nsrc in (2, 8):
            r = {}
            r["combine_sum_us"] = timed(lambda: shm.combine("sum", dtype, dst, srcs[:nsrc], n))
            rec["kernels"][f"{dtype}_{nsrc}_combine"] = shm.last_kernel_name()
            r["wide_16bit_us"] = timed(lambda: shm.combine_wide(dtype, dtype, dst, srcs[:nsrc], n))
            rec["kernels"][f"{dtype}_{nsrc}_wide_16bit"] = shm.last_kernel_name()
            r["wide_float_us"] = timed(lambda: shm.combine_wide(dtype, "float", dst, srcs[:nsrc], n))
            rec["kernels"][f"{dtype}_{nsrc}_wide_float"] = shm.last_kernel_name()
            b16, b32 = (nsrc + 1) * n * 2, (nsrc + 2) * n * 2
            tb = lambda nbytes, us: nbytes / (us * 1e-6) / 1e12     # noqa: E731
            r["combine_sum_TBps"] = tb(b16, r["combine_sum_us"]["median"])
            r["wide_16bit_TBps"] = tb(b16, r["wide_16bit_us"]["median"])
            r["wide_float_TBps"] = tb(b32, r["wide_float_us"]["median"])
            r["wide_16bit_time_ratio"] = r["wide_16bit_us"]["median"] / r["combine_sum_us"]["median"]
            r["wide_float_rate_ratio"] = r["wide_float_TBps"] / r["combine_sum_TBps"]
            rec["results"][f"{dtype}_{nsrc}src"] = r
    shm.free_device(dst)
    for s in reversed(srcs):
        shm.free_device(s)
    shm.finalize()
    line = json.dumps(rec)
    print("WIDE_BENCH " + line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
