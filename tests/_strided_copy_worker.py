"""The process of tests/test_gpu_strided_copy.py: mi355_strided_copy on
torch-allocated device buffers, like tests/_strided_pull_worker.py (the
library loaded beside torch without shmem_init). Runs every check once and
prints one JSON line of what failed.

Buffers are integer tensors of shape (elements, words): one row per element
(uint8 / int16 / int32 / int64 rows of one word, two int64 words for a 16-byte
element), so one indexing expression serves every element size."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "osss-gasnet_amd"))

import torch  # noqa: E402

import shmem_reduce  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0x5A
STRIDES = [(1, 2), (2, 1), (1, 3), (3, 1), (2, 5), (7, 7), (33, 1), (1, 33)]
NEW_SIZES = [1, 2, 16]
NSEGS = [1, 3, 64]
PASS_STRIDES = [(1, 2), (2, 1), (1, 3), (3, 2)]
PASS_CASES = [(1, 64), (2, 64), (16, 64), (1, 1)]
ROW = {1: (torch.uint8, 1), 2: (torch.int16, 1), 4: (torch.int32, 1), 8: (torch.int64, 1), 16: (torch.int64, 2)}


def tile(es):
    """elements of one block pass: 256 lanes x V = 16 / es elements per vector
    (a 16-byte element: 256 lanes x the 4 slots of the vector-less form)"""
    return 256 * (16 // es) if es < 16 else 1024


def nelems_of(es):
    t = tile(es)
    return [0, 1, 3, 5, 257, t - 1, t, t + 1, 2 * t + 37]


def random_rows(n, es, seed):
    dt, w = ROW[es]
    g = torch.Generator(device=DEV).manual_seed(seed)
    b = torch.randint(0, 256, (n * es,), generator=g, dtype=torch.uint8, device=DEV)
    return b.view(dt).view(n, w)


def sentinel_rows(n, es):
    dt, w = ROW[es]
    return torch.full((n * es,), SENTINEL, dtype=torch.uint8, device=DEV).view(dt).view(n, w)


def layout(base, nseg, n, stride):
    """segment s starts base + s * (n * stride + 3) elements in: an odd number
    of elements apart, so the segments' alignments differ"""
    pitch = n * stride + 3
    return pitch, [base + s * pitch for s in range(nseg)]


def expected(tgt, src, dfirst, sfirst, n, dst, sst):
    want = tgt.clone()
    if n:
        k = torch.arange(n, device=DEV)
        d0 = torch.tensor(dfirst, device=DEV)[:, None]
        s0 = torch.tensor(sfirst, device=DEV)[:, None]
        want[(d0 + k * dst).flatten()] = src[(s0 + k * sst).flatten()]
    return want


def describe(tgt, want):
    bad = torch.nonzero((tgt != want).any(dim=1)).flatten()
    return (f"{bad.numel()} elements differ, first at {int(bad[0])}: got {tgt[bad[0]].tolist()}, "
            f"want {want[bad[0]].tolist()}")


def run_one(call, es, tgt, src, dfirst, sfirst, n, dst, sst, tag, failures):
    """fill the target with the sentinel, launch, compare the WHOLE target and the source"""
    tgt.view(torch.uint8).fill_(SENTINEL)
    want = expected(tgt, src, dfirst, sfirst, n, dst, sst)
    before = src.clone()
    rc = call(es, [tgt.data_ptr() + f * es for f in dfirst], [src.data_ptr() + f * es for f in sfirst], dst, sst, n)
    torch.cuda.synchronize()
    if rc != 0:
        failures.append(f"{tag}: rc {rc}")
    elif not torch.equal(tgt, want):
        failures.append(f"{tag}: {describe(tgt, want)}")
    elif not torch.equal(src, before):
        failures.append(f"{tag}: the source changed")


def matrix(shm, es, nseg):
    """Every stride pair (gather, scatter, both strided) x sizes below, at and
    above one tile; bases one element off the allocation (for 16 bytes: 16
    bytes off a 128-byte line)."""
    total = 1 + nseg * (max(nelems_of(es)) * 33 + 3)
    src = random_rows(total, es, 1234 + es)
    tgt = sentinel_rows(total, es)
    failures = []
    for dst, sst in STRIDES:
        for n in nelems_of(es):
            _, dfirst = layout(1, nseg, n, dst)
            _, sfirst = layout(1, nseg, n, sst)
            run_one(shm.strided_copy, es, tgt, src, dfirst, sfirst, n, dst, sst, f"strides ({dst},{sst}) n {n}",
                    failures)
    return failures


def phases_of_one_byte(shm):
    """1-byte elements, the contiguous side at every 16-byte phase of its
    128-byte line (and 5 bytes past each): the peeled head takes every length"""
    n = 2 * tile(1) + 37
    total = 256 + n * 3 + 8
    src = random_rows(total, 1, 77)
    tgt = sentinel_rows(total, 1)
    assert src.data_ptr() % 128 == 0 and tgt.data_ptr() % 128 == 0
    failures = []
    for dst, sst in ((1, 3), (3, 1)):
        for phase in range(8):
            for extra in (0, 5):
                off = 16 * phase + extra
                d0, s0 = (off, 1) if dst == 1 else (1, off)
                run_one(shm.strided_copy, 1, tgt, src, [d0], [s0], n, dst, sst,
                        f"strides ({dst},{sst}) contiguous side {off} bytes into its line", failures)
    return failures


def same_as_pull(shm, es):
    """4 and 8 bytes: mi355_strided_copy and mi355_strided_pull on the same
    inputs give the same target (and the expected one)"""
    nseg, ns = 3, [0, 1, 5, 257, 4099]
    total = 1 + nseg * (max(ns) * 33 + 3)
    src = random_rows(total, es, 4321 + es)
    a, b = sentinel_rows(total, es), sentinel_rows(total, es)
    failures = []
    for dst, sst in [(1, 1)] + STRIDES:
        for n in ns:
            _, dfirst = layout(1, nseg, n, dst)
            _, sfirst = layout(1, nseg, n, sst)
            tag = f"strides ({dst},{sst}) n {n}"
            run_one(shm.strided_copy, es, a, src, dfirst, sfirst, n, dst, sst, tag + " copy", failures)
            run_one(shm.strided_pull, es, b, src, dfirst, sfirst, n, dst, sst, tag + " pull", failures)
            if not torch.equal(a, b):
                failures.append(f"{tag}: strided_copy and strided_pull differ")
    return failures


def passes_rule(gx, nelems):
    """a block makes at least two full trips and a partial one round its tile
    loop (4: the deepest per-lane unroll of the layer's kernels)"""
    return gx > 0 and nelems > 2 * 4 * 256 * gx


def passes(shm, es, nseg):
    """Beyond one grid pass: nelems = 9 * tile * gx + tile + 37 per segment,
    gx being the grid of that very launch (predicted from the launcher's cap
    of 8 blocks per CU over the segments, read back after the launch and
    checked against the pass rule). Source and target are allocated per case,
    each under 1 GiB. Returns (failures, [(strides, gx, gy, nelems)...])."""
    failures, info = [], []
    gx0 = max(1, shm.device_cus() * 8 // nseg)
    n = 9 * tile(es) * gx0 + tile(es) + 37
    for dst, sst in PASS_STRIDES:
        dpitch, dfirst = layout(1, nseg, n, dst)
        spitch, sfirst = layout(1, nseg, n, sst)
        dtotal, stotal = 1 + nseg * dpitch, 1 + nseg * spitch
        assert max(dtotal, stotal) * es < 2**30, (es, nseg, dst, sst, n)
        src = random_rows(stotal, es, 99 + es + nseg)
        tgt = sentinel_rows(dtotal, es)
        want = expected(tgt, src, dfirst, sfirst, n, dst, sst)
        rc = shm.strided_copy(es, [tgt.data_ptr() + f * es for f in dfirst], [src.data_ptr() + f * es for f in sfirst],
                              dst, sst, n)
        gx, gy = shm.last_launch_grid()
        torch.cuda.synchronize()
        info.append([[dst, sst], gx, gy, n])
        tag = f"strides ({dst},{sst}) n {n} grid {gx} x {gy}"
        if rc != 0:
            failures.append(f"{tag}: rc {rc}")
        elif not passes_rule(gx, n):
            failures.append(f"{tag}: the elements do not pass twice over the grid")
        elif not torch.equal(tgt, want):
            failures.append(f"{tag}: {describe(tgt, want)}")
        del src, tgt, want
        torch.cuda.empty_cache()
    return failures, info


def bad_arguments(shm):
    t = torch.zeros(128, dtype=torch.int64, device=DEV)
    p = t.data_ptr()
    rcs = [shm.strided_copy(3, [p], [p + 512], 1, 2, 4),          # element sizes
           shm.strided_copy(32, [p], [p + 512], 1, 2, 4),
           shm.strided_copy(0, [p], [p + 512], 1, 2, 4),
           shm.strided_copy(1, [p], [p + 512], 0, 2, 4),          # stride < 1
           shm.strided_copy(16, [p], [p + 512], 2, -1, 4),
           shm.strided_copy(2, [p + 1], [p + 512], 2, 1, 4),      # not element-aligned
           shm.strided_copy(2, [p], [p + 513], 1, 2, 4),
           shm.strided_copy(16, [p + 8], [p + 512], 2, 1, 4),
           shm.strided_copy(16, [p], [p + 520], 1, 2, 4),
           shm.strided_copy(1, [p] * 65, [p + 512] * 65, 2, 1, 1)]  # 65 segments
    torch.cuda.synchronize()
    return {"rcs": rcs, "untouched": int(t.abs().sum()) == 0}


def past_4_gib(shm):
    """2-byte elements 2^30 + 1 apart: the third lies past 4 GiB in an
    allocation that is otherwise never touched; as the source, then as the
    target."""
    stride = 2**30 + 1
    big = torch.empty(2 * stride + 8, dtype=torch.int16, device=DEV)   # ~4.3 GB, not filled
    vals = [11111, -22222, 3333]
    for k, v in enumerate(vals):
        big[1 + k * stride] = v
    out = torch.full((8,), -7, dtype=torch.int16, device=DEV)
    rc1 = shm.strided_copy(2, [out.data_ptr() + 2], [big.data_ptr() + 2], 1, stride, 3)
    torch.cuda.synchronize()
    gathered = out.tolist()
    rc2 = shm.strided_copy(2, [big.data_ptr() + 4], [out.data_ptr() + 2], stride, 1, 3)
    torch.cuda.synchronize()
    return {"rcs": [rc1, rc2], "last_byte_offset": (1 + 2 * stride) * 2, "vals": vals, "gathered": gathered,
            "scattered": [int(big[2 + k * stride]) for k in range(3)],
            "source_after": [int(big[1 + k * stride]) for k in range(3)]}


def main():
    shm = shmem_reduce.Shmem()   # loads the library; no shmem_init
    torch.cuda.set_device(0)
    rec = {"matrix": {f"{es}-{nseg}": matrix(shm, es, nseg) for es in NEW_SIZES for nseg in NSEGS},
           "phases_of_one_byte": phases_of_one_byte(shm),
           "same_as_pull": {str(es): same_as_pull(shm, es) for es in (4, 8)},
           "bad_arguments": bad_arguments(shm), "past_4_gib": past_4_gib(shm), "passes": {}, "passes_info": {}}
    for es, nseg in PASS_CASES:
        rec["passes"][f"{es}-{nseg}"], rec["passes_info"][f"{es}-{nseg}"] = passes(shm, es, nseg)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
