"""The process of tests/test_gpu_alltoall.py's kernel tests: mi355_strided_pull
on torch-allocated device buffers. It loads the library without shmem_init
(the kernel layer needs no runtime: no heap, no peers, no exit handler beside
torch's), runs every check once and prints one JSON line of what failed."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "osss-gasnet_amd"))

import torch  # noqa: E402

import shmem_reduce  # noqa: E402

SENTINEL = -7
STRIDES = [(1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (2, 5), (7, 7), (33, 1), (1, 33)]
NELEMS = [0, 1, 3, 5, 257, 4099]
DEV = "cuda:0"
PASS_CASES = [(4, 64), (8, 64), (8, 1)]   # 64 segments: the least data past one pass


def matrix(shm, es, nseg):
    """Every stride pair (each kernel form: gather, scatter, both strided, the
    copy) x sizes below, at and above one 256-lane tile and one 16-byte
    vector; bases one element off the allocation so neither side starts
    16-byte aligned, segments an odd number of elements apart so their
    alignments differ. The whole target is compared."""
    tdt = torch.int32 if es == 4 else torch.int64
    total = 1 + nseg * (max(NELEMS) * 33 + 3)
    g = torch.Generator(device="cpu").manual_seed(1234 + es)
    src = torch.randint(-2**31, 2**31 - 1, (total,), generator=g, dtype=torch.int64).to(tdt).to(DEV)
    tgt = torch.empty(total, dtype=tdt, device=DEV)
    failures = []
    for dst, sst in STRIDES:
        for n in NELEMS:
            dpitch, spitch = n * dst + 3, n * sst + 3
            tgt.fill_(SENTINEL)
            want = tgt.clone()
            k = torch.arange(n, device=DEV)
            seg = torch.arange(nseg, device=DEV)[:, None]
            want[1 + seg * dpitch + k * dst] = src[1 + seg * spitch + k * sst]
            dptrs = [tgt.data_ptr() + (1 + s * dpitch) * es for s in range(nseg)]
            sptrs = [src.data_ptr() + (1 + s * spitch) * es for s in range(nseg)]
            rc = shm.strided_pull(es, dptrs, sptrs, dst, sst, n)
            torch.cuda.synchronize()
            if rc != 0:
                failures.append(f"strides ({dst},{sst}) n {n}: rc {rc}")
            elif not torch.equal(tgt, want):
                bad = torch.nonzero(tgt != want).flatten()
                failures.append(f"strides ({dst},{sst}) n {n}: {bad.numel()} elements differ, first at "
                                f"{int(bad[0])}: got {int(tgt[bad[0]])}, want {int(want[bad[0]])}")
    return failures


PASS_STRIDES = [(1, 2), (1, 3), (2, 1), (3, 1), (2, 3), (3, 2)]   # gather, scatter, both strided
PASS_BUDGET = 640 << 20   # bytes of source and of target a "passes" case may span


def passes_rule(gx, nelems):
    """a block makes at least two full trips and a partial one round its tile
    loop (4: the deepest per-lane unroll of the layer's kernels)"""
    return nelems > 2 * 4 * 256 * gx


def passes_sized(gx):
    return 9 * 1024 * gx + 1024 + 37


def passes(shm, es, nseg):
    """Beyond one grid pass: every block takes several trips round its tile
    loop (the prefetch hand-off, the LDS tile reused between the barriers) and
    the last trip is partial (blocks without a next tile, a partly filled
    tile). The grid is read back from the library after a first launch over
    the whole buffer; nelems = 9 * 1024 * gx + 1024 + 37 per segment. Bases one
    element off alignment; the whole target is compared. Returns (failures,
    [(strides, gx, gy, nelems)...])."""
    tdt = torch.int32 if es == 4 else torch.int64
    total = PASS_BUDGET // es
    g = torch.Generator(device=DEV).manual_seed(4321 + es + nseg)
    lim = 2**31 - 1 if es == 4 else 2**62
    src = torch.randint(-lim, lim, (total,), generator=g, dtype=tdt, device=DEV)
    tgt = torch.empty(total, dtype=tdt, device=DEV)
    failures, info = [], []
    for dst, sst in PASS_STRIDES:
        big = max(dst, sst)
        room = ((total - 1) // nseg - 3) // big       # elements per segment the buffers hold
        probe_d = [tgt.data_ptr() + (1 + s * (room * dst + 3)) * es for s in range(nseg)]
        probe_s = [src.data_ptr() + (1 + s * (room * sst + 3)) * es for s in range(nseg)]
        rc = shm.strided_pull(es, probe_d, probe_s, dst, sst, room)
        gx, _ = shm.last_launch_grid()
        torch.cuda.synchronize()
        n = passes_sized(gx)
        if rc != 0 or gx == 0 or n > room:
            failures.append(f"strides ({dst},{sst}): probe rc {rc}, grid {gx}, {n} elements against room for {room}")
            continue
        dpitch, spitch = n * dst + 3, n * sst + 3
        tgt.fill_(SENTINEL)
        want = tgt.clone()
        k = torch.arange(n, device=DEV)
        seg = torch.arange(nseg, device=DEV)[:, None]
        want[1 + seg * dpitch + k * dst] = src[1 + seg * spitch + k * sst]
        dptrs = [tgt.data_ptr() + (1 + s * dpitch) * es for s in range(nseg)]
        sptrs = [src.data_ptr() + (1 + s * spitch) * es for s in range(nseg)]
        rc = shm.strided_pull(es, dptrs, sptrs, dst, sst, n)
        gx, gy = shm.last_launch_grid()
        torch.cuda.synchronize()
        info.append([[dst, sst], gx, gy, n])
        if rc != 0:
            failures.append(f"strides ({dst},{sst}) n {n}: rc {rc}")
        elif not passes_rule(gx, n):
            failures.append(f"strides ({dst},{sst}): {n} elements do not pass twice over a grid of {gx} x {gy}")
        elif not torch.equal(tgt, want):
            bad = torch.nonzero(tgt != want).flatten()
            failures.append(f"strides ({dst},{sst}) n {n} grid {gx} x {gy}: {bad.numel()} elements differ, first at "
                            f"{int(bad[0])}: got {int(tgt[bad[0]])}, want {int(want[bad[0]])}")
        del want
    return failures, info


def grid_of_four_segments(shm):
    """The saturated grid of a 32-bit strided pull of 4 segments, per stride
    pair: what a 4-PE shmem_alltoalls32 launches (test_alltoall_four_pes sizes
    its large case from it)."""
    buf = torch.empty(2 * (64 << 20), dtype=torch.int32, device=DEV)
    half = buf.numel() // 2
    out = {}
    for dst, sst in [(2, 3), (1, 3)]:
        room = (half // 4) // max(dst, sst)
        d = [buf.data_ptr() + s * (half // 4) * 4 for s in range(4)]
        sp = [buf.data_ptr() + (half + s * (half // 4)) * 4 for s in range(4)]
        rc = shm.strided_pull(4, d, sp, dst, sst, room)
        torch.cuda.synchronize()
        assert rc == 0, rc
        out[f"{dst},{sst}"] = shm.last_launch_grid()[0]
    return out


def bad_arguments(shm):
    t = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = t.data_ptr()
    rcs = [shm.strided_pull(2, [p], [p + 256], 1, 2, 4),        # element size
           shm.strided_pull(4, [p], [p + 256], 0, 2, 4),        # stride < 1
           shm.strided_pull(4, [p], [p + 256], 2, -1, 4),
           shm.strided_pull(8, [p + 4], [p + 256], 2, 1, 4),    # not element-aligned
           shm.strided_pull(4, [p] * 65, [p + 256] * 65, 2, 1, 1)]
    torch.cuda.synchronize()
    return {"rcs": rcs, "untouched": int(t.abs().sum()) == 0}


def past_4_gib(shm):
    """4-byte elements 2^29 + 1 apart: the third lies past 4 GiB in an
    allocation that is otherwise never touched; as the source, then as the
    target."""
    stride = 2**29 + 1
    big = torch.empty(2 * stride + 8, dtype=torch.int32, device=DEV)   # ~4.3 GB, not filled
    vals = [1111111, -2222222, 333333333]
    for k, v in enumerate(vals):
        big[1 + k * stride] = v
    out = torch.full((8,), SENTINEL, dtype=torch.int32, device=DEV)
    rc1 = shm.strided_pull(4, [out.data_ptr() + 4], [big.data_ptr() + 4], 1, stride, 3)
    torch.cuda.synchronize()
    gathered = out.tolist()
    rc2 = shm.strided_pull(4, [big.data_ptr() + 8], [out.data_ptr() + 4], stride, 1, 3)
    torch.cuda.synchronize()
    return {"rcs": [rc1, rc2], "last_byte_offset": (1 + 2 * stride) * 4, "vals": vals, "gathered": gathered,
            "scattered": [int(big[2 + k * stride]) for k in range(3)],
            "source_after": [int(big[1 + k * stride]) for k in range(3)]}


def main():
    shm = shmem_reduce.Shmem()   # loads the library; no shmem_init
    torch.cuda.set_device(0)
    rec = {"matrix": {f"{es}-{nseg}": matrix(shm, es, nseg) for es in (4, 8) for nseg in (1, 3, 64)},
           "bad_arguments": bad_arguments(shm), "past_4_gib": past_4_gib(shm),
           "grid_of_four_segments": grid_of_four_segments(shm), "passes": {}, "passes_info": {}}
    for es, nseg in PASS_CASES:
        rec["passes"][f"{es}-{nseg}"], rec["passes_info"][f"{es}-{nseg}"] = passes(shm, es, nseg)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
