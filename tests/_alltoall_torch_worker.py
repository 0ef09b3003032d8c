"""One PE of tests/test_gpu_alltoall.py::test_alltoall_tensors_two_pes:
Shmem.alltoall_tensors on symmetric-heap torch tensors, checked against torch
indexing of the inputs every PE can regenerate. Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "osss-gasnet_amd"))

import torch  # noqa: E402

import shmem_reduce  # noqa: E402


def inputs(pe, n, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed * 1009 + pe)
    if dtype.is_floating_point:
        return torch.randn(n, generator=g, dtype=dtype)
    return torch.randint(-2**40, 2**40, (n,), generator=g, dtype=dtype)


def main():
    shm = shmem_reduce.Shmem()
    shm.init()
    me, npes = shm.my_pe(), shm.n_pes()
    torch.cuda.set_device(shm.lib.shmemx_device_id())
    checked = 0
    # (dtype, elements per block): 64-bit moves, 32-bit moves (odd count of float32), a large one
    for k, (dtype, per) in enumerate([(torch.float32, 6), (torch.float32, 7), (torch.int64, 3), (torch.int64, 50001),
                                      (torch.float32, 100001)]):
        n = per * npes
        x = shm.heap_tensor(n, dtype)
        x.copy_(inputs(me, n, dtype, 40 + k))
        out = torch.full((n,), -7, dtype=dtype, device=x.device)   # outside the heap
        torch.cuda.synchronize()
        shm.alltoall_tensors(out, x)
        want = torch.cat([inputs(pe, n, dtype, 40 + k)[me * per:(me + 1) * per] for pe in range(npes)])
        assert torch.equal(out.cpu(), want), (me, dtype, per)
        checked += 1
        shm.barrier_all()
        shm.free_device(x.data_ptr())
    # a block that is no multiple of 4 bytes
    try:
        t = torch.zeros(3 * npes, dtype=torch.int16, device="cuda")
        shm.alltoall_tensors(t, t)
        raise AssertionError("no ValueError for a 6-byte block")
    except ValueError:
        pass
    shm.barrier_all()
    print(json.dumps({"pe": me, "ok": True, "checked": checked}), flush=True)
    shm.finalize()


if __name__ == "__main__":
    main()
