"""PyTorch tensors as *_to_all target/source at 2 PEs (sharing the test
GPU): the members map each other's caching-allocator segments for the call
(extmap.c) -- no staging copies -- and every PE gets the reference's result
for itself; a view off 16-byte alignment makes every member stage instead."""
import os
import sys

import pytest

from _pes import launch

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = [pytest.mark.gpu, pytest.mark.multipe]


def run_workers(script, npes=2):
    env = dict(SHMEM_DEVICE_HEAP_SIZE="64M", SHMEM_DEVICE_SCRATCH_SIZE="3M", SHMEM_BARRIER_TIMEOUT="120",
               SHMEM_PEER_ACQUIRE="1")
    return launch(npes, [sys.executable, os.path.join(HERE, script)], gpu=True, timeout=300, env=env).records()


def test_torch_tensors_mapped_between_pes():
    for rec in run_workers("_torch_tensor_worker.py"):
        for name, sched in rec["schedules"].items():
            assert sched.startswith("mapped-") == ("unaligned" not in name), (rec["pe"], name, sched)
        mapped, opened, closed = rec["map_stats"]
        assert opened >= 1 and closed == 0, rec


def test_torch_stream_and_graph():
    """Symmetric-heap torch tensors with the stream-ordered reduction between
    torch kernels on one torch stream, eager and captured by torch.cuda.graph
    (5 replays = 5 collectives), bit-exact against the oracle."""
    for rec in run_workers("_torch_graph_worker.py"):
        assert rec["ok"] and rec["replays"] == 5, rec
