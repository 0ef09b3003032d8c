"""GPU: mi355_strided_copy, the strided kernel for elements of 1, 2, 4, 8 and
16 bytes (shmem_iput / shmem_iget run on it).

The checks run in one process of their own on torch-allocated buffers
(tests/_strided_copy_worker.py), as tests/test_gpu_alltoall.py's kernel tests
do. Expected values are torch indexing of the inputs:
    dst[k * dst_stride] = src[k * src_stride]        k < nelems
Every target is pre-filled with a sentinel byte and compared WHOLE, gaps and
tail included; the source is compared afterwards too.
"""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results():
    r = subprocess.run([sys.executable, os.path.join(HERE, "_strided_copy_worker.py")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("nseg", [1, 3, 64])
@pytest.mark.parametrize("es", [1, 2, 16])
def test_strided_copy_kernel(results, es, nseg):
    """Strides (1,2) (2,1) (1,3) (3,1) (2,5) (7,7) (33,1) (1,33) x nelems 0, 1,
    3, 5, 257 and the tile edges 256V - 1, 256V, 256V + 1, 2 * 256V + 37 with
    V = 16 / es (16 bytes: 1023, 1024, 1025, 2085); bases one element off
    alignment."""
    failures = results["matrix"][f"{es}-{nseg}"]
    assert not failures, failures[:10]


def test_one_byte_elements_at_every_phase_of_the_line(results):
    """the contiguous side of the 1-byte gather and scatter 0, 16, ... 112 (and
    5 more) bytes into its 128-byte line"""
    assert not results["phases_of_one_byte"], results["phases_of_one_byte"][:10]


@pytest.mark.parametrize("es", [4, 8])
def test_strided_copy_equals_strided_pull(results, es):
    assert not results["same_as_pull"][str(es)], results["same_as_pull"][str(es)][:10]


@pytest.mark.parametrize("es,nseg", [(1, 64), (2, 64), (16, 64), (1, 1)])
def test_strided_copy_kernel_past_one_pass(results, es, nseg):
    """Strides (1,2) (2,1) (1,3) (3,2) at 9 * 256V * gx + 256V + 37 elements
    per segment (16 bytes: 9 * 1024 * gx + 1024 + 37), gx read back from the
    library for that very launch: every block takes several trips round its
    tile loop and the last one is partial."""
    failures = results["passes"][f"{es}-{nseg}"]
    info = results["passes_info"][f"{es}-{nseg}"]
    print(f"grid-pass | strided_copy es {es} x{nseg} | (strides, gx, gy, nelems) {info}")
    assert not failures, failures
    assert len(info) == 4, info
    for _, gx, gy, n in info:
        assert gx > 0 and n > 2 * 4 * 256 * gx and gy == nseg, info


def test_strided_copy_rejects_bad_arguments(results):
    """element sizes 3, 32 and 0, strides < 1, misaligned 2- and 16-byte
    pointers on either side, 65 segments: non-zero, buffers untouched"""
    rec = results["bad_arguments"]
    assert len(rec["rcs"]) == 10 and all(rc != 0 for rc in rec["rcs"]) and rec["untouched"], rec


def test_strided_copy_offsets_past_4_gib(results):
    rec = results["past_4_gib"]
    assert rec["rcs"] == [0, 0] and rec["last_byte_offset"] > 2**32, rec
    assert rec["gathered"] == [-7] + rec["vals"] + [-7] * 4, rec
    assert rec["scattered"] == rec["vals"] and rec["source_after"] == rec["vals"], rec
