"""examples/wsum_example.c (bfloat16 partial gradients summed into an fp32
buffer on every PE through shmemx_bfloat16_wsum_to_all_float) builds against
the library (CPU) and runs on 2 PEs sharing the test GPU (GPU), the way
tests/test_loc_example.py builds and runs its example."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "osss-gasnet_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "wsum_example")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "wsum_example.c"), "-L", LIBDIR, "-lshmem_reduce",
                    f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    return exe


def test_example_compiles_and_links(tmp_path):
    out = subprocess.check_output(["nm", "-u", build(tmp_path)], text=True)
    assert "shmemx_bfloat16_wsum_to_all_float" in out


@pytest.mark.gpu
@pytest.mark.multipe
def test_example_runs_two_pes(tmp_path):
    exe = build(tmp_path)
    env = dict(os.environ, SHMEM_DEVICE_HEAP_SIZE="16M", SHMEM_DEVICE_SCRATCH_SIZE="3M", SHMEM_BARRIER_TIMEOUT="120")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "oshrun"), "-np", "2", "--same-device", exe],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": OK") == 2, r.stdout
