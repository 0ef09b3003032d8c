"""CPU: the C surface of the 16-bit float reductions -- the 16 shmemx_ entry
points are exported and declared, the two dtypes have their sizes and
operator matrix, the reference's 44 stay what they were."""
import ctypes
import os
import re

import pytest

import shmem_reduce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("half", "bfloat16")
OPS = ("sum", "prod", "min", "max")
NAMES = [f"shmemx_{t}_{op}_to_all{sfx}" for t in TYPES for op in OPS for sfx in ("", "_on_stream")]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(shmem_reduce.LIB_PATH):
        pytest.fail(f"{shmem_reduce.LIB_PATH} not built (run __graft_entry__.build())")
    return shmem_reduce.load()


def header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_sixteen_entry_points_exported_and_declared(lib):
    assert len(NAMES) == 16
    text = header("shmemx.h")
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(rf"^void {n} \(", text, flags=re.M), n
    assert re.search(r"typedef unsigned short shmemx_half_t, shmemx_bfloat16_t;", text)
    # no bitwise operators, no pshmem twins, nothing added to shmem.h / pshmem.h
    for t in TYPES:
        for op in ("and", "or", "xor"):
            assert not hasattr(lib, f"shmemx_{t}_{op}_to_all")
        assert not hasattr(lib, f"pshmemx_{t}_sum_to_all") and not hasattr(lib, f"pshmem_{t}_sum_to_all")
        assert not hasattr(lib, f"shmem_{t}_sum_to_all")
        for h in ("shmem.h", "pshmem.h"):
            assert t not in header(h)


def test_dtype_numbers_sizes_and_op_matrix(lib):
    text = header("mi355_reduce.h")
    assert re.search(r"MI355_HALF = 9,", text) and re.search(r"MI355_BFLOAT16 = 10,", text)
    assert re.search(r"MI355_NUM_DTYPES = 11\b", text)
    assert shmem_reduce.DTYPES.index("half") == 9 and shmem_reduce.DTYPES.index("bfloat16") == 10
    assert lib.mi355_dtype_size(9) == 2 and lib.mi355_dtype_size(10) == 2
    assert lib.mi355_dtype_size(11) == 0
    for t in (9, 10):
        for op, name in enumerate(shmem_reduce.OPS):
            assert bool(lib.mi355_op_supported(op, t)) == (name in OPS), (name, t)
    assert not lib.mi355_op_supported(0, 11)


def test_python_tables():
    import numpy as np
    assert shmem_reduce.NP["half"] is np.float16 and shmem_reduce.NP["bfloat16"] is np.uint16
    assert shmem_reduce.TORCH_DTYPES["float16"] == "half" and shmem_reduce.TORCH_DTYPES["bfloat16"] == "bfloat16"
    s = shmem_reduce.Shmem()   # loads the library; no shmem_init
    for t in TYPES:
        for op in OPS:
            assert s._reduction(op, t) is not None and s._stream_reduction(op, t) is not None
    with pytest.raises(AttributeError):
        s._reduction("xor", "half")


def test_combine_rejects_what_the_types_lack(lib):
    """argument checks only (no launch): a bitwise operator on a 16-bit float is unsupported"""
    buf = (ctypes.c_uint16 * 8)()
    srcs = (ctypes.c_void_p * 2)(ctypes.addressof(buf), ctypes.addressof(buf))
    for t in (9, 10):
        for op in (2, 3, 4):
            assert lib.mi355_combine(op, t, ctypes.addressof(buf), srcs, 2, 8, None) == -2
            assert lib.mi355_combine_orders(op, t, srcs, srcs, 2, 8, None) == -2
