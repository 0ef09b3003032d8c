"""CPU: the C surface of the scan collectives -- the 104 shmemx_<T>_<op>_inscan /
_exscan entry points (one pair per (type, op) that has a *_to_all) and
mi355_combine_prefix are declared in the headers and exported by the built
library; no pshmem_ twin, no stream-ordered form."""
import ctypes
import os
import re

import pytest

import _scan_ref
import shmem_reduce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("inscan", "exscan")
NAMES = [f"shmemx_{t}_{op}_{form}" for op, t in _scan_ref.PAIRS for form in FORMS]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(shmem_reduce.LIB_PATH):
        pytest.fail(f"{shmem_reduce.LIB_PATH} not built (run __graft_entry__.build())")
    return ctypes.CDLL(shmem_reduce.LIB_PATH)


def header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_104_entry_points_declared_and_exported(lib):
    assert len(NAMES) == 104 and len(set(NAMES)) == 104
    text = header("shmemx.h")
    declared = re.findall(r"^void (shmemx_[a-z0-9]+_[a-z]+_(?:inscan|exscan)) \(", text, flags=re.M)
    assert sorted(declared) == sorted(NAMES)
    missing = [n for n in NAMES if not hasattr(lib, n)]
    assert not missing, missing


def test_argument_types_follow_to_all():
    """each declaration is its *_to_all's with the name changed"""
    x = header("shmemx.h")
    std = header("shmem.h")
    for op, t in _scan_ref.PAIRS:
        if t in _scan_ref.HALF_TYPES:
            m = re.search(rf"^void shmemx_{t}_{op}_to_all \((.*?)\);", x, flags=re.M | re.S)
        else:
            m = re.search(rf"^\s*void shmem_{t}_{op}_to_all \((.*?)\);", std, flags=re.M | re.S)
        assert m, (op, t)
        want = re.sub(r"\s+", " ", m.group(1))
        for form in FORMS:
            d = re.search(rf"^void shmemx_{t}_{op}_{form} \((.*?)\);", x, flags=re.M | re.S)
            assert d and re.sub(r"\s+", " ", d.group(1)) == want, (op, t, form)


def test_no_twins_and_no_other_pairs(lib):
    for op, t in _scan_ref.PAIRS:
        for form in FORMS:
            assert not hasattr(lib, f"pshmem_{t}_{op}_{form}") and not hasattr(lib, f"shmem_{t}_{op}_{form}")
            assert not hasattr(lib, f"shmemx_{t}_{op}_{form}_on_stream")
    for t, op in (("float", "and"), ("complexf", "max"), ("half", "xor"), ("bfloat16", "or"), ("double", "xor")):
        assert not hasattr(lib, f"shmemx_{t}_{op}_inscan"), (t, op)
    for h in ("shmem.h", "pshmem.h", "shmem_fortran.h"):
        assert "scan" not in header(h), h


def test_combine_prefix_exported_and_checks_its_arguments(lib):
    assert re.search(r"^int mi355_combine_prefix \(int op, int dtype, void \*const \*dsts, const void \*const \*srcs,\s*"
                     r"int nsrc, size_t n, void \*stream\);", header("mi355_reduce.h"), flags=re.M)
    f = lib.mi355_combine_prefix
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                  ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(buf)
    two = (ctypes.c_void_p * 2)(p, p)
    # argument checks only (nothing is launched): an invalid pair, counts out of range, a null source
    assert f(2, 5, two, two, 2, 8, None) == -2          # double and
    assert f(5, 7, two, two, 2, 8, None) == -2          # float complex min
    assert f(4, 9, two, two, 2, 8, None) == -2          # half xor
    assert f(0, 5, two, two, 0, 8, None) == -1
    many = (ctypes.c_void_p * 33)(*([p] * 33))
    assert f(0, 5, many, many, 33, 8, None) == -1
    assert f(0, 5, two, (ctypes.c_void_p * 2)(p, None), 2, 8, None) == -1
    assert f(0, 5, None, two, 2, 8, None) == -1


def test_python_binding_resolves_every_pair():
    s = shmem_reduce.Shmem()   # loads the library; no shmem_init
    for op, t in _scan_ref.PAIRS:
        for excl in (False, True):
            assert s._scan_fn(op, t, excl) is not None
    with pytest.raises(AttributeError):
        s._scan_fn("xor", "float", False)
