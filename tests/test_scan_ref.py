"""CPU: the scan's expected values (tests/_scan_ref.py) on the golden and
NaN-family sources of tests/golden/: the last member's inscan is the
reference's result on the first member over all sources (the recorded golden
output), exscan(j) is inscan(j - 1), member 0's exscan is "untouched", and
prefix 0 is the source's bits."""
import json
import os

import numpy as np
import pytest

import _half_ref
import _scan_ref as S
import oracle

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MAN = json.load(open(os.path.join(GOLDEN, "manifest.json")))


def families(op, dtype):
    """(sources, the reference's recorded result on member 0) of every fixture of the pair"""
    out = []
    for key, stem in (("cases", "golden"), ("nan_cases", "golden_nan")):
        rows = MAN[key].get(f"{op}_{dtype}")
        if not rows:
            continue
        z = np.load(os.path.join(GOLDEN, f"{stem}_{op}_{dtype}.npz"))
        for k, c in enumerate(rows):
            ins = z[f"in_{k}"]
            out.append(([ins[i] for i in range(c["npes"])], z[f"out_{k}"][0]))
    return out


def same(a, b, op, dtype):
    return a.shape == b.shape and len(S.differing(a, b, op, dtype)) == 0


@pytest.mark.parametrize("op,dtype", oracle.PAIRS)
def test_golden_sources(op, dtype):
    fams = families(op, dtype)
    assert fams
    for srcs, out0 in fams:
        n = len(srcs)
        last = S.expected(op, dtype, srcs, n - 1, False)
        assert same(last, oracle.reduce_pe(op, dtype, srcs, 0), op, dtype)
        assert same(last, out0, op, dtype)                    # the fixture's recorded bits
        assert same(S.expected(op, dtype, srcs, 0, False), srcs[0], op, dtype)
        assert isinstance(S.expected(op, dtype, srcs, 0, True), str) and S.expected(op, dtype, srcs, 0, True) == S.UNTOUCHED
        for j in range(1, n):
            assert same(S.expected(op, dtype, srcs, j, True), S.expected(op, dtype, srcs, j - 1, False), op, dtype)


@pytest.mark.parametrize("op,dtype", S.HALF_PAIRS)
def test_half_sources(op, dtype):
    srcs = _half_ref.sources(dtype, 9, 4099, 77)
    assert same(S.expected(op, dtype, srcs, 8, False), _half_ref.left_fold(op, dtype, srcs), op, dtype)
    assert (S.expected(op, dtype, srcs, 0, False) == srcs[0]).all()
    assert S.expected(op, dtype, srcs, 0, True) == S.UNTOUCHED
    for j in range(1, 9):
        assert same(S.expected(op, dtype, srcs, j, True), S.expected(op, dtype, srcs, j - 1, False), op, dtype)
    # each prefix is one model step on the one before
    for j in range(1, 9):
        step = _half_ref.step(op, dtype, S.prefix(op, dtype, srcs, j - 1), srcs[j])
        assert (step == S.prefix(op, dtype, srcs, j)).all()


def test_generated_sources_are_nan_rich_where_it_matters():
    for dtype in ("float", "double", "complexf", "complexd"):
        srcs = S.sources("sum", dtype, 3, 257, 5)
        x = srcs[1]
        nan = np.isnan(x.real) | np.isnan(x.imag) if dtype.startswith("complex") else np.isnan(x)
        assert nan.sum() > 40, dtype
    assert len(S.sources("sum", "double", 4, 0, 1)[3]) == 0
    assert S.sources("max", "half", 2, 9, 3)[0].dtype == np.uint16
