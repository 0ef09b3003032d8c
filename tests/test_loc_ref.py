"""CPU: the model of the value-and-location reductions (tests/_loc_ref.py)
against hand-written cases for every rule, and the property that makes the
result independent of the schedule: without a double tie, every order of the
members gives the same pair."""
import itertools

import numpy as np
import pytest

import _loc_ref as L

F = lambda *x: np.array(x, dtype=np.float32).view(np.uint32)   # noqa: E731
U = lambda *x: np.array(x, dtype=np.uint32)                    # noqa: E731
I64 = lambda *x: np.array(x, dtype=np.int64)                   # noqa: E731
QNAN, NAN2 = 0x7FC00000, 0xFFC12345


def one(op, dtype, pairs, **kw):
    """fold of one element: pairs = [(pattern, loc or None), ...] -> (pattern, loc)"""
    vals = [np.array([v], dtype=L.STORE[dtype]) for v, _ in pairs]
    locs = [None if l is None else I64(l) for _, l in pairs]
    v, l = L.fold(op, dtype, vals, locs, **kw)
    return int(v[0]), int(l[0])


@pytest.mark.parametrize("op", L.OPS)
def test_nan_beats_every_number_in_both_operators(op):
    big, small = int(F(np.inf)[0]), int(F(-np.inf)[0])
    for number in (big, small, int(F(1.0)[0])):
        assert one(op, "float", [(number, 5), (QNAN, 9)]) == (QNAN, 9)      # the later, larger location still wins
        assert one(op, "float", [(QNAN, 9), (number, 5)]) == (QNAN, 9)      # and is not beaten
        assert one(op, "float", [(number, 1), (NAN2, 7), (number, 0)]) == (NAN2, 7)


@pytest.mark.parametrize("op", L.OPS)
def test_two_nans_the_smaller_location_payload_kept(op):
    assert one(op, "float", [(QNAN, 4), (NAN2, 3)]) == (NAN2, 3)
    assert one(op, "float", [(NAN2, 3), (QNAN, 4)]) == (NAN2, 3)
    assert one(op, "float", [(QNAN, 4), (NAN2, 4)]) == (QNAN, 4)            # equal locations: the lower member
    assert one(op, "double", [(0x7FF8000000000001, -2), (0xFFF8000000000002, -3)]) == (0xFFF8000000000002, -3)


@pytest.mark.parametrize("op", L.OPS)
def test_zero_signs_are_equal_and_bits_survive(op):
    pz, nz = int(F(0.0)[0]), int(F(-0.0)[0])
    assert one(op, "float", [(pz, 2), (nz, 1)]) == (nz, 1)
    assert one(op, "float", [(nz, 2), (pz, 1)]) == (pz, 1)
    assert one(op, "float", [(nz, 1), (pz, 1)]) == (nz, 1)
    assert one(op, "float", [(pz, 1), (nz, 1)]) == (pz, 1)
    # 16-bit patterns that differ with equal values: half +-0, bfloat16 +-0
    for dtype in ("half", "bfloat16"):
        assert one(op, dtype, [(0x0000, 9), (0x8000, 8)]) == (0x8000, 8)
        assert one(op, dtype, [(0x8000, 8), (0x0000, 8)]) == (0x8000, 8)


def test_values_decide_before_locations():
    assert one("max", "int", [(3, 0), (7, 9), (5, 1)]) == (7, 9)
    assert one("min", "int", [(3, 5), (7, 0), (3, 4)]) == (3, 4)
    assert one("max", "half", [(0x3C00, 1), (0x4000, 2)]) == (0x4000, 2)     # 1.0, 2.0
    assert one("min", "bfloat16", [(0x3F80, 1), (0xBF80, 2)]) == (0xBF80, 2)  # 1.0, -1.0
    assert one("max", "short", [(-32768, 1), (32767, 2)]) == (32767, 2)
    assert one("min", "long", [(-2 ** 63, 4), (2 ** 63 - 1, 2)]) == (-2 ** 63, 4)
    # half compares by value, not by pattern: -2.0 (0xC000) < 1.0 (0x3C00) although its pattern is larger
    assert one("max", "half", [(0xC000, 1), (0x3C00, 2)]) == (0x3C00, 2)


def test_equal_value_and_location_keeps_the_lower_member():
    # distinguishable only through a third property: the patterns (+0 / -0)
    assert one("max", "double", [(0, 3), (1 << 63, 3), (0, 3)]) == (0, 3)
    assert one("min", "int", [(4, 3), (4, 3)]) == (4, 3)


def test_negative_and_implicit_locations():
    assert one("max", "int", [(4, -1), (4, -7), (4, 2)]) == (4, -7)
    assert one("max", "int", [(4, None), (4, None), (9, None)]) == (9, 2)
    assert one("min", "int", [(4, None), (4, None)]) == (4, 0)
    assert one("min", "int", [(4, None), (4, None)], loc_base=31) == (4, 31)
    assert one("min", "int", [(4, 40), (4, None), (3, None)], loc_base=31) == (3, 33)   # mixed: entry j is loc_base + j
    v, l = L.fold("max", "float", [F(1.0, 2.0)], None)
    assert (v == F(1.0, 2.0)).all() and (l == 0).all()                         # one member: a copy and a fill


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("op", L.OPS)
def test_every_member_order_gives_the_same_pair_without_double_ties(op, dtype):
    n, members = 4000, 4
    vals, locs = L.inputs(dtype, members, n, seed=99)
    # no double tie: no two members with equal class and equal location at one element
    keep = np.ones(n, dtype=bool)
    for a, b in itertools.combinations(range(members), 2):
        counts = {}
        L.count_rules(op, dtype, vals[a], locs[a], vals[b], locs[b], counts)
        va, na = L.denoted(vals[a], dtype)
        vb, nb = L.denoted(vals[b], dtype)
        with np.errstate(invalid="ignore"):
            same_class = (na & nb) | (~na & ~nb & (va == vb))
        keep &= ~(same_class & (locs[a] == locs[b]))
    assert 200 < keep.sum() < n, keep.sum()
    vals = [v[keep] for v in vals]
    locs = [l[keep] for l in locs]
    want = L.fold(op, dtype, vals, locs)
    for perm in itertools.permutations(range(members)):
        got = L.fold(op, dtype, [vals[i] for i in perm], [locs[i] for i in perm])
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), perm


def test_the_generated_inputs_exercise_every_rule():
    for dtype in ("float", "bfloat16", "int"):
        counts = {}
        vals, locs = L.inputs(dtype, 3, 40000, seed=5)
        L.fold("max", dtype, vals, locs, counts=counts)
        for rule in L.rules_of(dtype):
            assert counts.get(rule, 0) > 0, (dtype, rule, counts)
