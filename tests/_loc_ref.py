"""The specification of the value-and-location reductions (shmemx.h,
shmemx_<T>_maxloc_to_all / _minloc_to_all; mi355_reduce.h, mi355_combine_loc)
as a numpy model on bit patterns -- the reference has nothing comparable.

A candidate is a pair (value, location). Values travel as their storage
patterns (STORE[dtype]: the integer types as themselves, float / double / half /
bfloat16 as unsigned integers of their width) so that "the winner's bits
unchanged" is an integer comparison; locations are int64.

  b beats a (maxloc)  <=>  b.v is a NaN and (a.v is not a NaN or b.l < a.l), or
                           neither is a NaN and (b.v > a.v or (b.v == a.v and b.l < a.l))
  minloc: < for > on the values. The fold runs over members 0, 1, ... in
  ascending order from member 0's pair: acc = cand if beats(cand, acc) else acc.
"""
import numpy as np

OPS = ("max", "min")
DTYPES = ("short", "int", "long", "longlong", "float", "double", "half", "bfloat16")
STORE = {"short": np.int16, "int": np.int32, "long": np.int64, "longlong": np.int64,
         "float": np.uint32, "double": np.uint64, "half": np.uint16, "bfloat16": np.uint16}
FLOATS = ("float", "double", "half", "bfloat16")
RULES_INT = ("value", "value_tie_loc", "double_tie")
RULES_FLOAT = RULES_INT + ("nan_beats_number", "number_loses_to_nan", "nan_nan_loc", "nan_nan_double_tie", "zero_signs")


def denoted(bits, dtype):
    """(values as float64 or int64 -- exact for every type here --, isnan mask)"""
    b = np.ascontiguousarray(bits, dtype=STORE[dtype])
    if dtype not in FLOATS:
        return b.astype(np.int64), np.zeros(b.shape, dtype=bool)
    with np.errstate(invalid="ignore"):     # widening a signalling NaN raises the flag; it stays a NaN
        if dtype == "float":
            v = b.view(np.float32).astype(np.float64)
        elif dtype == "double":
            v = b.view(np.float64)
        elif dtype == "half":
            v = b.view(np.float16).astype(np.float64)
        else:
            v = (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return v, np.isnan(v)


def beats(op, dtype, bv, bl, av, al):
    """elementwise: candidate (bv, bl) beats the running (av, al)"""
    b, nb = denoted(bv, dtype)
    a, na = denoted(av, dtype)
    bl, al = np.asarray(bl, dtype=np.int64), np.asarray(al, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        better = b > a if op == "max" else b < a
        number = ~nb & ~na & (better | ((b == a) & (bl < al)))
    return (nb & (~na | (bl < al))) | number


def locations(locs, j, n, loc_base=0):
    """member j's location array: explicit, or the implicit loc_base + j"""
    if locs is None or locs[j] is None:
        return np.full(n, loc_base + j, dtype=np.int64)
    return np.ascontiguousarray(locs[j], dtype=np.int64)


def fold(op, dtype, vals, locs=None, loc_base=0, counts=None):
    """The left fold over the members in ascending order: (bits, locations).
    vals: one STORE[dtype] array per member; locs: None, or a list whose entries
    may be None (implicit). counts: a dict that receives, per rule, how many
    (element, step) pairs exercised it."""
    assert op in OPS and dtype in DTYPES and len(vals) >= 1
    n = len(vals[0])
    av = np.ascontiguousarray(vals[0], dtype=STORE[dtype]).copy()
    al = locations(locs, 0, n, loc_base).copy()
    for j in range(1, len(vals)):
        bv = np.ascontiguousarray(vals[j], dtype=STORE[dtype])
        bl = locations(locs, j, n, loc_base)
        take = beats(op, dtype, bv, bl, av, al)
        if counts is not None:
            count_rules(op, dtype, bv, bl, av, al, counts)
        av = np.where(take, bv, av)
        al = np.where(take, bl, al)
    return av, al


def count_rules(op, dtype, bv, bl, av, al, counts):
    b, nb = denoted(bv, dtype)
    a, na = denoted(av, dtype)
    both = ~nb & ~na
    with np.errstate(invalid="ignore"):
        eq = both & (b == a)
        ne = both & (b != a)
    add = {"value": ne, "value_tie_loc": eq & (bl != al), "double_tie": eq & (bl == al)}
    if dtype in FLOATS:
        add.update({"nan_beats_number": nb & ~na, "number_loses_to_nan": ~nb & na,
                    "nan_nan_loc": nb & na & (bl != al), "nan_nan_double_tie": nb & na & (bl == al),
                    "zero_signs": eq & (np.asarray(bv) != np.asarray(av))})
    for k, m in add.items():
        counts[k] = counts.get(k, 0) + int(np.count_nonzero(m))


def rules_of(dtype):
    return RULES_FLOAT if dtype in FLOATS else RULES_INT


# ---------------------------------------------------------------------------
# inputs built so that the rules fire
# ---------------------------------------------------------------------------
def value_set(dtype):
    """(numbers, NaNs) as STORE[dtype] patterns: +-0, +-inf, a few ordinary
    numbers; NaNs of distinct payloads, quiet and signalling, both signs"""
    if dtype not in FLOATS:
        info = np.iinfo(STORE[dtype])
        return np.array([0, 1, -1, 2, -2, 7, 100, -100, info.max, info.min], dtype=STORE[dtype]), None
    if dtype == "float":
        num = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1.5, -2.25, 3e-39, 1e30], dtype=np.float32).view(np.uint32)
        nan = np.array([0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7F800001, 0xFF923456, 0x7FFFFFFF], dtype=np.uint32)
    elif dtype == "double":
        num = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1.5, -2.25, 3e-310, 1e300]).view(np.uint64)
        nan = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0x7FF0000000000001,
                        0xFFF4567812345678, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64)
    elif dtype == "half":
        num = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1.5, -2.25, 6e-8, 60000.0], dtype=np.float16).view(np.uint16)
        nan = np.array([0x7E00, 0xFE00, 0x7E01, 0x7C01, 0xFD23, 0x7FFF], dtype=np.uint16)
    else:
        num = np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0x3F80, 0xBF80, 0x3FC0, 0xC010, 0x0001, 0x7F00], dtype=np.uint16)
        nan = np.array([0x7FC0, 0xFFC0, 0x7FC1, 0x7F81, 0xFFA3, 0x7FFF], dtype=np.uint16)
    return num, nan


def inputs(dtype, members, n, seed, explicit=True, loc_span=3):
    """(vals, locs): per member n values drawn from value_set (about 5 % NaNs
    for the float types) and, when explicit, locations from a range of
    loc_span values around a per-member offset that may be negative -- so that
    about a quarter of the elements have a value tie and some of those a
    location tie as well. locs is None when not explicit."""
    rng = np.random.default_rng(seed)
    num, nan = value_set(dtype)
    vals, locs = [], []
    for j in range(members):
        # half the draws from the first four numbers: two members tie in about a fifth of the elements
        v = num[np.where(rng.random(n) < 0.5, rng.integers(0, 4, n), rng.integers(0, len(num), n))]
        if nan is not None:
            v = np.where(rng.random(n) < 0.05, nan[rng.integers(0, len(nan), n)], v)
        vals.append(np.ascontiguousarray(v, dtype=STORE[dtype]))
        locs.append(rng.integers(-1, -1 + loc_span, n).astype(np.int64) * 1000003)
    return vals, (locs if explicit else None)
