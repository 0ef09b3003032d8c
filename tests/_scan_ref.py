"""Expected values of the scan collectives and of mi355_combine_prefix (test
infrastructure): no operator is restated here. Prefix k of the sources is the
ascending left fold of srcs[:k + 1], which for the reference's types is what
the reference computes on the FIRST member of a set of those k + 1 members
(oracle.reduce_pe(op, dtype, srcs[:k + 1], 0)) and for the 16-bit floats the
model's left fold (tests/_half_ref.py). Compare with tests/_compare.py (the
reference's types: every value bit, long double's 10 bytes) or bit patterns
(the 16-bit floats, uint16)."""
import numpy as np

import _half_ref
import oracle

UNTOUCHED = "untouched"
HALF_TYPES = _half_ref.TYPES
HALF_PAIRS = [(op, t) for t in _half_ref.TYPES for op in _half_ref.OPS]
PAIRS = list(oracle.PAIRS) + HALF_PAIRS
assert len(PAIRS) == 52
NP = dict(oracle.NP, half=np.uint16, bfloat16=np.uint16)   # the 16-bit floats as their bit patterns


def prefix(op, dtype, srcs, k):
    """srcs[0] op srcs[1] op ... op srcs[k], the accumulator on the left"""
    if dtype in HALF_TYPES:
        return _half_ref.left_fold(op, dtype, srcs[:k + 1])
    return oracle.reduce_pe(op, dtype, srcs[:k + 1], 0)


def expected(op, dtype, srcs, j, exclusive):
    """member j's result (srcs in active-set order); UNTOUCHED for exscan's member 0"""
    k = j - 1 if exclusive else j
    if k < 0:
        return UNTOUCHED
    return prefix(op, dtype, srcs, k)


def differing(got, want, op, dtype):
    """indices where got != want"""
    if dtype in HALF_TYPES:
        got = np.ascontiguousarray(got).view(np.uint16)
        want = np.ascontiguousarray(want).view(np.uint16)
        assert got.shape == want.shape, (got.shape, want.shape)
        return np.nonzero(got != want)[0]
    import _compare
    return _compare.mismatches(got, want, op, dtype, strict=True)


def sources(op, dtype, nsrc, n, seed):
    """seeded sources: the golden fixtures' generator (NaN-rich for float,
    double and complex sum/prod), the model's special-value table for the
    16-bit floats"""
    if dtype in HALF_TYPES:
        return _half_ref.sources(dtype, nsrc, n, seed)
    import gen_golden
    out = []
    for k in range(nsrc):
        rng = np.random.default_rng(seed * 1009 + k)
        if n == 0:
            out.append(np.zeros(0, dtype=oracle.NP[dtype]))
        elif (op, dtype) in gen_golden.NAN_PAIRS and k % 2 == 1:
            out.append(gen_golden.nan_values(rng, dtype, n))
        else:
            out.append(gen_golden.values(rng, op, dtype, n))
    return out
