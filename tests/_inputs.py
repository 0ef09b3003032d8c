"""Seeded inputs shared by the GPU workers and the checking side."""
import numpy as np

import gen_golden


def source(op, dtype, n, seed, pe):
    rng = np.random.default_rng(seed * 1009 + pe)
    if n == 0:
        import oracle
        return np.zeros(0, dtype=oracle.NP[dtype])
    return gen_golden.values(rng, op, dtype, n)


def nan_source(op, dtype, n, seed, pe):
    """The NaN-payload families' generator (gen_golden.nan_values: a third of
    the elements NaNs of random sign, payload and kind) under source()'s
    seeding rule; float, double and the complex types only."""
    assert (op, dtype) in gen_golden.NAN_PAIRS, (op, dtype)
    return gen_golden.nan_values(np.random.default_rng(seed * 1009 + pe), dtype, n)


def finite_source(op, dtype, n, seed, pe):
    """source() without its specials: gen_golden.values plants NaN, +-Inf and
    +-FLT_MAX-sized values in 8 % of the elements (two of them meet in one
    element of most calls from a few thousand elements on), so a call meant to
    come out NaN-free takes these: every element that is not finite, or so
    large that a short chain of sums or products of it could overflow, becomes
    1. float and double only."""
    assert dtype in ("float", "double"), dtype
    x = source(op, dtype, n, seed, pe).copy()
    with np.errstate(invalid="ignore"):
        x[~(np.abs(x) <= 256)] = 1
    return x


def by_kind(kind, op, dtype, n, seed, pe):
    """the "inputs" entries of a stream case (tests/pe_worker.py run_stream)"""
    return {"finite": finite_source, "nan": nan_source, "default": source}[kind](op, dtype, n, seed, pe)


def paths_source(op, dtype, n, spacing, member):
    """Member `member`'s source of a directed-table case ("inputs": "paths"):
    the operand table of tests/_op_paths.py spread over n elements, one row
    every `spacing` elements among plain finite ones and repeated to the end.
    Member 0 holds the accumulators and member 1 the incoming operands, so the
    two meet as (acc, src) in the order the table names; further members hold
    plain elements (the special result is carried on)."""
    import _op_paths
    return _op_paths.spaced_layout(op, dtype, n, spacing, member)
