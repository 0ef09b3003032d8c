"""CPU: the 16-bit float model (tests/_half_ref.py) against independent
implementations, so the definition the GPU tests compare with cannot drift.

Every 16-bit pattern with 64 partners each (half of them near in exponent):
4.2 M pairs per type. bfloat16: torch's CPU bfloat16 + and *; half: numpy's
native float16 + and *. Non-NaN results must agree bit for bit, NaN-ness
everywhere; the model's NaNs are canonical. The same on product_pairs (every
pattern with 64 partners aimed at the product's edges), and the properties of
both sets that tests/test_gpu_half_pairs.py relies on.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _half_ref as R
import shmem_reduce

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch_bf16(tmp_path_factory):
    """torch's results, from a child process (tests/_half_torch_native.py):
    torch brings its own HIP runtime and this process may hold the library's"""
    out = str(tmp_path_factory.mktemp("half_ref") / "torch_bf16.npz")
    subprocess.run([sys.executable, os.path.join(HERE, "_half_torch_native.py"), out], check=True, timeout=300)
    return np.load(out)


def native(dtype, op, pairs, a, b, torch_bf16):
    if dtype == "bfloat16":
        return torch_bf16[f"{pairs}_{op}"]
    with np.errstate(all="ignore"):
        x, y = a.view(np.float16), b.view(np.float16)
        return (x + y if op == "sum" else x * y).view(np.uint16)


def is_nan(dtype, bits):
    return np.isnan(R.widen(dtype, bits))


@pytest.mark.parametrize("dtype", R.TYPES)
@pytest.mark.parametrize("op", ["sum", "prod"])
def test_model_equals_native_arithmetic(dtype, op, torch_bf16):
    model_equals_native(dtype, op, "exhaustive", torch_bf16)


@pytest.mark.parametrize("dtype", R.TYPES)
@pytest.mark.parametrize("op", ["sum", "prod"])
def test_model_equals_native_arithmetic_on_product_pairs(dtype, op, torch_bf16):
    """the same on the product-edge set: subnormal, underflowing and
    overflowing results are where a rounding model goes wrong"""
    model_equals_native(dtype, op, "product", torch_bf16)


def model_equals_native(dtype, op, pairs, torch_bf16):
    a, b = R.PAIR_SETS[pairs](dtype)
    got = R.step(op, dtype, a, b)
    want = native(dtype, op, pairs, a, b, torch_bf16)
    nan_g, nan_w = is_nan(dtype, got), is_nan(dtype, want)
    assert (nan_g == nan_w).all()
    assert (got[nan_g] == R.CANONICAL_NAN[dtype]).all()
    bad = np.nonzero((got != want) & ~nan_g)[0]
    assert bad.size == 0, (hex(a[bad[0]]), hex(b[bad[0]]), hex(got[bad[0]]), hex(want[bad[0]]))
    # commutative, NaNs included: the two-member sum/prod needs no per-member order
    assert (R.step(op, dtype, b, a) == got).all()


def bits_of(dtype, value):
    if dtype == "half":
        return int(np.array([value], dtype=np.float16).view(np.uint16)[0])
    f = np.array([value], dtype=np.float32)
    assert (f.view(np.uint32) & 0xFFFF == 0).all(), value   # exactly representable
    return int(f.view(np.uint32)[0] >> 16)


def one_step(op, dtype, a, b):
    return int(R.step(op, dtype, np.array([a], dtype=np.uint16), np.array([b], dtype=np.uint16))[0])


@pytest.mark.parametrize("dtype,p", [("half", 11), ("bfloat16", 8)])
def test_ties_go_to_even(dtype, p):
    """p significant bits: 1 + 2^-p is a tie and rounds to 1 (even);
    (1 + 2^-(p-1)) + 2^-p is a tie and rounds up to 1 + 2^-(p-2) (even)"""
    one, half_ulp = bits_of(dtype, 1.0), bits_of(dtype, 2.0 ** -p)
    assert one_step("sum", dtype, one, half_ulp) == one
    odd = bits_of(dtype, 1.0 + 2.0 ** -(p - 1))
    assert one_step("sum", dtype, odd, half_ulp) == bits_of(dtype, 1.0 + 2.0 ** -(p - 2))
    # just above the tie rounds up
    assert one_step("sum", dtype, one, half_ulp + 1) == one + 1


@pytest.mark.parametrize("dtype", R.TYPES)
def test_overflow_subnormals_and_nans(dtype):
    inf = 0x7C00 if dtype == "half" else 0x7F80
    big = inf - 1
    assert one_step("sum", dtype, big, big) == inf
    assert one_step("prod", dtype, big, big | 0x8000) == inf | 0x8000
    assert one_step("sum", dtype, 0x0001, 0x0001) == 0x0002          # subnormals kept, both sides
    assert one_step("sum", dtype, 0x0001, 0x8001) == 0x0000
    assert one_step("prod", dtype, 0x0001, bits_of(dtype, 2.0)) == 0x0002
    canon = R.CANONICAL_NAN[dtype]
    assert one_step("sum", dtype, inf, inf | 0x8000) == canon        # invalid: sign clear
    assert one_step("prod", dtype, 0x0000, inf) == canon
    for nan in (inf | 1, inf | 0x8000 | 3, canon | 0x8000 | 1):
        assert one_step("sum", dtype, nan, 0x3C00) == canon
        assert one_step("prod", dtype, 0x3C00, nan) == canon
        # min/max: `a < b ? a : b` is false with a NaN: the SECOND operand, bits unchanged
        assert one_step("min", dtype, nan, 0x3C00) == 0x3C00
        assert one_step("min", dtype, 0x3C00, nan) == nan
        assert one_step("max", dtype, 0x3C00, nan) == nan
    assert one_step("min", dtype, 0x0000, 0x8000) == 0x8000          # +-0 pair: by position
    assert one_step("min", dtype, 0x8000, 0x0000) == 0x0000
    assert one_step("max", dtype, 0x8000, 0x0000) == 0x0000


@pytest.mark.parametrize("dtype", R.TYPES)
def test_fold_order_and_inputs(dtype):
    srcs = R.sources(dtype, 3, 5000, 42)
    t = R.special_table(dtype)
    assert t.size == 64
    # every ordered pair of table entries meets in sources 0 and 1
    pairs = set(zip(srcs[0][:4096].tolist(), srcs[1][:4096].tolist()))
    assert len(pairs) == 4096
    for q in range(3):
        others = [m for m in range(3) if m != q]
        want = R.step("sum", dtype, R.step("sum", dtype, srcs[q], srcs[others[0]]), srcs[others[1]])
        assert (R.fold("sum", dtype, srcs, q) == want).all()
    # per-step rounding makes the members' sums differ somewhere
    assert (R.fold("sum", dtype, srcs, 0) != R.fold("sum", dtype, srcs, 2)).any()


@pytest.mark.parametrize("dtype", R.TYPES)
def test_product_pairs_reach_the_products_edges(dtype):
    """conditions on the inputs, from the model alone: among the pairs with
    both operands finite and non-zero, the shares of products that are
    subnormal, zero, infinite and in the top two finite binades"""
    mant, emax_field = (10, 31) if dtype == "half" else (7, 255)
    a, b = R.product_pairs(dtype)
    ea, eb = (a & 0x7FFF) >> mant, (b & 0x7FFF) >> mant
    proper = (ea < emax_field) & (eb < emax_field) & (a & 0x7FFF != 0) & (b & 0x7FFF != 0)
    r = R.step("prod", dtype, a, b)[proper] & 0x7FFF
    er = r >> mant
    share = {"subnormal": ((er == 0) & (r != 0)).mean(), "zero": (r == 0).mean(),
             "infinite": (r == emax_field << mant).mean(), "top two binades": ((er == emax_field - 1) | (er == emax_field - 2)).mean()}
    print(dtype, {k: round(float(v), 4) for k, v in share.items()})
    assert not np.isnan(R.widen(dtype, r)).any()    # finite non-zero operands make no NaN
    assert share["subnormal"] >= 0.10, share
    assert share["zero"] >= 0.01, share
    assert share["infinite"] >= 0.05, share
    assert share["top two binades"] >= 0.04, share


@pytest.mark.parametrize("dtype", R.TYPES)
def test_pair_sets_hold_every_pattern_and_order_sensitive_chains(dtype):
    every = np.arange(1 << 16, dtype=np.uint16)
    for pairs in R.PAIR_SETS.values():
        a, b = pairs(dtype)
        assert a.size == b.size == 64 << 16 and a.dtype == b.dtype == np.uint16
        assert (a.reshape(1 << 16, 64) == every[:, None]).all()     # every pattern, 64 partners each
    # the 9-source subset: every 8th pair still holds every pattern as a, with 8 partners
    assert (a[::8].reshape(1 << 16, 8) == every[:, None]).all()
    a, b = R.exhaustive_pairs(dtype)
    c = R.third_operand(dtype, a, b)
    mant = 10 if dtype == "half" else 7
    es, ec = (R.step("sum", dtype, a, b) & 0x7FFF) >> mant, (c & 0x7FFF) >> mant
    assert (np.abs(es.astype(np.int64) - ec)[1::2] <= 3).all()
    assert np.isin(c[::64], R.special_table(dtype)).all() and not np.isfinite(R.widen(dtype, c[::64])).any()
    assert (R.third_operand(dtype, a, b, 1) != c).mean() > 0.9      # another seed, another array
    # per-step rounding makes the members' sums differ: an order mistake cannot pass
    srcs = [a, b, c]
    assert (R.fold("sum", dtype, srcs, 0) != R.fold("sum", dtype, srcs, 2)).sum() >= 1000
    assert (R.fold("min", dtype, srcs[:2], 0) != R.fold("min", dtype, srcs[:2], 1)).sum() >= 1000


def test_bf16_helpers_equal_the_model():
    """shmem_reduce.bf16_from_f32 on every upper half (low 16 bits zero, and
    the tie and near-tie low halves) against the model's rounding"""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    for low in (0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x0001):
        f = (hi | low).view(np.float32)
        assert (shmem_reduce.bf16_from_f32(f) == R.round_to("bfloat16", f)).all(), hex(low)
    bits = np.arange(1 << 16, dtype=np.uint16)
    back = shmem_reduce.bf16_to_f32(bits)
    assert back.dtype == np.float32 and (back.view(np.uint32) == hi).all()
    assert shmem_reduce.bf16_from_f32([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8]).tolist() == [0x3F80, 0x3F82]
    assert shmem_reduce.bf16_from_f32(np.array([np.nan, -np.nan], dtype=np.float32)).tolist() == [0x7FC0, 0x7FC0]
