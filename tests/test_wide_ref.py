"""CPU: the wide sums' model (tests/_wide_ref.py) checks itself -- its binary32
add against the exact integer adder of tests/_fp_add_cases.py, hand-written
rows, and the condition on the inputs the GPU tests rely on: for every (type,
source count, size) they use, the generator alone hits every class of the
model and the wide result differs from the stepwise 16-bit fold on at least
5 % of the elements, so a kernel that were the old fold could not pass."""
import numpy as np
import pytest

import _fp_add_cases as A
import _half_ref as H
import _wide_ref as W

# the (nsrc >= 3, n >= 257) of tests/test_gpu_wide_kernel.py and tests/test_gpu_wide.py are
# W.gpu_shapes(): both draw their shapes through W.gpu_shape, which refuses any other
MIN_DIFFERENT = 0.05


def test_the_hosts_float32_add_is_the_exact_adder():
    t, s = A.cases("float")
    want, nan = A.expected("float")
    got = W.add32(t, s)
    assert A.mismatches("float", got) is None, A.mismatches("float", got)
    assert (np.isnan(got) == nan).all()
    assert (got.view(np.uint32)[~nan] == want[~nan]).all()


def h(x):
    return int(np.array([x], np.float16).view(np.uint16)[0])


def bf(x):
    b = np.array([x], np.float32).view(np.uint32)[0]
    assert b & 0xFFFF == 0, x
    return int(b >> 16)


def f32(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def run(dtype, *vals):
    srcs = [np.array([v], np.uint16) for v in vals]
    return int(W.wsum(dtype, srcs)[0]), int(W.wsum_float(dtype, srcs)[0]), srcs


def test_half_excursion_beyond_the_range_comes_back():
    r16, r32, srcs = run("half", h(60000), h(60000), h(-60000))
    assert r16 == h(60000) and r32 == f32(60000.0)
    assert int(H.left_fold("sum", "half", srcs)[0]) == 0x7C00      # the stepwise fold: inf for good


def test_one_plus_two_to_the_minus_twelve_eight_times_in_bfloat16():
    """1 + 2^-12 + ... + 2^-12: every stepwise sum rounds back to 1; the wide
    sum keeps the terms -- 1 + 2^-9 in the float result after eight of them, and
    after 32 of them the 16-bit result moves, to 1 + 2^-7"""
    one, eps = 0x3F80, bf(2.0 ** -12)
    r16, r32, arr = run("bfloat16", one, *([eps] * 8))
    assert r32 == f32(1.0 + 2.0 ** -9) and r16 == one
    assert int(H.left_fold("sum", "bfloat16", arr)[0]) == one
    r16, r32, arr = run("bfloat16", one, *([eps] * 32))
    assert r32 == f32(1.0 + 2.0 ** -7) and r16 == one + 1
    assert int(H.left_fold("sum", "bfloat16", arr)[0]) == one      # the stepwise fold loses all 32


@pytest.mark.parametrize("dtype", W.TYPES)
def test_final_rounding_ties_go_to_even_both_ways(dtype):
    one, m = W.ONE[dtype], W.MANT[dtype]
    half_ulp = one - ((m + 1) << m)
    assert run(dtype, one, half_ulp)[0] == one                   # down to the even 1.0
    assert run(dtype, one + 1, half_ulp)[0] == one + 2           # up to the even 1 + 2 ulp
    assert run(dtype, one | 0x8000, half_ulp | 0x8000)[0] == one | 0x8000
    assert run(dtype, (one + 1) | 0x8000, half_ulp | 0x8000)[0] == (one + 2) | 0x8000
    assert run(dtype, one, half_ulp, half_ulp)[0] == one + 1     # not a tie twice, as stepwise


def test_two_bfloat16_subnormals_sum_to_a_binary32_subnormal():
    r16, r32, _ = run("bfloat16", 0x0001, 0x0003)
    assert r32 == 0x00040000 and r16 == 0x0004
    assert 0 < np.uint32(r32).view(np.float32) < np.float32(2.0 ** -126)
    r16, r32, _ = run("bfloat16", 0x0001, 0x8003)
    assert r32 == 0x80020000 and r16 == 0x8002


def test_half_subnormals_are_kept():
    assert run("half", 0x0001, 0x0001)[:2] == (0x0002, f32(2.0 ** -23))
    assert run("half", 0x03FF, 0x0001)[0] == 0x0400              # into the smallest normal


@pytest.mark.parametrize("dtype", W.TYPES)
def test_signed_zeros(dtype):
    assert run(dtype, 0x8000, 0x8000)[:2] == (0x8000, 0x80000000)
    assert run(dtype, 0x8000, 0x0000)[:2] == (0x0000, 0x00000000)
    assert run(dtype, 0x8000)[:2] == (0x8000, 0x80000000)
    one = W.ONE[dtype]
    assert run(dtype, one, one | 0x8000, 0x8000)[:2] == (0x0000, 0x00000000)


@pytest.mark.parametrize("dtype", W.TYPES)
def test_every_nan_is_canonical_in_both_outputs(dtype):
    inf, m, canon = W.INF[dtype], W.MANT[dtype], W.CANONICAL_NAN[dtype]
    one = W.ONE[dtype]
    assert run(dtype, inf, inf | 0x8000)[:2] == (canon, W.FLOAT_NAN)             # inf - inf
    assert run(dtype, inf | 1, one)[:2] == (canon, W.FLOAT_NAN)                  # a signalling NaN in
    for nan in (inf | 1, inf | (1 << (m - 1)) | 3, inf | 0x8000 | (1 << (m - 1))):
        assert run(dtype, nan)[:2] == (canon, W.FLOAT_NAN), hex(nan)             # N = 1: not a byte copy
    assert run(dtype, inf, one)[:2] == (inf, f32(np.inf))
    assert run(dtype, inf | 0x8000)[:2] == (inf | 0x8000, f32(-np.inf))


def test_overflow_happens_at_the_one_rounding():
    assert run("half", h(65504), h(65504), h(-65504))[0] == h(65504)
    assert run("half", h(65504), h(65504))[:2] == (0x7C00, f32(131008.0))
    assert run("half", h(65504), h(16))[0] == 0x7C00             # 65520: the tie at the top goes to inf
    assert run("half", h(65504), h(8))[0] == h(65504)
    assert run("bfloat16", 0x7F7F, 0x7F7F)[:2] == (0x7F80, f32(np.inf))


@pytest.mark.parametrize("dtype", W.TYPES)
def test_crafted_rows_hit_the_class_they_are_for(dtype):
    rows = W.crafted_rows(dtype)
    hits = [W.rules_hit(dtype, [np.array([r[min(k, 3)]], np.uint16) for k in range(5)]) for r in rows]
    for rule in W.RULES:
        assert any(hh[rule] for hh in hits), rule


def test_the_classifier_is_silent_on_plain_sums():
    for dtype in W.TYPES:
        one = W.ONE[dtype]
        hit = W.rules_hit(dtype, [np.array([one], np.uint16)] * 3)
        assert all(v == 0 for v in hit.values()), hit


@pytest.mark.parametrize("dtype", W.TYPES)
@pytest.mark.parametrize("nsrc,n", W.gpu_shapes())
def test_the_generator_alone_hits_every_class(dtype, nsrc, n):
    for seed in W.SEEDS:
        srcs = W.sources(dtype, nsrc, n, seed)
        assert len(srcs) == nsrc and all(s.dtype == np.uint16 and s.shape == (n,) for s in srcs)
        hit = W.rules_hit(dtype, srcs)
        for rule in W.RULES:
            assert hit[rule] > 0, (dtype, nsrc, n, seed, rule, hit)
        assert hit["differs"] >= MIN_DIFFERENT * n, (dtype, nsrc, n, seed, hit["differs"] / n)
        again = W.sources(dtype, nsrc, n, seed)
        assert all((a == b).all() for a, b in zip(srcs, again))


def test_the_shape_table_covers_what_it_says():
    shapes = W.gpu_shapes()
    assert all(k >= 3 and n >= 257 for k, n in shapes)
    assert {(k, n) for k in W.GPU_NSRC for n in W.GPU_N} <= set(shapes)
    assert (3, 256 * 4 * 256 * 8 + 4099) in shapes and (3, 256 * 4 * 256 * 4 + 4099) in shapes
    assert W.gpu_shape(2, 10 ** 7) == (2, 10 ** 7) and W.gpu_shape(32, 9) == (32, 9)     # outside the condition
    with pytest.raises(AssertionError):
        W.gpu_shape(5, 261)


def test_the_result_does_not_depend_on_who_asks():
    """one order for every member: the model takes no member index at all, and
    differs from the per-member folds of the stepwise model"""
    srcs = W.sources("bfloat16", 4, 4099, 3)
    per_member = {H.fold("sum", "bfloat16", srcs, q).tobytes() for q in range(4)}
    assert len(per_member) > 1
    assert W.wsum("bfloat16", srcs).tobytes() not in per_member
