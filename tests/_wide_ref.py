"""The wide sums' model (include/shmemx.h "wide sum", csrc/wide.hip): plain numpy.

The reference has no half or bfloat16, and nothing that accumulates wider than
its element type, so this file is the definition mi355_combine_wide and
shmemx_<T>_wsum_to_all / _wsum_to_all_float are held to, bit for bit. Elements
are uint16 bit patterns throughout; the float result is uint32 bit patterns.

  acc = float32(src_0)                                 exact widening
  for j in 1 .. N-1:  acc = fl32(acc + float32(src_j)) ascending, on every member
  result_T     = round_to_T(acc)   one rounding: nearest even, subnormals kept,
                                   overflow to +-inf; NaN -> 0x7E00 / 0x7FC0
  result_float = bits of acc       NaN -> 0x7FC00000

fl32 is the IEEE binary32 add (nearest even, subnormal operands and results
kept): numpy's float32 add on the host, which tests/test_wide_ref.py checks
against the exact integer adder of tests/_fp_add_cases.py.
"""
import numpy as np

from _half_ref import CANONICAL_NAN, TYPES, left_fold, round_to, widen  # noqa: F401

FLOAT_NAN = 0x7FC00000
MANT = {"half": 10, "bfloat16": 7}
INF = {"half": 0x7C00, "bfloat16": 0x7F80}
ONE = {"half": 0x3C00, "bfloat16": 0x3F80}
# the largest finite value of the type, and its smallest normal
T_MAX = {"half": np.float32(65504.0), "bfloat16": np.float32(np.uint32(0x7F7F0000).view(np.float32))}
T_MIN_NORMAL = {"half": np.float32(2.0 ** -14), "bfloat16": np.float32(2.0 ** -126)}


def add32(a, b):
    """fl32(a + b), element-wise"""
    with np.errstate(all="ignore"):
        return np.add(np.asarray(a, np.float32), np.asarray(b, np.float32), dtype=np.float32)


def partials(dtype, sources_bits):
    """the running binary32 sums after source 0, 1, ..., N-1 (float32 arrays)"""
    acc = widen(dtype, sources_bits[0]).copy()
    out = [acc]
    for s in sources_bits[1:]:
        acc = add32(acc, widen(dtype, s))
        out.append(acc)
    return out


def accumulate(dtype, sources_bits):
    return partials(dtype, sources_bits)[-1]


def wsum(dtype, sources_bits):
    """the 16-bit result: uint16 bit patterns"""
    return round_to(dtype, accumulate(dtype, sources_bits))


def wsum_float(dtype, sources_bits):
    """the float result: uint32 bit patterns"""
    acc = accumulate(dtype, sources_bits)
    return np.where(np.isnan(acc), np.uint32(FLOAT_NAN), acc.view(np.uint32)).astype(np.uint32)


def result(dtype, out_float, sources_bits):
    return wsum_float(dtype, sources_bits) if out_float else wsum(dtype, sources_bits)


# ---------------------------------------------------------------------------
# what an input set exercises
# ---------------------------------------------------------------------------
# "subnormal": for bfloat16 a binary32-subnormal running sum. Every half is a
# multiple of 2^-24, so no sum of halves is a binary32 subnormal (2^-126 and
# below): for half the class is a nonzero running sum below half's smallest
# normal, 2^-14 -- the subnormal path of the widening and narrowing converts.
RULES = ("differs", "tie", "excursion", "subnormal", "nan", "inf", "zero")


def _is_tie(dtype, acc):
    """acc is exactly half way between two neighbours of the type"""
    acc = np.asarray(acc, np.float32)
    fin = np.isfinite(acc)
    if dtype == "bfloat16":
        return fin & ((acc.view(np.uint32) & 0xFFFF) == 0x8000)
    with np.errstate(all="ignore"):
        h = acc.astype(np.float16)
        toward = np.where(acc.astype(np.float64) > h.astype(np.float64), np.float16(np.inf), np.float16(-np.inf))
        h2 = np.nextafter(h, toward.astype(np.float16))
        d1 = np.abs(acc.astype(np.float64) - h.astype(np.float64))
        d2 = np.abs(acc.astype(np.float64) - h2.astype(np.float64))
        return fin & np.isfinite(h) & np.isfinite(h2) & (d1 != 0) & (d1 == d2)


def rules_hit(dtype, sources_bits):
    """{class: number of elements} of RULES, counted on the model alone"""
    n_src = len(sources_bits)
    parts = partials(dtype, sources_bits)
    acc = parts[-1]
    res = round_to(dtype, acc)
    mag = res & 0x7FFF
    res_nan, res_inf = mag > INF[dtype], mag == INF[dtype]
    with np.errstate(all="ignore"):
        beyond = np.zeros(acc.shape, bool)
        for p in parts[1:n_src - 1]:                      # intermediates: neither the first source nor the end
            beyond |= np.isfinite(p) & (np.abs(p) > T_MAX[dtype])
        sub = np.zeros(acc.shape, bool)
        for p in parts[1:]:
            sub |= (p != 0) & (np.abs(p) < T_MIN_NORMAL[dtype])
    neg_zero_in = np.zeros(acc.shape, bool)
    for s in sources_bits:
        neg_zero_in |= np.asarray(s, np.uint16) == 0x8000
    hit = {
        "differs": res != left_fold("sum", dtype, sources_bits),
        "tie": _is_tie(dtype, acc),
        "excursion": beyond & ~res_nan & ~res_inf,
        "subnormal": sub,
        "nan": res_nan,
        "inf": res_inf,
        "zero": (acc == 0) & neg_zero_in,
    }
    return {k: int(v.sum()) for k, v in hit.items()}


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
# What the GPU tests draw their inputs with: the seeds, and every (source
# count, size) with nsrc >= 3 and n >= 257 -- the one table both sides read.
# tests/test_wide_ref.py asserts the condition on the inputs (every class hit,
# 5 % or more of the elements unlike the stepwise fold) for exactly these;
# tests/test_gpu_wide_kernel.py and tests/test_gpu_wide.py take their shapes
# from here (gpu_shape) and so cannot use one that is not asserted.
SEEDS = (1, 7001)
GPU_NSRC = (3, 4, 5, 8, 9, 32)
GPU_N = (257, 4099, 40000)
GPU_CUS = 256                   # the MI355X; the second-grid-pass case's size follows from it
PASS_EXTRA = 4099               # ... n = one grid pass + this
BLOCKS_PER_CU, BLOCK = 4, 256   # csrc/wide_plan.h; tests/test_wide_plan.py holds the library to these
PER_LANE = {False: 8, True: 4}  # elements of a lane's unit, by float output


def grid_pass(out_float, cus=GPU_CUS):
    """elements one pass of a saturating vector-form grid covers (mi355_combine_wide_plan)"""
    return cus * BLOCKS_PER_CU * BLOCK * PER_LANE[bool(out_float)]


def gpu_shapes():
    """every (nsrc, n) with nsrc >= 3 and n >= 257 a GPU test draws inputs at"""
    shapes = {(k, n) for k in GPU_NSRC for n in GPU_N}
    shapes |= {(3, grid_pass(f) + PASS_EXTRA) for f in (False, True)}
    return sorted(shapes)


def gpu_shape(nsrc, n):
    """(nsrc, n), checked: a shape the CPU test asserts the input condition for"""
    assert nsrc < 3 or n < 257 or (nsrc, n) in gpu_shapes(), f"({nsrc}, {n}) is not in _wide_ref.gpu_shapes()"
    return nsrc, n


def crafted_rows(dtype):
    """[(source 0, source 1, source 2, the pattern of every further source)]:
    one element each, hand-made for the classes of RULES"""
    m, one, inf = MANT[dtype], ONE[dtype], INF[dtype]
    half_ulp = one - ((m + 1) << m)                    # 2^-(m+1): half an ulp of 1.0
    neg, z, nz = 0x8000, 0x0000, 0x8000
    if dtype == "half":
        big, lift = 0x7B53, 0x7B53                     # 60000 + 60000 - 60000
    else:
        big, lift = 0x7F7F, 0x7B00                     # max + 2^119 - 2^119: 2^128 - 2^119 is beyond max
    return [
        (big, lift, lift | neg, z),                    # excursion; the stepwise fold overflows
        (one, half_ulp, z, z),                         # tie, to the even neighbour below
        (one + 1, half_ulp, z, z),                     # tie, to the even neighbour above
        (one, half_ulp, half_ulp, z),                  # two half ulps: 1 + ulp wide, 1 stepwise
        (0x0001, 0x0001, 0x8001, z),                   # subnormals
        (0x0001, 0x0001, z, z),
        (inf, inf | neg, one, z),                      # inf - inf
        (inf | 1, one, one, z),                        # a signalling NaN in
        (inf | (1 << (m - 1)) | 5 | neg, one, one, z),   # a quiet NaN with a payload and a sign
        (inf, one, one | neg, z),                      # an infinity in
        (inf - 1, inf - 1, one, z),                    # max + max: past the type's range, an infinity out
        (nz, nz, nz, nz),                              # -0 + -0 ... = -0
        (nz, z, nz, nz),                               # -0 + +0 = +0
        (one, one | neg, nz, nz),                      # x - x = +0, + -0 = +0
    ]


def sources(dtype, nsrc, n, seed):
    """nsrc arrays of n bit patterns, seeded. Elements whose index is a
    multiple of 4 walk crafted_rows (where nsrc >= 3; with fewer sources they
    are random like the rest); every 16th of the others is random in all 16
    bits (NaNs, infinities, subnormals, far-apart exponents); the rest share
    an exponent to within 3 across the sources, random significands and signs,
    so that most steps of a stepwise fold round."""
    m = MANT[dtype]
    emax = 0x7FFF >> m
    rng = np.random.default_rng([seed, nsrc, n, m])
    centre = rng.integers(4, emax - 4, n)
    out = []
    for _ in range(nsrc):
        e = np.clip(centre + rng.integers(-3, 4, n), 0, emax)
        rest = rng.integers(0, 1 << m, n) | (rng.integers(0, 2, n) << 15)
        v = ((e << m) | rest).astype(np.uint16)
        wild = rng.integers(0, 1 << 16, n, dtype=np.uint16)
        v[1::16] = wild[1::16]
        out.append(v)
    if nsrc >= 3:
        rows = crafted_rows(dtype)
        idx = np.arange(0, n, 4)
        for k in range(nsrc):
            out[k][idx] = np.array([r[min(k, 3)] for r in rows], np.uint16)[(idx // 4) % len(rows)]
    return out
