"""The 16-bit float reductions' model (include/shmemx.h): plain numpy.

The reference has no half or bfloat16, so this file is the definition the
kernels are held to, bit for bit. Elements are uint16 bit patterns throughout.

  sum / prod step  r = round_to_T(float32(a) op float32(b)): to nearest, ties
                   to even, subnormals kept, overflow to +-inf; a NaN result is
                   the canonical quiet NaN (0x7E00 half, 0x7FC0 bfloat16)
  min / max step   a < b ? a : b, a > b ? a : b on the values; the chosen
                   operand's bits unchanged (a NaN or a +-0 pair selects by position)
  fold             PE q receives (((src_q op src_m0) op src_m1) ...), m0 < m1 < ...
                   the members other than q
"""
import functools

import numpy as np

TYPES = ("half", "bfloat16")
OPS = ("sum", "prod", "min", "max")
CANONICAL_NAN = {"half": 0x7E00, "bfloat16": 0x7FC0}


def widen(dtype, bits):
    """bit patterns -> the float32 values they denote (exact for both types)"""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "half":
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def round_to(dtype, r):
    """float32 -> bit patterns, round to nearest even; NaN -> canonical"""
    r = np.ascontiguousarray(r, dtype=np.float32)
    with np.errstate(all="ignore"):
        if dtype == "half":
            bits = r.astype(np.float16).view(np.uint16)
        else:
            u = r.view(np.uint32).astype(np.uint64)
            bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(r), np.uint16(CANONICAL_NAN[dtype]), bits).astype(np.uint16)


def step(op, dtype, a, b):
    """one operator application on bit patterns: a is the accumulator (left)"""
    a = np.ascontiguousarray(a, dtype=np.uint16)
    b = np.ascontiguousarray(b, dtype=np.uint16)
    x, y = widen(dtype, a), widen(dtype, b)
    with np.errstate(all="ignore"):
        if op == "sum":
            return round_to(dtype, x + y)
        if op == "prod":
            return round_to(dtype, x * y)
        if op == "min":
            return np.where(x < y, a, b)
        if op == "max":
            return np.where(x > y, a, b)
    raise ValueError(op)


def fold(op, dtype, sources_bits, q):
    """PE q's result: its own source first, then the other members in ascending order"""
    acc = np.ascontiguousarray(sources_bits[q], dtype=np.uint16).copy()
    for m, s in enumerate(sources_bits):
        if m != q:
            acc = step(op, dtype, acc, s)
    return acc


def left_fold(op, dtype, sources_bits):
    """(((s0 op s1) op s2) ...): mi355_combine's order, PE_start's result"""
    return fold(op, dtype, sources_bits, 0)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def special_table(dtype):
    """64 bit patterns: +-0, +-inf, quiet and signalling NaNs (several payloads,
    both signs), subnormal extremes, smallest normal, largest finite, 1.0, the
    tie makers (1 + ulp/2 steps), and neighbours."""
    if dtype == "half":
        mant, one = 10, 0x3C00
    else:
        mant, one = 7, 0x3F80
    exp_all = 0x7FFF & ~((1 << mant) - 1)          # the exponent field all ones: +inf
    quiet = 1 << (mant - 1)
    top = (1 << mant) - 1
    pos = [
        0x0000, exp_all,                            # +0, +inf
        exp_all | quiet, exp_all | quiet | 1, exp_all | top,       # quiet NaNs
        exp_all | 1, exp_all | 2, exp_all | (quiet - 1),           # signalling NaNs
        0x0001, 0x0002, top, top - 1,               # smallest / largest subnormals
        1 << mant, (1 << mant) + 1,                 # smallest normal and its neighbour
        exp_all - 1, exp_all - 2,                   # largest finite and its neighbour
        one, one + 1, one + 2, one + 3, one - 1,    # 1.0, 1 + ulp .. 1 + 3 ulp, 1 - ulp/2
        one - ((mant + 1) << mant),                 # 2^-(mant+1): half an ulp of 1.0 (the tie maker)
        one - ((mant + 1) << mant) + 1,             # just above the tie
        one - ((mant + 2) << mant),                 # a quarter ulp of 1.0
        one + (1 << mant), one + (1 << mant) + 1,   # 2.0 and 2 + ulp
        one + (8 << mant),                          # 256.0
        exp_all - (1 << mant),                      # 2^emax (times itself: overflow)
        one + (((exp_all >> mant) - (one >> mant)) // 2 << mant) + 3,   # about sqrt(max)
        one - (((one >> mant) - 1) // 2 << mant) - 5,                   # about sqrt(min normal)
        0x3555 if dtype == "half" else 0x3EAB,      # about 1/3
        (2 << mant) | 5,                            # a small normal
    ]
    assert len(pos) == 32, len(pos)
    table = np.array(pos + [p | 0x8000 for p in pos], dtype=np.uint16)
    assert len(set(table.tolist())) == 64
    return table


def exponent_near(dtype, rng, partner, width=3):
    """random patterns whose exponent field is within `width` of the partner's"""
    mant = 10 if dtype == "half" else 7
    emax = (0x7FFF >> mant)
    e = ((partner.astype(np.int64) & 0x7FFF) >> mant) + rng.integers(-width, width + 1, partner.size)
    e = np.clip(e, 0, emax)
    rest = rng.integers(0, 1 << mant, partner.size) | (rng.integers(0, 2, partner.size) << 15)
    return ((e << mant) | rest).astype(np.uint16)


def exhaustive_pairs(dtype):
    """every 16-bit pattern with 64 partners each, half of them near in exponent: 4.2 M pairs"""
    rng = np.random.default_rng(1234)
    a = np.repeat(np.arange(1 << 16, dtype=np.uint16), 64)
    b = rng.integers(0, 1 << 16, a.size, dtype=np.uint16)
    near = exponent_near(dtype, rng, a)
    b[1::2] = near[1::2]
    return a, b


def product_pairs(dtype):
    """every 16-bit pattern with 64 partners each, aimed at the product's
    edges: partner i's exponent field puts the product's at one of four
    targets (around 1.0, the smallest normal, half the smallest subnormal, the
    last finite binade) plus a jitter in [-2, 2]; mantissa and sign random"""
    mant, bias, emax_field = (10, 15, 31) if dtype == "half" else (7, 127, 255)
    rng = np.random.default_rng(4321)
    a = np.repeat(np.arange(1 << 16, dtype=np.uint16), 64)
    target = np.array([bias, 1, -mant, emax_field - 1], dtype=np.int64)[np.arange(a.size) % 4]
    target += rng.integers(-2, 3, a.size)
    ea = (a.astype(np.int64) & 0x7FFF) >> mant
    eb = np.clip(target + bias - np.maximum(ea, 1), 0, emax_field - 1)
    rest = rng.integers(0, 1 << mant, a.size) | (rng.integers(0, 2, a.size) << 15)
    return a, ((eb << mant) | rest).astype(np.uint16)


PAIR_SETS = {"exhaustive": exhaustive_pairs, "product": product_pairs}


@functools.lru_cache(maxsize=None)
def pair_set(name, dtype):
    """(a, b) of PAIR_SETS[name], generated once per process and read-only"""
    a, b = PAIR_SETS[name](dtype)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def third_operand(dtype, a, b, seed=0):
    """a third array for three-step chains on the pairs (a, b): seeded random
    bit patterns, every second element with an exponent field within 3 of that
    of step("sum", a, b) (so the second sum rounds, cancels or overflows), every
    64th element a NaN or an infinity of the special table"""
    rng = np.random.default_rng(8642 + seed)
    s = step("sum", dtype, a, b)
    c = rng.integers(0, 1 << 16, s.size, dtype=np.uint16)
    near = exponent_near(dtype, rng, s)
    c[1::2] = near[1::2]
    t = special_table(dtype)
    inf = 0x7FFF & ~((1 << (10 if dtype == "half" else 7)) - 1)
    nonfinite = t[(t & 0x7FFF) >= inf]
    c[::64] = nonfinite[rng.integers(0, nonfinite.size, c[::64].size)]
    return c


def sources(dtype, nsrc, n, seed):
    """nsrc arrays of n bit patterns. The first 4096 elements (where n allows)
    meet every ordered pair of the special table in sources 0 and 1 (the other
    sources walk the table at other strides); the rest are seeded random bit
    patterns, every second element of each source with an exponent near that
    of source 0's element."""
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 1 << 16, n, dtype=np.uint16) for _ in range(nsrc)]
    for k in range(1, nsrc):
        near = exponent_near(dtype, rng, out[0])
        out[k][1::2] = near[1::2]
    t = special_table(dtype)
    m = min(n, 4096)
    i = np.arange(m)
    for k in range(nsrc):
        if k == 0:
            idx = i // 64
        elif k == 1:
            idx = i % 64
        else:
            idx = (i * (2 * k + 1) + i // 64 + k) % 64
        out[k][:m] = t[idx]
    return out
