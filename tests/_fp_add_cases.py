"""Operand pairs for one IEEE-754 add, and an exact model of it (host-only).

The arithmetic of shmemx_float_atomic_add_v / shmemx_double_atomic_add_v --
global_atomic_add_f32 / _f64 in the memory-side atomic unit on the device
heap, an SSE add inside a compare-and-swap loop on the host heap -- is held
to model(): ONE correctly rounded add, nearest-even, gradual underflow,
overflow to Inf, IEEE zero signs. The same bits in either heap.

  cases(dtype)        (t, s): target and source operands, equal-length arrays
                      of float32 / float64 ("float" / "double"); seeded, fixed
  labels(dtype)       the class of every row, for failure messages
  model(t, s, dtype)  (bits, is_nan): the sum's bit patterns as uint32 /
                      uint64, and the rows whose result is a NaN. On those the
                      contract is "a NaN", nothing more: sign, payload and
                      quiet bit are unspecified and `bits` holds a placeholder
  mismatches(...)     the comparison every user of the table makes: every bit
                      on non-NaN rows, NaN-ness on NaN rows; a message that
                      names class, row, operands and got / want in hex
  WRONG_ADDERS        roundings the table must tell from model(): the same
                      exact machinery with one rule changed
                      (tests/test_fp_add_cases.py asserts that each differs)

The exact sum is an integer: every finite value of a format is a multiple of
its smallest subnormal, so t + s is an integer count of those, rounded once.
Every class appears in both operand orders: the target is the memory operand
and the source the data operand of the atomic.
"""
import functools

import numpy as np


class Fmt:
    def __init__(self, name, p, ebits, np_float, np_uint):
        self.name, self.p, self.ebits, self.np_float, self.np_uint = name, p, ebits, np_float, np_uint
        self.width = 1 + ebits + p - 1
        self.bias = (1 << (ebits - 1)) - 1
        self.emax = self.bias                       # largest binade: 2^emax <= max < 2^(emax + 1)
        self.emin = 1 - self.bias                   # smallest normal 2^emin
        self.qmin = self.emin - (p - 1)             # smallest subnormal 2^qmin
        self.sign_bit = 1 << (self.width - 1)
        self.inf = ((1 << ebits) - 1) << (p - 1)    # magnitude bits of Inf; above it: NaNs
        self.max = self.inf - 1                     # magnitude bits of the largest finite value
        self.min_normal = 1 << (p - 1)              # magnitude bits of 2^emin
        self.qnan = self.inf | (1 << (p - 2))

    def units(self, mag):
        """a finite magnitude's value in units of the smallest subnormal"""
        e, frac = mag >> (self.p - 1), mag & ((1 << (self.p - 1)) - 1)
        return frac if e == 0 else (frac | (1 << (self.p - 1))) << (e - 1)

    def enc(self, m, e, sign=0):
        """bits of (-1)^sign * m * 2^e, which must be exactly representable"""
        if m < 0:
            m, sign = -m, 1 - sign
        k = e - self.qmin
        assert k >= 0 or m % (1 << -k) == 0, (m, e)
        n = m << k if k >= 0 else m >> -k
        shift = max(0, n.bit_length() - self.p)
        assert n & ((1 << shift) - 1) == 0, ("not representable", self.name, m, e)
        mag = (shift << (self.p - 1)) + (n >> shift)
        assert mag < self.inf, ("overflows", self.name, m, e)
        return mag | (self.sign_bit if sign else 0)


FORMATS = {"float": Fmt("float", 24, 8, np.float32, np.uint32), "double": Fmt("double", 53, 11, np.float64, np.uint64)}


# ---------------------------------------------------------------------------
# the model, and the wrong adders made from it
# ---------------------------------------------------------------------------
def _round(F, neg, n, rule):
    """magnitude bits of the nonzero exact value (-1)^neg * n * 2^qmin rounded to the format"""
    shift = max(0, n.bit_length() - F.p)
    q, rem = n >> shift, n & ((1 << shift) - 1)
    half = (1 << shift) >> 1
    if rule == "toward_zero":
        up = 0
    elif rule == "half_away":
        up = rem != 0 and rem >= half
    elif rule == "toward_neg_inf":
        up = rem != 0 and neg
    else:                                           # nearest, ties to even
        up = rem > half or (rem == half and rem != 0 and (q & 1))
    mag = (shift << (F.p - 1)) + q + int(up)        # a carry out of the mantissa runs into the exponent field
    if mag >= F.inf:
        to_max = rule in ("toward_zero", "saturate") or (rule == "toward_neg_inf" and not neg)
        mag = F.max if to_max else F.inf
    if rule == "flush_results" and mag < F.min_normal:
        mag = 0
    return mag


def _add_bits(F, a, b, rule):
    """bits of a + b under `rule`, or None where the result is a NaN"""
    sa, sb = a >> (F.width - 1), b >> (F.width - 1)
    ma, mb = a & (F.sign_bit - 1), b & (F.sign_bit - 1)
    if ma > F.inf or mb > F.inf:
        return None
    if ma == F.inf or mb == F.inf:
        if ma == mb and sa != sb:
            return None                             # Inf + -Inf: invalid
        return a if ma == F.inf else b
    if rule == "flush_inputs":
        ma, mb = (0 if ma < F.min_normal else ma), (0 if mb < F.min_normal else mb)
    if ma == 0 and mb == 0:
        neg = (sa | sb) if rule == "toward_neg_inf" else (sa & sb)
        return F.sign_bit if neg else 0
    n = (-F.units(ma) if sa else F.units(ma)) + (-F.units(mb) if sb else F.units(mb))
    if n == 0:                                      # exact cancellation: +0, but -0 when rounding down
        return F.sign_bit if rule == "toward_neg_inf" else 0
    return _round(F, n < 0, abs(n), rule) | (F.sign_bit if n < 0 else 0)


def _add_arrays(t, s, dtype, rule):
    F = FORMATS[dtype]
    tb = np.ascontiguousarray(t).view(F.np_uint).tolist()
    sb = np.ascontiguousarray(s).view(F.np_uint).tolist()
    out = [_add_bits(F, a, b, rule) for a, b in zip(tb, sb)]
    nan = np.array([o is None for o in out], bool)
    return np.array([F.qnan if o is None else o for o in out], F.np_uint), nan


def model(t, s, dtype):
    """(bits, is_nan) of t + s, element-wise: one correctly rounded IEEE add"""
    return _add_arrays(t, s, dtype, "nearest_even")


WRONG_ADDERS = {
    "subnormal inputs flushed to zero": "flush_inputs",
    "subnormal results flushed to zero": "flush_results",
    "round toward zero": "toward_zero",
    "round half away from zero": "half_away",
    "round toward -Inf": "toward_neg_inf",
    "saturation to max instead of Inf": "saturate",
}


def wrong_adder(t, s, dtype, name):
    return _add_arrays(t, s, dtype, WRONG_ADDERS[name])


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
def _build(dtype):
    F = FORMATS[dtype]
    p, emin, emax, qmin = F.p, F.emin, F.emax, F.qmin
    rng = np.random.default_rng({"float": 2401, "double": 5301}[dtype])
    rows = []                                       # (label, target bits, source bits)

    def both(label, a, b):
        rows.append((label, a, b))
        rows.append((label, b, a))

    def mant():
        """a full-mantissa significand in [2^(p-1), 2^p)"""
        return (1 << (p - 1)) | int(rng.integers(0, 1 << (p - 1)))

    top = 1 << (p - 1)
    neg = F.sign_bit
    MAX, MINN, MINSUB = F.max, F.min_normal, 1

    # -- ties and sticky bits: t = (2^(p-1) + m) 2^e, in the binade of 2^E, has ulp 2^e
    for E in {"float": (-100, -60, -1, 0, 1, 30, 100), "double": (-900, -300, -1, 0, 1, 300, 1000)}[dtype]:
        e = E - (p - 1)
        for m in (0, 1, 2, 3, top - 2, top - 1):
            for st in (0, 1):
                t = F.enc(top + m, e, st)
                for ss in (0, 1):
                    both("tie", t, F.enc(1, e - 1, ss))
                    for k in (p - 2, 10):           # half an ulp +- a far smaller power of two
                        both("just above a tie", t, F.enc((1 << k) + 1, e - 1 - k, ss))
                        both("just below a tie", t, F.enc((1 << k) - 1, e - 1 - k, ss))
    # -- the binade boundary: below t = 2^k the ulp halves
    for k in {"float": (-100, -1, 0, 1, 24, 100), "double": (-900, -1, 0, 1, 53, 900)}[dtype]:
        u = k - (p - 1)                             # ulp(2^k) = 2^u
        for st in (0, 1):
            t = F.enc(1, k, st)
            both("binade boundary", t, F.enc(1, u - 2, 1 - st))       # a tie between t - ulp/2 and t
            both("binade boundary", t, F.enc(1, u - 1, 1 - st))       # exact: t - ulp/2
            both("binade boundary", t, F.enc(9, u - 5, 1 - st))       # ulp/4 + ulp/32
            both("binade boundary", t, F.enc(7, u - 5, 1 - st))       # ulp/4 - ulp/32
            both("binade boundary", t, F.enc(3, u - 2, 1 - st))       # a tie between t - ulp and t - ulp/2

    # -- random full-mantissa pairs at every exponent difference (negative and
    #    positive differences are the two operand orders)
    span = {"float": 40, "double": 400}[dtype]
    for d in range(-(p + 3), p + 4):
        for i in range(64):
            et = int(rng.integers(-span, span + 1))
            st, ss = i & 1, (i >> 1) & 1
            rows.append((f"random pair, exponents differ by {d}", F.enc(mant(), et - (p - 1), st),
                         F.enc(mant(), et + d - (p - 1), ss)))
    # sums that carry out of the top binade's neighbour, and differences that
    # renormalise by many bits: equal exponents, all sign pairs
    for i in range(128):
        et = int(rng.integers(-span, span + 1))
        rows.append(("random pair, equal exponents", F.enc(mant(), et, i & 1), F.enc(mant(), et, (i >> 1) & 1)))

    # -- cancellation
    specials = [MAX, MINN, MINSUB, MINN - 1, F.enc(1, 0), F.enc(3, -1)]
    for x in specials + [F.enc(mant(), int(rng.integers(-span, span))) for _ in range(32)] + \
            [int(rng.integers(1, MINN)) for _ in range(8)]:
        both("x + (-x)", x, x | neg)
    for _ in range(32):
        x = F.enc(mant(), int(rng.integers(-span, span)))
        both("cancellation to one ulp", x, (x + 1) | neg)
        both("cancellation to one ulp", x | neg, x - 1)
    for j in range(1, p - 1):                       # both operands normal, the difference subnormal and exact
        x = F.enc(mant() | 1, emin + j - (p - 1))
        k = int(rng.integers(1, 1 << (p - 1 - j)))  # the difference, k 2^(qmin + j) < 2^emin
        y = F.units(x) + (k << j) if F.units(x) + (k << j) < (top << (j + 1)) else F.units(x) - (k << j)
        both("cancellation into the subnormals", x, F.enc(y, qmin, 1))
        both("cancellation into the subnormals", x | neg, F.enc(y, qmin))
    both("cancellation into the subnormals", F.enc(1, emin + 1), F.enc((top << 1) - 1, qmin, 1))

    # -- gradual underflow
    for i in range(64):
        a, b = int(rng.integers(1, MINN)), int(rng.integers(1, MINN))
        both("subnormal + subnormal", a | (neg if i & 1 else 0), b | (neg if i & 2 else 0))
    for k in (1, 2, 3, top >> 1, top - 1):
        both("subnormals that sum to the smallest normal", top - k, k)
        both("subnormals that sum to the smallest normal", (top - k) | neg, k | neg)
    for sg in (0, neg):
        both("smallest normal - smallest subnormal", MINN | sg, MINSUB | (neg ^ sg))
        both("smallest subnormal + smallest subnormal", MINSUB | sg, MINSUB | sg)
        both("smallest subnormal + smallest subnormal", MINSUB | sg, MINSUB | (neg ^ sg))
        for z in (0, neg):
            both("subnormal + 0", MINSUB | sg, z)
            both("subnormal + 0", (MINN - 1) | sg, z)
            both("subnormal + 0", int(rng.integers(2, MINN - 1)) | sg, z)
    for j in range(1, p - 1):                       # t's ulp is 2^(qmin + j): a subnormal s decides the rounding
        for m in (0, 1, top - 1):
            for st in (0, neg):
                t = F.enc(top + m, qmin + j) | st
                for ss in (0, neg):
                    both("normal + subnormal, a tie", t, (1 << (j - 1)) | ss)
                    if j >= 2:
                        both("normal + subnormal, just above a tie", t, ((1 << (j - 1)) + 1) | ss)
                        both("normal + subnormal, just below a tie", t, ((1 << (j - 1)) - 1) | ss)

    # -- overflow: ulp(max) = 2^(emax - p + 1)
    for sg in (0, neg):
        both("max + half an ulp: a tie, to Inf", MAX | sg, F.enc(1, emax - p) | sg)
        both("max + a quarter ulp: stays max", MAX | sg, F.enc(1, emax - p - 1) | sg)
        both("max + just below half an ulp: stays max", MAX | sg, F.enc((1 << 10) - 1, emax - p - 10) | sg)
        both("max + just above half an ulp: to Inf", MAX | sg, F.enc((1 << 10) + 1, emax - p - 10) | sg)
        both("max + max", MAX | sg, MAX | sg)
        both("max + one ulp: to Inf", MAX | sg, F.enc(1, emax - p + 1) | sg)
        both("below max + one ulp: max", (MAX - 1) | sg, F.enc(1, emax - p + 1) | sg)
        both("2^emax + 2^emax", F.enc(1, emax) | sg, F.enc(1, emax) | sg)
        both("max - half an ulp: a tie, to the even neighbour below", MAX | sg, F.enc(1, emax - p) | (neg ^ sg))

    # -- zeros
    for a in (0, neg):
        for b in (0, neg):
            rows.append(("zeros", a, b))

    # -- infinities
    finite = [F.enc(1, 0), F.enc(mant(), 3 - (p - 1)), MAX, MINN, MINSUB, MINN - 1]
    for si in (0, neg):
        for x in finite:
            for sx in (0, neg):
                both("Inf + finite", F.inf | si, x | sx)
        for z in (0, neg):
            both("Inf + 0", F.inf | si, z)
        for sj in (0, neg):
            rows.append(("Inf + Inf" if si == sj else "Inf + -Inf", F.inf | si, F.inf | sj))

    # -- NaNs: quiet and signalling, both signs, several payloads; as target,
    #    as source and as both, against a member of every other class
    quiet = 1 << (p - 2)
    payloads = (1, 0x2A, quiet - 1, (quiet >> 1) | 5)
    nans = [F.inf | q | pay | sg for q in (quiet, 0) for pay in payloads for sg in (0, neg)] + [F.inf | quiet,
                                                                                               F.inf | quiet | neg]
    others = [F.enc(top + 1, 0), F.enc(1, -1), F.enc(mant(), -7, 1), F.enc(1, emin + 2), MINSUB, (MINN - 1) | neg,
              MINN, MAX, MAX | neg, F.enc(1, emax - p), 0, neg, F.inf, F.inf | neg]
    for x in nans:
        for y in others:
            both("NaN + non-NaN", x, y)
        for y in nans:
            rows.append(("NaN + NaN", x, y))

    lab = [r[0] for r in rows]
    t = np.array([r[1] for r in rows], F.np_uint).view(F.np_float)
    s = np.array([r[2] for r in rows], F.np_uint).view(F.np_float)
    t.flags.writeable = s.flags.writeable = False
    return t, s, lab


@functools.lru_cache(maxsize=None)
def _table(dtype):
    t, s, lab = _build(dtype)
    bits, nan = model(t, s, dtype)
    bits.flags.writeable = nan.flags.writeable = False
    return t, s, lab, bits, nan


def cases(dtype):
    """(t, s) for "float" or "double": read-only arrays, the same on every call"""
    return _table(dtype)[:2]


def labels(dtype):
    return _table(dtype)[2]


def expected(dtype):
    """model() of the table, computed once per process: (bits, is_nan)"""
    return _table(dtype)[3:]


def mismatches(dtype, got, order=None, where=""):
    """None, or a message: `got` (floats or bit patterns, one per row) against
    the model of the table; `order` is the row each element of `got` came
    from, where the table was run permuted."""
    F = FORMATS[dtype]
    t, s, lab, want, nan = _table(dtype)
    order = np.arange(t.size) if order is None else np.asarray(order)
    got = np.ascontiguousarray(got).view(F.np_uint)
    assert got.shape == order.shape == want.shape, (got.shape, order.shape, want.shape)
    want, nan = want[order], nan[order]
    got_nan = (got & F.np_uint(F.sign_bit - 1)) > F.np_uint(F.inf)
    bad = np.nonzero(np.where(nan, ~got_nan, got != want))[0]
    if bad.size == 0:
        return None
    tb, sb = t.view(F.np_uint)[order], s.view(F.np_uint)[order]
    h = lambda v: f"{int(v):#0{F.width // 4 + 2}x}"  # noqa: E731
    lines = [f"{dtype} {where}: {bad.size} of {got.size} rows differ from one correctly rounded add;"
             f" classes: {sorted({lab[order[i]] for i in bad})[:12]}"]
    for i in bad[:8]:
        lines.append(f"  [{lab[order[i]]}] row {int(order[i])} (element {int(i)}): t {h(tb[i])} + s {h(sb[i])}: "
                     f"got {h(got[i])}, want {'a NaN' if nan[i] else h(want[i])}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------
# several adders at once: every legal result of an element
# ---------------------------------------------------------------------------
ORDERS_N = 4096 + 64        # one wave-instruction's worth past 4,096 elements
# the share of elements that must have two or more distinct legal results, by
# PE count: the seeds below give 27.7 % (2 PEs, float and double) and 82.7 % /
# 82.5 % (4 PEs, float / double); tests/test_fp_add_cases.py asserts it of the inputs
ORDERS_MIN_SHARE = {2: 0.25, 4: 0.75}


@functools.lru_cache(maxsize=None)
def orders_case(dtype, npes):
    """(init, sources, legal, share) for `npes` PEs adding into one target at
    once: init and sources[pe] are ORDERS_N full-mantissa values of magnitude
    in [1, 256) and random sign (within 2^8 of each other and of every partial
    sum's ulp: no term can be absorbed, so a lost or a doubled update equals
    no legal result); legal[k] holds the bits of the sum taken in the k-th of
    the npes! arrival orders, each add rounded in the format, on top of init;
    share is the fraction of elements with two or more distinct legal results.
    Seeded: the same on every PE and in every process."""
    import itertools
    F = FORMATS[dtype]
    rng = np.random.default_rng(7700 + F.p + npes)

    def draw():
        m = rng.integers(0, 1 << (F.p - 1), ORDERS_N, dtype=np.int64) + (1 << (F.p - 1))
        v = np.ldexp(m.astype(np.float64), rng.integers(0, 8, ORDERS_N) - (F.p - 1))
        assert ((v >= 1) & (v < 256)).all()
        out = (v * rng.choice([-1.0, 1.0], ORDERS_N)).astype(F.np_float)
        assert (out.astype(np.float64) == np.abs(v) * np.sign(out)).all()      # exact in the format
        out.flags.writeable = False
        return out

    init = draw()
    sources = [draw() for _ in range(npes)]
    legal = []
    for perm in itertools.permutations(range(npes)):
        acc = init.copy()
        for pe in perm:
            acc = (acc + sources[pe]).astype(F.np_float)
        legal.append(acc.view(F.np_uint))
    legal = np.stack(legal)
    share = float((legal != legal[0]).any(axis=0).mean())
    return init, sources, legal, share


def illegal_elements(dtype, npes, got):
    """indices of the elements of `got` that equal the sum in no arrival order"""
    F = FORMATS[dtype]
    legal = orders_case(dtype, npes)[2]
    return np.nonzero(~(np.ascontiguousarray(got).view(F.np_uint)[None, :] == legal).any(axis=0))[0]
