"""Which branch of the element operators an operand pair takes (host-only).

The kernels promise the reference's bits through a few dozen hand-written
branches of osss-gasnet_amd/csrc/ops.h (x86_result, cmul, cplx_op, the min/max
selects, the 16-bit floats' canonical NaN). This file names them:

  CATALOGUE[(op, dtype)]        the branch names of a pair
  paths(op, dtype, acc, src)    per element, the name of the branch that
                                apply<OP>(acc, src) takes (acc on the left, as
                                in the reference's fold)
  table(op, dtype)              (acc, src): a directed operand table that
                                reaches every catalogue entry, in both operand
                                orders where the order can matter
  WRONG_OPERATORS               one-rule mutations of model(), which the table
                                must tell from the reference
  rule_violations(...)          what a branch name says about the result's
                                bits, checked against a result (the oracle's)

The classifier restates the DECISIONS of ops.h, not its arithmetic: where a
decision hangs on a computed value (a partial product that overflowed, a sum
that came out subnormal) that value is numpy's own arithmetic in the type.
The arbiter of every result is the compiled reference operator
(oracle.reduce_pe; tests/_half_ref.py for the 16-bit floats, which the
reference lacks); the classifier only names the case.

Elements are numpy arrays of oracle.NP[dtype]; the 16-bit floats are uint16
bit patterns, long double the 16-byte x87 slots.

The layouts at the end place a table in arrays the way the streaming kernels
cut them into waves (one 16-byte vector per lane, 64 lanes per wave): see
wave_layout() and spaced_layout().
"""
import functools

import numpy as np

import _half_ref
import oracle

INTS = ("short", "int", "long", "longlong")
HALF = _half_ref.TYPES
PAIRS = list(oracle.PAIRS) + [(op, t) for t in HALF for op in _half_ref.OPS]
NP = dict(oracle.NP, half=np.uint16, bfloat16=np.uint16)
ES = {t: np.dtype(NP[t]).itemsize for t in NP}


class Bits:
    """the fields of binary32 / binary64"""

    def __init__(self, f, u, mbits):
        bits = np.dtype(u).itemsize * 8
        self.f, self.u = f, u
        self.sign = u(1 << (bits - 1))
        self.quiet = u(1 << (mbits - 1))
        self.exp = u(((1 << (bits - 1 - mbits)) - 1) << mbits)
        self.indefinite = u(self.sign | self.exp | self.quiet)      # SSE's invalid-operation NaN
        self.default_nan = u(self.exp | self.quiet)                 # the GPU's own: sign clear

    def nan(self, payload, negative=False, quiet=True):
        v = int(self.exp) | int(payload) | (int(self.quiet) if quiet else 0) | (int(self.sign) if negative else 0)
        return np.array([v], self.u).view(self.f)[0]


FMT = {"float": Bits(np.float32, np.uint32, 23), "double": Bits(np.float64, np.uint64, 52)}
FMT["complexf"], FMT["complexd"] = FMT["float"], FMT["double"]


def _c(x):
    return np.ascontiguousarray(x)


def _bits(F, x):
    return _c(x).view(F.u)


def _names(codes, names):
    return np.array(names, dtype=object)[codes]


# ---------------------------------------------------------------------------
# float, double: x86_result's four outcomes; the selects of min/max
# ---------------------------------------------------------------------------
NUMBER, ACC_NAN, SRC_NAN, INDEFINITE, BOTH_NAN = 0, 1, 2, 3, 4
PART = {NUMBER: "a number", ACC_NAN: "the accumulator's NaN, quieted", SRC_NAN: "the incoming NaN, quieted",
        BOTH_NAN: "both NaN, payloads differ"}
INVALID = {"sum": "the indefinite of Inf - Inf", "prod": "the indefinite of 0 x Inf"}


def _part_names(op, both=False):
    return [PART[NUMBER], PART[ACC_NAN], PART[SRC_NAN], INVALID[op]] + ([PART[BOTH_NAN]] if both else [])


def _real_codes(op, a, b, first_is_src=False, split_both=False, F=None):
    """x86_result(a op b, a, b): which operand's NaN, or the invalid operation.
    first_is_src: the operation is b op a (float complex's imaginary add)."""
    na, nb = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        if op == "sum":
            invalid = np.isinf(a) & np.isinf(b) & (np.signbit(a) != np.signbit(b))
        else:
            invalid = (np.isinf(a) & (b == 0)) | ((a == 0) & np.isinf(b))
    first, second = (nb, na) if first_is_src else (na, nb)
    code = np.where(first, SRC_NAN if first_is_src else ACC_NAN,
                    np.where(second, ACC_NAN if first_is_src else SRC_NAN, np.where(invalid, INDEFINITE, NUMBER)))
    if split_both:
        code = np.where(na & nb & (_bits(F, a) != _bits(F, b)), BOTH_NAN, code)
    return code


MM = ["the first operand (ordered)", "the second operand (ordered)", "the second: unordered by the first operand",
      "the second: unordered by the second operand", "the second: +0 then -0", "the second: -0 then +0"]


def _minmax_codes(op, a, b):
    with np.errstate(invalid="ignore"):
        zeros = (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))
        first = a < b if op == "min" else a > b
    return np.where(np.isnan(a), 2, np.where(np.isnan(b), 3, np.where(zeros, np.where(np.signbit(a), 5, 4),
                                                                      np.where(first, 0, 1))))


# ---------------------------------------------------------------------------
# complex product: libgcc's __mulsc3 / __muldc3 (ops.h cmul)
# ---------------------------------------------------------------------------
CP_PLAIN, CP_ONE, CP_BOTH = "no NaN part", "one NaN part: no recovery", "both parts NaN, no recovery condition"
CP_REC = ["recovery by the first operand's infinity", "recovery by the second operand's infinity",
          "recovery by both operands' infinities", "recovery by an overflowed partial product"]
CP_SUB = ["infinite parts", "a part made the indefinite"]
CP_NAMES = [CP_PLAIN, CP_ONE, CP_BOTH] + [f"{r}: {s}" for r in CP_REC for s in CP_SUB]


def _x86(F, r, a, b, mut=()):
    """SSE's a op b from the plain result r: the first NaN operand quieted, else the indefinite"""
    ua, ub = _bits(F, a) | F.quiet, _bits(F, b) | F.quiet
    indef = F.default_nan if "indefinite with its sign clear" in mut else F.indefinite
    if "the second NaN taken before the first" in mut:
        pick = np.where(np.isnan(b), ub, np.where(np.isnan(a), ua, indef))
    else:
        pick = np.where(np.isnan(a), ua, np.where(np.isnan(b), ub, indef))
    return np.where(np.isnan(r), pick.astype(F.u).view(F.f), r)


def _cmul(F, a, b, c, d, mut=()):
    """(x, y, path codes into CP_NAMES) of (a + ib)(c + id)"""
    f = F.f
    a, b, c, d = (_c(v).astype(f) for v in (a, b, c, d))
    one, zero, inf = f(1), f(0), f(np.inf)
    with np.errstate(all="ignore"):
        ac, bd = _x86(F, a * c, a, c, mut), _x86(F, b * d, b, d, mut)
        ad, bc = _x86(F, a * d, a, d, mut), _x86(F, c * b, c, b, mut)
        x, y = _x86(F, ac - bd, ac, bd, mut), _x86(F, ad + bc, ad, bc, mut)
        nx, ny = np.isnan(x), np.isnan(y)
        both = nx & ny
        r1 = both & (np.isinf(a) | np.isinf(b))
        r2 = both & (np.isinf(c) | np.isinf(d))
        r3 = both & ~r1 & ~r2 & (np.isinf(ac) | np.isinf(bd) | np.isinf(ad) | np.isinf(bc))
        if "cmul without its third recovery condition" in mut:
            r3 = r3 & False
        keep_nan = "cmul without the copysign(0, .) replacement of NaN operands" in mut

        def box(v, on):
            return np.where(on, np.copysign(np.where(np.isinf(v), one, zero), v), v)

        def unnan(v, on):
            return v if keep_nan else np.where(on & np.isnan(v), np.copysign(zero, v), v)

        A, B, C, D = box(a, r1), box(b, r1), unnan(c, r1), unnan(d, r1)
        C, D, A, B = box(C, r2), box(D, r2), unnan(A, r2), unnan(B, r2)
        A, B, C, D = unnan(A, r3), unnan(B, r3), unnan(C, r3), unnan(D, r3)
        rx, ry = inf * (A * C - B * D), inf * (A * D + B * C)
        rec = r1 | r2 | r3
        made = rec & (np.isnan(rx) | np.isnan(ry))
        left = F.default_nan if "cmul's recomputation left NaN" in mut else F.indefinite
        fill = np.full(a.shape, left, F.u).view(f)
        x = np.where(rec, np.where(np.isnan(rx), fill, rx), x)
        y = np.where(rec, np.where(np.isnan(ry), fill, ry), y)
    which = np.where(r1 & r2, 2, np.where(r1, 0, np.where(r2, 1, 3)))
    code = np.where(rec, 3 + 2 * which + made, np.where(both, 2, np.where(nx | ny, 1, 0)))
    return x, y, code


# ---------------------------------------------------------------------------
# integers
# ---------------------------------------------------------------------------
def _int_names(op, dtype):
    if op in ("sum", "prod"):
        return ["fits", "truncated after promotion to int" if dtype == "short" else "wraps"]
    if op in ("min", "max"):
        return ["the first operand", "the second operand", "a tie: the second operand"]
    return ["bitwise"]


def _exact(op, a, b):
    a, b = a.astype(object), b.astype(object)
    return a + b if op == "sum" else a * b


def _int_codes(op, dtype, a, b):
    if op in ("sum", "prod"):
        info = np.iinfo(NP[dtype])
        r = _exact(op, a, b)
        return ((r < info.min) | (r > info.max)).astype(int)
    if op in ("min", "max"):
        return np.where(a == b, 2, np.where(a < b if op == "min" else a > b, 0, 1))
    return np.zeros(len(a), int)


# ---------------------------------------------------------------------------
# half, bfloat16 (tests/_half_ref.py is their definition)
# ---------------------------------------------------------------------------
H_NAMES = ["a number", "a NaN operand, not the canonical one", "the canonical NaN as an operand",
           "an invalid operation", "overflow to Inf", "a subnormal result"]


def _half_inf(dtype):
    return 0x7C00 if dtype == "half" else 0x7F80


def _half_codes(op, dtype, a, b):
    a, b = _c(a).astype(np.uint16), _c(b).astype(np.uint16)
    inf, canon = _half_inf(dtype), _half_ref.CANONICAL_NAN[dtype]
    na, nb = (a & 0x7FFF) > inf, (b & 0x7FFF) > inf
    if op in ("min", "max"):
        return _minmax_codes(op, _half_ref.widen(dtype, a), _half_ref.widen(dtype, b))
    r = _half_ref.step(op, dtype, a, b)
    mag = r & 0x7FFF
    odd = (na & (a != canon)) | (nb & (b != canon))
    finite_in = ((a & 0x7FFF) < inf) & ((b & 0x7FFF) < inf)
    return np.where(odd, 1, np.where(na | nb, 2, np.where(mag > inf, 3, np.where(finite_in & (mag == inf), 4, np.where(
        (mag < (inf & -inf)) & (mag != 0), 5, 0)))))


# ---------------------------------------------------------------------------
# long double: the operands' classes (the arithmetic is x80.h's, checked by
# tests/native/x80_host_check.cpp and the x87 GPU tests)
# ---------------------------------------------------------------------------
X_CLASSES = ["zero", "denormal", "pseudo-denormal", "normal", "infinity", "quiet NaN", "signalling NaN",
             "unsupported encoding"]
X_RESULTS = ["normal", "denormal", "overflow", "NaN", "indefinite"]


def x87(sign, efield, mant):
    """one long double from its fields"""
    b = np.zeros(16, dtype=np.uint8)
    b[:8] = np.frombuffer(np.uint64(mant).tobytes(), dtype=np.uint8)
    b[8:10] = np.frombuffer(np.uint16((sign << 15) | efield).tobytes(), dtype=np.uint8)
    return b.view(np.longdouble)[0]


def _x_fields(v):
    raw = _c(v).view(np.uint8).reshape(-1, 16)
    m = raw[:, 0:8].copy().view(np.uint64).reshape(-1)
    se = raw[:, 8:10].copy().view(np.uint16).reshape(-1)
    return m, se


def _x_class(v):
    m, se = _x_fields(v)
    e = se & 0x7FFF
    top, second = (m >> np.uint64(63)) != 0, ((m >> np.uint64(62)) & np.uint64(1)) != 0
    low = e == 0
    high = e == 0x7FFF
    return np.where(low, np.where(m == 0, 0, np.where(top, 2, 1)),
                    np.where(high, np.where(~top, 7, np.where(m == np.uint64(1 << 63), 4, np.where(second, 5, 6))),
                             np.where(top, 3, 7)))


def _x_result_class(r):
    """X_RESULTS index of a result, -1 for a zero or an infinity from an infinity"""
    m, se = _x_fields(r)
    cls = _x_class(r)
    indefinite = (se == 0xFFFF) & (m == np.uint64(3 << 62))
    return np.where(indefinite, 4, np.where((cls == 5) | (cls == 6), 3, np.where(cls == 4, 2, np.where(
        (cls == 1) | (cls == 2), 1, np.where(cls == 3, 0, -1)))))


def _x_names(op):
    names = [f"{a}, {b}" for a in X_CLASSES for b in X_CLASSES]
    if op == "prod":       # 0 x Inf is always invalid
        names = [s for s in names if s not in ("zero, infinity", "infinity, zero")]
    if op in ("sum", "prod"):
        names += [f"normal, normal: {r} result" for r in ("denormal", "overflow")]
        names += ["infinity, infinity: indefinite"] if op == "sum" else ["zero, infinity: indefinite",
                                                                          "infinity, zero: indefinite"]
    return names


def _x_paths(op, a, b):
    ca, cb = _x_class(a), _x_class(b)
    out = np.array([f"{X_CLASSES[i]}, {X_CLASSES[j]}" for i, j in zip(ca, cb)], dtype=object)
    if op in ("sum", "prod"):
        with np.errstate(all="ignore"):
            r = _x_result_class(_c(a) + _c(b) if op == "sum" else _c(a) * _c(b))
        both_normal = (ca == 3) & (cb == 3)
        out[both_normal & (r == 1)] = "normal, normal: denormal result"
        out[both_normal & (r == 2)] = "normal, normal: overflow result"
        clean = (ca < 5) & (cb < 5) & (r == 4)      # no NaN, no unsupported operand: the operation was invalid
        for i in np.nonzero(clean)[0]:
            out[i] += ": indefinite"
    return out


# ---------------------------------------------------------------------------
# the catalogue and the classifier
# ---------------------------------------------------------------------------
def _catalogue(op, dtype):
    if dtype in INTS:
        return _int_names(op, dtype)
    if dtype in HALF:
        return MM if op in ("min", "max") else H_NAMES
    if dtype == "longdouble":
        return _x_names(op)
    if dtype in ("float", "double"):
        return MM if op in ("min", "max") else _part_names(op)
    if op == "sum":
        return [f"re {r}, im {i}" for r in _part_names(op) for i in _part_names(op, both=True)]
    return CP_NAMES


CATALOGUE = {(op, t): _catalogue(op, t) for op, t in PAIRS}


def components(op, dtype, name):
    """the branches a catalogue entry stands for: a complex sum's entry names
    one x86_result outcome per part, every other entry is one branch"""
    if dtype in ("complexf", "complexd") and op == "sum":
        re, im = name.split(", im ")
        return [re, "im " + im]
    return [name]


def paths(op, dtype, acc, src):
    """per element, the name of the branch apply<OP>(acc, src) takes"""
    acc, src = _c(acc), _c(src)
    names = CATALOGUE[(op, dtype)]
    if dtype in INTS:
        return _names(_int_codes(op, dtype, acc, src), names)
    if dtype in HALF:
        return _names(_half_codes(op, dtype, acc, src), names)
    if dtype == "longdouble":
        return _x_paths(op, acc, src)
    F = FMT[dtype]
    if dtype in ("float", "double"):
        return _names(_minmax_codes(op, acc, src) if op in ("min", "max") else _real_codes(op, acc, src), names)
    if op == "sum":
        re = _real_codes(op, _c(acc.real), _c(src.real))
        im = _real_codes(op, _c(acc.imag), _c(src.imag), first_is_src=dtype == "complexf", split_both=True, F=F)
        rn, inn = _part_names(op), _part_names(op, both=True)
        return np.array([f"re {rn[r]}, im {inn[i]}" for r, i in zip(re, im)], dtype=object)
    return _names(_cmul(F, acc.real, acc.imag, src.real, src.imag)[2], names)


# ---------------------------------------------------------------------------
# the operators in numpy, for the mutations only
# ---------------------------------------------------------------------------
def model(op, dtype, acc, src, mut=()):
    """acc op src as ops.h computes it, with the rules named in `mut` broken;
    float, double, the complex types and the 16-bit floats"""
    acc, src = _c(acc), _c(src)
    if dtype in HALF:
        if op in ("min", "max"):
            return _select(op, _half_ref.widen(dtype, acc), _half_ref.widen(dtype, src), acc, src, mut)
        r = _half_ref.step(op, dtype, acc, src)
        if "the 16-bit NaN left uncanonical" in mut:      # SSE's rule instead: the first NaN operand, quieted
            inf = _half_inf(dtype)
            quiet = np.uint16((inf & -inf) >> 1)
            na, nb = (acc & 0x7FFF) > inf, (src & 0x7FFF) > inf
            r = np.where(na, acc | quiet, np.where(nb, src | quiet, r)).astype(np.uint16)
        return r
    F = FMT[dtype]
    with np.errstate(all="ignore"):
        if dtype in ("float", "double"):
            if op in ("min", "max"):
                return _select(op, acc, src, acc, src, mut)
            return _x86(F, acc + src if op == "sum" else acc * src, acc, src, mut)
        a, b, c, d = _c(acc.real), _c(acc.imag), _c(src.real), _c(src.imag)
        out = np.empty_like(acc)
        if op == "sum":
            out.real = _x86(F, a + c, a, c, mut)
            swapped = dtype == "complexf" and "complexf's imaginary add in accumulator-first order" not in mut
            out.imag = _x86(F, d + b, d, b, mut) if swapped else _x86(F, b + d, b, d, mut)
        else:
            out.real, out.imag, _ = _cmul(F, a, b, c, d, mut)
        return out


def _select(op, x, y, a, b, mut):
    with np.errstate(invalid="ignore"):
        first = x < y if op == "min" else x > y
        if "min/max returning the first operand when unordered" in mut:
            first = first | np.isnan(x) | np.isnan(y)
        if "the +-0 pair resolved by sign" in mut:      # IEEE minimum / maximum: -0 < +0
            zeros = (x == 0) & (y == 0)
            first = np.where(zeros, np.signbit(x) if op == "min" else ~np.signbit(x), first)
    return np.where(first, a, b)


_FP_ARITH = [(op, t) for op in ("sum", "prod") for t in ("float", "double", "complexf", "complexd")]
_CPROD = [("prod", "complexf"), ("prod", "complexd")]
_SELECTS = [(op, t) for op in ("min", "max") for t in ("float", "double") + HALF]
# name -> the pairs whose table must tell the mutation from the reference
WRONG_OPERATORS = {
    "the second NaN taken before the first": _FP_ARITH,
    "indefinite with its sign clear": _FP_ARITH,
    "complexf's imaginary add in accumulator-first order": [("sum", "complexf")],
    "cmul without its third recovery condition": _CPROD,
    "cmul without the copysign(0, .) replacement of NaN operands": _CPROD,
    "cmul's recomputation left NaN": _CPROD,
    "min/max returning the first operand when unordered": _SELECTS,
    "the +-0 pair resolved by sign": _SELECTS,
    "the 16-bit NaN left uncanonical": [(op, t) for op in ("sum", "prod") for t in HALF],
}


def wrong_operator(name, op, dtype, acc, src):
    assert (op, dtype) in WRONG_OPERATORS[name], (name, op, dtype)
    return model(op, dtype, acc, src, mut=(name,))


# ---------------------------------------------------------------------------
# the reference's answer, and what a branch name says about its bits
# ---------------------------------------------------------------------------
def reference(op, dtype, acc, src):
    """acc op src by the arbiter: the oracle; the model for the 16-bit floats"""
    if dtype in HALF:
        return _half_ref.step(op, dtype, acc, src)
    return oracle.reduce_pe(op, dtype, [acc, src], 0)


def same_bits(dtype, x, y):
    """per element: every value bit equal (long double: its 10 bytes)"""
    if dtype in HALF:
        return _c(x).view(np.uint16) == _c(y).view(np.uint16)
    return (oracle.as_value_bytes(x, dtype) == oracle.as_value_bytes(y, dtype)).all(axis=1)


def _part_rule(F, name, r, a, b):
    """per element: does part result r look as the part's branch `name` says"""
    rb, ab, bb = _bits(F, r), _bits(F, a), _bits(F, b)
    if name == PART[NUMBER]:
        return ~np.isnan(r)
    if name == PART[ACC_NAN]:
        return rb == (ab | F.quiet)
    if name == PART[SRC_NAN]:
        return rb == (bb | F.quiet)
    if name in INVALID.values():
        return rb == F.indefinite
    raise KeyError(name)


def rule_violations(op, dtype, acc, src, res):
    """indices where `res` does not look as paths(op, dtype, acc, src) says it
    must; with the rules' wording, for the message"""
    acc, src, res = _c(acc), _c(src), _c(res)
    p = paths(op, dtype, acc, src)
    ok = np.ones(len(p), bool)
    if dtype in INTS:
        if op in ("sum", "prod"):
            exact = _exact(op, acc, src)
            bits = 8 * ES[dtype]
            wrapped = np.array([((int(v) + (1 << (bits - 1))) % (1 << bits)) - (1 << (bits - 1)) for v in exact], object)
            ok = np.where(p == "fits", res.astype(object) == exact, (res.astype(object) == wrapped) & (wrapped != exact))
        elif op in ("min", "max"):
            ok = np.where(p == "the first operand", res == acc, res == src)
            ok &= np.where(p == "a tie: the second operand", acc == src, acc != src)
        else:
            ok = res == {"and": acc & src, "or": acc | src, "xor": acc ^ src}[op]
    elif op in ("min", "max") and dtype != "longdouble":
        ok = np.where(p == MM[0], same_bits(dtype, res, acc), same_bits(dtype, res, src))
        ok &= np.where(p == MM[0], ~same_bits(dtype, acc, src), True)      # a rule that can fail
    elif dtype in HALF:
        inf, canon = _half_inf(dtype), _half_ref.CANONICAL_NAN[dtype]
        mag = res & 0x7FFF
        for name, cond in ((H_NAMES[0], mag <= inf), (H_NAMES[1], res == canon), (H_NAMES[2], res == canon),
                           (H_NAMES[3], res == canon), (H_NAMES[4], mag == inf),
                           (H_NAMES[5], (mag < (inf & -inf)) & (mag != 0))):
            ok = np.where(p == name, cond, ok)
    elif dtype == "longdouble":
        ca, cb, rc = _x_class(acc), _x_class(src), _x_result_class(res)
        nan_in = (ca == 5) | (ca == 6) | (cb == 5) | (cb == 6)
        if op in ("sum", "prod"):
            ok = np.where(nan_in, (rc == 3) | (rc == 4), ok)                # a NaN operand: a NaN comes out
            ok = np.where(~nan_in & ((ca == 7) | (cb == 7)), rc == 4, ok)   # an unsupported one: the indefinite
            for suffix, want in (("denormal result", 1), ("overflow result", 2), (": indefinite", 4)):
                ok = np.where(np.array([s.endswith(suffix) for s in p]), rc == want, ok)
            plain = np.array([": " not in s for s in p]) & (ca < 5) & (cb < 5)
            ok = np.where(plain, rc != 4, ok)
        else:
            ok = same_bits(dtype, res, acc) | same_bits(dtype, res, src)
            unordered = nan_in | (ca == 7) | (cb == 7)
            ok = np.where(unordered, same_bits(dtype, res, src), ok)
    elif dtype in ("float", "double"):
        for name in set(p.tolist()):
            ok = np.where(p == name, _part_rule(FMT[dtype], name, res, acc, src), ok)
    elif op == "sum":
        F = FMT[dtype]
        re = _real_codes(op, _c(acc.real), _c(src.real))
        im = _real_codes(op, _c(acc.imag), _c(src.imag), first_is_src=dtype == "complexf", split_both=True, F=F)
        rn = _part_names(op)
        for code in range(4):
            ok = np.where(re == code, _part_rule(F, rn[code], _c(res.real), _c(acc.real), _c(src.real)), ok)
            ok &= np.where(im == code, _part_rule(F, rn[code], _c(res.imag), _c(acc.imag), _c(src.imag)), True)
        # both NaN, payloads differ: float complex takes the incoming one, double complex the accumulator's
        winner = _c(src.imag) if dtype == "complexf" else _c(acc.imag)
        ok &= np.where(im == BOTH_NAN, _bits(F, _c(res.imag)) == (_bits(F, winner) | F.quiet), True)
    else:
        F = FMT[dtype]
        x, y = _c(res.real), _c(res.imag)
        nx, ny = np.isnan(x), np.isnan(y)
        indef = (_bits(F, x) == F.indefinite) | (_bits(F, y) == F.indefinite)
        for name in CP_NAMES:
            if name == CP_PLAIN:
                cond = ~nx & ~ny
            elif name == CP_ONE:
                cond = nx ^ ny
            elif name == CP_BOTH:
                cond = nx & ny
            elif name.endswith(CP_SUB[0]):
                cond = np.isinf(x) & np.isinf(y)
            else:       # recovery: an infinite part or (Inf x 0 twice) none, and every NaN part the indefinite
                cond = (nx | ny) & indef & (~nx | (_bits(F, x) == F.indefinite)) & (~ny | (_bits(F, y) == F.indefinite))
            ok = np.where(p == name, cond, ok)
    return np.nonzero(~np.asarray(ok, bool))[0], p


# ---------------------------------------------------------------------------
# the directed tables
# ---------------------------------------------------------------------------
def _cross(vals, t):
    v = np.array(vals, dtype=t) if not isinstance(vals, np.ndarray) else vals
    return np.repeat(v, len(v)), np.tile(v, len(v))


def _real_values(dtype):
    F = FMT[dtype]
    fi = np.finfo(F.f)
    q = int(F.quiet)
    return np.array([F.nan(0x155), F.nan(q - 1, negative=True), F.nan(1, quiet=False), F.nan(0x2A, True, False),
                     np.inf, -np.inf, 0.0, -0.0, 1.5, -2.25, fi.max, -fi.max, fi.tiny / 4, 1 + fi.eps, 3.0], dtype=F.f)


def _int_values(dtype):
    info = np.iinfo(NP[dtype])
    root = int(np.floor(np.sqrt(float(info.max))))
    while (root + 1) ** 2 <= info.max:
        root += 1
    while root ** 2 > info.max:
        root -= 1
    return np.array([0, 1, -1, 2, -2, 7, info.min, info.max, info.min + 1, info.max - 1, info.max // 2 + 1,
                     info.min // 2, root, root + 1, -root, 300, -12345], dtype=NP[dtype])


def _half_values(dtype):
    t = _half_ref.special_table(dtype)[:32]
    pick = [0, 1, 2, 3, 5, 8, 10, 12, 14, 16, 17, 21, 24, 27, 28, 29]
    pos = t[pick]
    return np.concatenate([pos, pos[[0, 1, 2, 4, 5, 8, 9, 13]] | 0x8000]).astype(np.uint16)


def _x_values():
    top = 1 << 63
    v = [x87(0, 0, 0), x87(1, 0, 0),                                            # zeros
         x87(0, 0, 0x123456789), x87(1, 0, top - 1),                            # denormals
         x87(0, 0, top | 0x123), x87(1, 0, top | (top - 1)),                    # pseudo-denormals
         x87(0, 16383, top | 0x5555), x87(1, 16385, top | (top - 1)),           # normals
         x87(0, 0x7FFF, top), x87(1, 0x7FFF, top),                              # infinities
         x87(0, 0x7FFF, (3 << 62) | 12345), x87(1, 0x7FFF, (3 << 62) | 7),      # quiet NaNs
         x87(0, 0x7FFF, top | 777), x87(1, 0x7FFF, top | 1),                    # signalling NaNs
         x87(0, 100, 0x7FFFFFFFFFFFFFFF), x87(1, 0x7FFF, 0x4000000000000001),   # unnormal, pseudo-NaN
         x87(0, 0x7FFE, top | 99), x87(0, 0x7FFD, (top - 1) | top),             # normals whose sum and product overflow
         x87(0, 8200, top | 5), x87(1, 8160, top | 3),                          # normals whose product is denormal
         x87(0, 2, top | (1 << 40)), x87(1, 2, top)]                            # normals whose sum is denormal
    return np.array(v, dtype=np.longdouble)


def _complex_sum_table(dtype):
    F = FMT[dtype]
    qa, sb = F.nan(0x155), F.nan(0x2A, True, False)
    part = {"number": [(1.5, 2.25), (np.inf, np.inf)], "acc": [(qa, 1.5), (sb, np.inf)],
            "src": [(1.5, qa), (-np.inf, sb)], "both": [(qa, sb), (sb, qa)], "invalid": [(np.inf, -np.inf), (-np.inf, np.inf)]}
    pairs = [p for k in ("number", "acc", "src", "both", "invalid") for p in part[k]]
    pairs += [(y, x) for x, y in pairs if not any(_same_pair(F, (y, x), q) for q in pairs)]     # both orders
    acc, src = [], []
    for ra, rb in pairs:
        for ia, ib in pairs:
            acc.append((ra, ia))
            src.append((rb, ib))
    return _complex(dtype, acc), _complex(dtype, src)


def _same_pair(F, p, q):
    return _bits(F, np.array(p, F.f)).tolist() == _bits(F, np.array(q, F.f)).tolist()


def _complex(dtype, parts):
    F = FMT[dtype]
    out = np.empty(len(parts), dtype=NP[dtype])
    out.real = np.array([p[0] for p in parts], dtype=F.f)
    out.imag = np.array([p[1] for p in parts], dtype=F.f)
    return out


def _complex_prod_table(dtype):
    F = FMT[dtype]
    inf, H = np.inf, np.finfo(F.f).max
    n1, n2, n3 = F.nan(0x155), F.nan(0x2A, True, False), F.nan(7, True)
    vals = [(inf, n1), (n2, inf), (inf, inf), (n1, n3), (0.0, 0.0), (1.0, 2.0), (-0.0, inf), (H, H), (n3, 0.0),
            (0.0, -inf), (H, n2), (n1, -H), (H, 0.0), (1.5, -0.0), (-inf, 1.0), (-H, 1.0)]
    i, j = np.repeat(np.arange(len(vals)), len(vals)), np.tile(np.arange(len(vals)), len(vals))
    return _complex(dtype, [vals[k] for k in i]), _complex(dtype, [vals[k] for k in j])


@functools.lru_cache(maxsize=None)
def table(op, dtype):
    """(acc, src): read-only arrays, the same on every call"""
    if dtype in INTS:
        acc, src = _cross(_int_values(dtype), NP[dtype])
    elif dtype in HALF:
        acc, src = _cross(_half_values(dtype), np.uint16)
    elif dtype == "longdouble":
        acc, src = _cross(_x_values(), np.longdouble)
    elif dtype in ("float", "double"):
        acc, src = _cross(_real_values(dtype), NP[dtype])
    elif op == "sum":
        acc, src = _complex_sum_table(dtype)
    else:
        acc, src = _complex_prod_table(dtype)
    acc.flags.writeable = src.flags.writeable = False
    return acc, src


PER_MUTANT = 3      # rows per wrong operator in representatives(), before their transposes


@functools.lru_cache(maxsize=None)
def representatives(op, dtype):
    """Row indices into table() for the layouts that spend a whole wave on a
    row: the first row of every catalogue entry; for every wrong operator of
    the pair the first, the middle and the last of the rows on which it
    differs from the reference (for the NaN-selection rules these hold two
    NaNs of different payloads, quiet and signalling); and every such row's
    transpose, so that each stands in both operand orders."""
    acc, src = table(op, dtype)
    p = paths(op, dtype, acc, src)
    rows = [int(np.nonzero(p == name)[0][0]) for name in CATALOGUE[(op, dtype)]]
    want = reference(op, dtype, acc, src)
    for name, pairs in WRONG_OPERATORS.items():
        if (op, dtype) in pairs:
            kills = np.nonzero(~same_bits(dtype, wrong_operator(name, op, dtype, acc, src), want))[0]
            rows += [int(kills[i]) for i in sorted({0, len(kills) // 2, len(kills) - 1})[:PER_MUTANT]]
    index = {(acc[i:i + 1].tobytes(), src[i:i + 1].tobytes()): i for i in range(len(acc))}
    rows += [index[(src[i:i + 1].tobytes(), acc[i:i + 1].tobytes())] for i in rows]
    return tuple(dict.fromkeys(rows))


# ---------------------------------------------------------------------------
# layouts: the table as the streaming kernels cut an array into waves
# ---------------------------------------------------------------------------
LANES = 64


def plain(op, dtype, n, seed):
    """n plain finite elements: no NaN, infinity or zero, magnitudes in
    [1, 2) (a chain of a few sums or products of them stays finite and normal)"""
    rng = np.random.default_rng(seed)
    if dtype in INTS:
        return rng.integers(2, 100, n).astype(NP[dtype])
    if dtype in HALF:
        mant = 10 if dtype == "half" else 7
        return ((0x3C00 if dtype == "half" else 0x3F80) + rng.integers(0, 1 << mant, n)).astype(np.uint16)
    if dtype == "longdouble":
        return (1 + rng.random(n)).astype(np.longdouble) * np.where(rng.random(n) < 0.5, -1, 1)
    if dtype in ("float", "double"):
        return ((1 + rng.random(n)) * np.where(rng.random(n) < 0.5, -1, 1)).astype(NP[dtype])
    return ((1 + rng.random(n)) + 1j * (1 + rng.random(n))).astype(NP[dtype])


def wave_layout(op, dtype, body0=0, rotation=0, full=True):
    """Operand arrays [acc, src, third] (third: plain finite), and where the
    table's rows went: a list of (kind, row, element index).

    body0 elements come first (the head the kernels peel when the target is
    off its 128-byte line; 0: none), then whole waves of 64 vectors of
    V = 16 / element size elements, then V - 1 tail elements:

      head, tail  consecutive table rows, starting at row rotation x (body0 +
                  V - 1): over all rotations() every row falls into one once
      sparse      (full only) one wave per row of representatives(): the row alone
                  among plain elements, at lane (5 k + 3) mod 64 and vector
                  element k mod V for the k-th
      uniform     (full only) one wave per row of representatives(): the row in
                  every lane and vector element
      packed      the whole table, consecutive, padded to whole vectors
    """
    acc_t, src_t = table(op, dtype)
    rows = len(acc_t)
    V = 16 // ES[dtype]
    wave = LANES * V
    reps = list(representatives(op, dtype)) if full else []
    packed = -(-rows // V) * V
    nbody = 2 * len(reps) * wave + packed
    n = body0 + nbody + (V - 1)
    seed = 77 + body0 + 13 * rotation
    out = [plain(op, dtype, n, seed), plain(op, dtype, n, seed + 1), plain(op, dtype, n, seed + 2)]
    where = []

    def put(kind, row, at):
        out[0][at], out[1][at] = acc_t[row], src_t[row]
        where.append((kind, row, at))

    edge = body0 + V - 1
    for k in range(edge):
        put("head" if k < body0 else "tail", (rotation * edge + k) % rows, k if k < body0 else body0 + nbody + k - body0)
    for k, row in enumerate(reps):
        put("sparse", row, body0 + k * wave + ((5 * k + 3) % LANES) * V + k % V)
    for k, row in enumerate(reps):
        for e in range(wave):
            put("uniform", row, body0 + (len(reps) + k) * wave + e)
    for row in range(rows):
        put("packed", row, body0 + 2 * len(reps) * wave + row)
    return out, where


def rotations(op, dtype, body0):
    """how many rotations of wave_layout put every row into a head or a tail"""
    edge = body0 + 16 // ES[dtype] - 1
    return -(-len(table(op, dtype)[0]) // edge) if edge else 0


def spaced_layout(op, dtype, n, spacing, member):
    """Member `member`'s n elements of the table spread over an array: row r
    of the table at element r x spacing + r mod 5 (so that rows fall on
    different lanes and vector elements), the table repeated to the array's
    end, plain elements between. Member 0 holds the accumulators, member 1 the
    incoming operands, further members plain elements throughout."""
    acc_t, src_t = table(op, dtype)
    x = plain(op, dtype, n, 500 + member)
    if member < 2 and n:
        t = (acc_t, src_t)[member]
        at = np.arange(0, n, spacing)
        at = at[at + 4 < n]
        r = np.arange(len(at)) % len(t)
        x[at + r % 5] = t[r]
    return x
