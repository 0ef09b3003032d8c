"""CPU: the operand table and the exact model of tests/_fp_add_cases.py, and
the host-heap path of shmemx_float_atomic_add_v / shmemx_double_atomic_add_v.

The table is what holds the accumulate's arithmetic to one correctly rounded
IEEE add on the GPU (tests/test_gpu_atomic.py, tests/atomic_worker.py), so it
is itself under test here: the model against numpy's add of the same format,
six wrong adders that the table must tell from the model, and the whole table
through the library's host loop (an SSE add in a compare-and-swap loop on the
bit pattern) before a GPU sees it.
"""
import os

import numpy as np
import pytest

import _fp_add_cases as fp
import test_bootstrap

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = ["float", "double"]


@pytest.mark.parametrize("dtype", TYPES)
def test_table_shape(dtype):
    """two equal-length arrays of the format, at most about 20,000 rows, the
    same on every call; at most 15 % of the rows are NaN rows, so the bit
    comparison covers the rest; every class the table names is there"""
    F = fp.FORMATS[dtype]
    t, s = fp.cases(dtype)
    assert t.dtype == s.dtype == F.np_float and t.shape == s.shape and t.ndim == 1
    assert 5000 <= t.size <= 20000
    t2, s2, _ = fp._build(dtype)
    assert (t2.view(F.np_uint) == t.view(F.np_uint)).all() and (s2.view(F.np_uint) == s.view(F.np_uint)).all()
    _, nan = fp.expected(dtype)
    assert 0.02 <= nan.mean() <= 0.15, nan.mean()
    lab = fp.labels(dtype)
    assert len(lab) == t.size
    for d in range(-(F.p + 3), F.p + 4):
        assert lab.count(f"random pair, exponents differ by {d}") >= 64, d
    for c in ("tie", "just above a tie", "just below a tie", "binade boundary", "x + (-x)", "cancellation to one ulp",
              "cancellation into the subnormals", "subnormal + subnormal", "subnormals that sum to the smallest normal",
              "smallest normal - smallest subnormal", "normal + subnormal, a tie",
              "smallest subnormal + smallest subnormal", "subnormal + 0", "max + half an ulp: a tie, to Inf",
              "max + a quarter ulp: stays max", "max + max", "zeros", "Inf + finite", "Inf + -Inf", "Inf + 0",
              "NaN + non-NaN", "NaN + NaN"):
        assert c in lab, c


@pytest.mark.parametrize("dtype", TYPES)
def test_the_results_the_issue_names(dtype):
    """x + (-x) = +0 in both orders, -0 + -0 = -0 and the other three zero
    pairs +0, max + half an ulp = Inf, max + a quarter ulp = max, Inf + -Inf
    a NaN, the smallest subnormal doubled"""
    F = fp.FORMATS[dtype]
    t, s = fp.cases(dtype)
    tb, sb = t.view(F.np_uint), s.view(F.np_uint)
    bits, nan = fp.expected(dtype)
    lab = np.array(fp.labels(dtype))
    assert (bits[lab == "x + (-x)"] == 0).all()
    z = lab == "zeros"
    assert z.sum() == 4
    both_neg = (tb[z] == F.sign_bit) & (sb[z] == F.sign_bit)
    assert (bits[z] == np.where(both_neg, F.np_uint(F.sign_bit), F.np_uint(0))).all() and both_neg.sum() == 1
    over = lab == "max + half an ulp: a tie, to Inf"
    assert ((bits[over] & F.np_uint(F.sign_bit - 1)) == F.inf).all() and not nan[over].any()
    stays = lab == "max + a quarter ulp: stays max"
    assert ((bits[stays] & F.np_uint(F.sign_bit - 1)) == F.max).all()
    assert nan[lab == "Inf + -Inf"].all() and not nan[lab == "Inf + Inf"].any()
    assert nan[lab == "NaN + non-NaN"].all() and nan[lab == "NaN + NaN"].all()
    tiny = (lab == "smallest subnormal + smallest subnormal") & (tb == 1) & (sb == 1)
    assert tiny.any() and (bits[tiny] == 2).all()


@pytest.mark.parametrize("dtype", TYPES)
def test_model_equals_numpy_add(dtype):
    """numpy's add of the same format (the host's SSE add): every bit on every
    non-NaN row, a NaN on every NaN row"""
    F = fp.FORMATS[dtype]
    t, s = fp.cases(dtype)
    bits, nan = fp.expected(dtype)
    with np.errstate(all="ignore"):
        ref = t + s
    assert ref.dtype == F.np_float
    assert (np.isnan(ref) == nan).all()
    msg = fp.mismatches(dtype, ref, where="numpy")
    assert msg is None, msg


# a class of rows on which each wrong adder has to show, beyond "somewhere"
SHOWS_IN = {
    "subnormal inputs flushed to zero": "subnormal + 0",
    "subnormal results flushed to zero": "smallest normal - smallest subnormal",
    "round toward zero": "just above a tie",
    "round half away from zero": "tie",
    "round toward -Inf": "x + (-x)",
    "saturation to max instead of Inf": "max + max",
}


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("wrong", list(fp.WRONG_ADDERS))
def test_a_wrong_adder_cannot_pass_the_table(dtype, wrong):
    """the same exact machinery with one rule changed differs from the model
    on non-NaN rows of each type (and in the class that rule is about), and
    the table's own comparison reports it"""
    assert set(SHOWS_IN) == set(fp.WRONG_ADDERS)
    t, s = fp.cases(dtype)
    bits, nan = fp.expected(dtype)
    got, got_nan = fp.wrong_adder(t, s, dtype, wrong)
    assert (got_nan == nan).all()
    differs = (got != bits) & ~nan
    assert differs.any(), (dtype, wrong)
    lab = np.array(fp.labels(dtype))
    assert differs[lab == SHOWS_IN[wrong]].any(), (dtype, wrong, SHOWS_IN[wrong])
    if wrong == "round toward -Inf":
        cancel = lab == "x + (-x)"
        assert (got[cancel] == fp.FORMATS[dtype].sign_bit).all()      # it shows as -0 on exact cancellation
    msg = fp.mismatches(dtype, got, where=wrong)
    assert msg is not None and f"{int(differs.sum())} of {t.size} rows" in msg and "row " in msg and "0x" in msg


@pytest.mark.parametrize("dtype", TYPES)
def test_comparison_takes_any_nan_for_a_nan_row_and_nothing_else(dtype):
    F = fp.FORMATS[dtype]
    bits, nan = fp.expected(dtype)
    got = bits.copy()
    got[nan] = F.inf | F.sign_bit | 1                       # a negative signalling NaN: still a NaN
    assert fp.mismatches(dtype, got) is None
    i = int(np.nonzero(nan)[0][0])
    got[i] = F.inf                                          # Inf is not
    assert "want a NaN" in fp.mismatches(dtype, got)
    order = np.arange(bits.size)[::-1]
    assert fp.mismatches(dtype, bits[::-1].copy(), order=order) is None
    assert fp.mismatches(dtype, bits[::-1].copy()) is not None


@pytest.mark.parametrize("npes", [2, 4])
@pytest.mark.parametrize("dtype", TYPES)
def test_arrival_orders_are_distinguishable(dtype, npes):
    """the inputs of the worker test accumulate_orders: finite, magnitudes in
    [1, 256), npes! orders, and the stated share of elements (25 % for 2 PEs,
    75 % for 4) with two or more distinct legal results; dropping or doubling
    one PE's term equals no legal result anywhere"""
    F = fp.FORMATS[dtype]
    init, sources, legal, share = fp.orders_case(dtype, npes)
    assert init.size == fp.ORDERS_N == 4096 + 64 and legal.shape == ({2: 2, 4: 24}[npes], init.size)
    for a in [init] + sources:
        assert a.dtype == F.np_float and ((np.abs(a) >= 1) & (np.abs(a) < 256)).all()
    assert share >= fp.ORDERS_MIN_SHARE[npes], share
    assert fp.illegal_elements(dtype, npes, legal[-1]).size == 0
    for k in (0, npes - 1):
        lost = init.copy()
        doubled = init.copy()
        for pe in range(npes):
            if pe != k:
                lost = (lost + sources[pe]).astype(F.np_float)
            doubled = (doubled + sources[pe]).astype(F.np_float)
        doubled = (doubled + sources[k]).astype(F.np_float)
        assert fp.illegal_elements(dtype, npes, lost).size == init.size
        assert fp.illegal_elements(dtype, npes, doubled).size == init.size


@pytest.mark.parametrize("npes", [1, 2])
def test_the_table_through_the_host_heap(tmp_path, npes):
    """shmemx_float_atomic_add_v and shmemx_double_atomic_add_v on a host-heap
    target without a GPU: 1 PE onto itself, and 2 PEs of which only PE 0 adds,
    into PE 1 (one adder: one right answer). The target sits one element off
    a 16-byte boundary between sentinels. Every non-NaN row equals the model
    in every bit, NaN rows are NaNs, sentinels and source stay as they were.
    The PEs write what they hold to files; the comparison is made here."""
    body = f"""
    import numpy as np
    sys.path.insert(0, {HERE!r})
    import _fp_add_cases as fp
    G = 16
    for name in ('float', 'double'):
        t, s = fp.cases(name)
        n, es = t.size, t.itemsize
        buf = shm.malloc((G + 1 + n + G) * es)
        assert buf % 16 == 0
        B = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)), shape=((G + 1 + n + G) * es,))
        B[:] = 0xA5
        B[(G + 1) * es: (G + 1 + n) * es] = t.view(np.uint8)
        src = s.copy()
        shm.barrier_all()
        if me == 0:
            shm.atomic_add_v(name, buf + (G + 1) * es, src.ctypes.data, n, npes - 1)
        shm.barrier_all()
        np.save(os.path.join({str(tmp_path)!r}, f'{{name}}_target_{{me}}.npy'), B.copy())
        np.save(os.path.join({str(tmp_path)!r}, f'{{name}}_source_{{me}}.npy'), src.view(np.uint8))
        shm.barrier_all()
        shm.free(buf)
    shm.finalize()
    print('ok')
    """
    for rc, out in test_bootstrap.spawn(npes, body, tmp_path):
        assert rc == 0 and "ok" in out, out
    G = 16
    for dtype in TYPES:
        F = fp.FORMATS[dtype]
        t, s = fp.cases(dtype)
        n, es = t.size, t.itemsize
        for pe in range(npes):
            B = np.load(tmp_path / f"{dtype}_target_{pe}.npy")
            src = np.load(tmp_path / f"{dtype}_source_{pe}.npy")
            assert B.size == (G + 1 + n + G) * es
            assert (B[:(G + 1) * es] == 0xA5).all() and (B[(G + 1 + n) * es:] == 0xA5).all(), (dtype, pe, "sentinels")
            assert (src == s.view(np.uint8)).all(), (dtype, pe, "source changed")
            got = B[(G + 1) * es: (G + 1 + n) * es].copy().view(F.np_uint)
            if pe == npes - 1:
                msg = fp.mismatches(dtype, got, where=f"host heap, {npes} PEs")
                assert msg is None, msg
            else:
                assert (got == t.view(F.np_uint)).all(), (dtype, pe, "the adder's own copy changed")
