"""CPU: the expectations of tests/test_gpu_stream_matrix.py are not vacuous.

The case builders of the stream matrix run here against the oracle alone:
  * a case that claims NaN coverage has an element where two members' inputs
    are NaNs of different bits and the oracle's results for those two members
    differ there -- so PE_start's result delivered to every member, or a
    gather that did not patch, would be caught;
  * an input called "finite" holds no NaN and its chain produces none (so the
    NaN word of such a call is clear, which is what the call is there for);
  * a rounds case is above or below one round as its expected schedule says;
  * every size class lies on its side of the one-shot and fused limits for
    its element size.
"""
import numpy as np

import _half_ref as R
import _inputs
import oracle
import test_gpu_stream_matrix as M

FUSED_MAX, ONESHOT_MAX = M.MATRIX_THRESHOLDS


def value_bytes(x, dtype):
    return oracle.as_value_bytes(np.ascontiguousarray(x), dtype)


def nan_met(c, xs, outs):
    """elements where members 0 and 1 both hold a NaN, of different bits, and
    the oracle's results for the two differ"""
    a, b = xs[0], xs[1]
    both = np.isnan(a) & np.isnan(b) & (value_bytes(a, c["dtype"]) != value_bytes(b, c["dtype"])).any(axis=1)
    differ = (value_bytes(outs[0], c["dtype"]) != value_bytes(outs[1], c["dtype"])).any(axis=1)
    return int((both & differ).sum())


def nan_claims():
    """(label, case, set, input kind, seed) of every call that claims NaN coverage"""
    out = []
    for f, o in M.FIXTURE_SETTINGS[:1]:      # the rows are the same under every setting
        out += [(f"fixture {c['id']}", c, c["sets"][0], "default", c["seed"]) for c in M.fixture_cases(f, o)
                if c.get("nan_claim")]
    seq, mixed = M.sequence_cases("0")
    out += [(f"sequence call {q['id']}", q, M.PAIR[0], "default", q["seed"]) for q in seq["calls"] if q.get("nan_claim")]
    for c in mixed:
        out += [(f"mixed {c['id']} chain", c, M.PAIR[0], "nan", c["seed"]),
                (f"mixed {c['id']} blocking call", c, M.PAIR[0], "nan", c["seed"] + 1)]
    for c in M.graph_pair_cases():
        for r, kind in enumerate(c["inputs"]):
            if kind == "nan":
                out.append((f"graph {c['id']} replay {r}", c, M.PAIR[0], kind, c["seed"] + r))
        for e, kind in enumerate(c["eager_after"]):
            if kind == "nan":
                out.append((f"graph {c['id']} eager {e}", c, M.PAIR[0], kind, c["seed"] + c["graph"] + e))
    return out


def test_nan_cases_meet_two_different_nans():
    claims = nan_claims()
    assert len(claims) > 40
    for label, c, s, kind, seed in claims:
        mem = M.members(*s)
        xs = M.first_sources(c, mem, kind, seed)
        steps = M.steps_of(c, s, kind, seed)
        assert nan_met(c, xs, steps[0]) > 0, f"{label}: no element where two NaNs of different bits meet"
        if "golden" in c:      # the fixture's rows are what the GPU test compares with: the oracle agrees
            for j, row in enumerate(M.golden_rows(c, "out")):
                assert (value_bytes(steps[0][j], c["dtype"]) == value_bytes(row, c["dtype"])).all(), (label, j)


def finite_calls():
    out = []
    seq, _ = M.sequence_cases("0")
    out += [(q, M.PAIR[0], q["seed"]) for q in seq["calls"] if q.get("inputs") == ["finite"]]
    for c in M.graph_pair_cases():
        out += [(c, M.PAIR[0], c["seed"] + r) for r, kind in enumerate(c["inputs"]) if kind == "finite"]
        out += [(c, M.PAIR[0], c["seed"] + c["graph"] + e) for e, kind in enumerate(c["eager_after"])
                if kind == "finite"]
    return out


def test_finite_inputs_hold_and_produce_no_nan():
    calls = finite_calls()
    assert len(calls) > 30
    for c, s, seed in calls:
        mem = M.members(*s)
        for x in M.first_sources(c, mem, "finite", seed):
            assert np.isfinite(x).all(), (c["id"], "a finite input is not finite")
        for step in M.steps_of(c, s, "finite", seed):
            for y in step:
                assert not np.isnan(y).any(), (c["id"], c["op"], "the oracle's result of finite inputs holds a NaN")


def test_the_seeded_source_is_not_nan_free():
    """why "finite" is not _inputs.source: the golden generator plants NaN and
    Inf in 8 % of the elements, and at the sequence's finite size two of them
    meet in one element"""
    xs = [_inputs.source("sum", "float", 70001, 900, pe) for pe in range(2)]
    assert np.isnan(xs[0]).any() and np.isnan(oracle.reduce_pe("sum", "float", xs, 0)).any()


def test_rounds_cases_lie_on_their_side_of_one_round():
    assert M.ROUND_BYTES == 84480
    cases = M.rounds_cases()
    for c in cases:
        nbytes = c["n"] * M.elem_size(c["dtype"])
        if c["ordered"]:
            assert (nbytes > M.ROUND_BYTES) == (c["expect"] == M.ROUNDS), c
        else:   # beside the ordered ones: larger than a round, and still none
            assert nbytes > M.ROUND_BYTES and c["expect"] == M.P2P, c
    by = {(c["op"], c["dtype"], bool(c.get("inplace")), bool(c.get("graph"))): c for c in cases}
    assert len(by) == len(cases) == 2 * (len(M.ROUNDS_TABLE) + 1)
    c = by["sum", "double", False, False]
    assert -(-c["n"] * 8 // M.ROUND_BYTES) == 4 and c["n"] * 8 % M.ROUND_BYTES != 0    # 4 rounds, the last partial
    assert {c["expect"] for c in cases} == {M.ROUNDS, M.P2P}


def test_size_classes_lie_on_their_side_of_the_limits():
    assert (FUSED_MAX, ONESHOT_MAX) == (64 << 10, 16 << 10)
    assert len(M.ALL_PAIRS) == 52 and len(set(M.ALL_PAIRS)) == 52
    for op, dtype in M.ALL_PAIRS:
        es = M.elem_size(dtype)
        half = dtype in R.TYPES
        one, two, multi = (M.class_size(cls, dtype) for cls in ("oneshot", "twoshot", "multi"))
        assert one * es <= ONESHOT_MAX
        assert multi * es > FUSED_MAX
        assert (multi * es) % 16 != 0 or es == 16      # a partial last vector (one element is one at 16 bytes)
        assert multi % (256 // es) != 0                # a partial shard (shards are 256-byte granular)
        if half:
            assert two is None and (one, multi) == (257, 33025)
        else:
            assert ONESHOT_MAX < two * es <= FUSED_MAX
        for cls in M.CLASSES:
            for inplace in (False, True):
                n = M.class_size(cls, dtype)
                if n is None:
                    continue
                want = M.class_schedule(cls, dtype, inplace)
                if half or (cls == "unaligned" and es < 16) or n * es > FUSED_MAX:
                    assert want == M.P2P
                elif n * es <= ONESHOT_MAX and not inplace:
                    assert want == M.ONESHOT
                else:
                    assert want == M.TWOSHOT
    # every matrix job: 52 pairs (44 where the 16-bit floats have no size), the 8 pe_start ones, the strided two
    for cls in M.CLASSES:
        for inplace in (False, True):
            cases = M.matrix_cases(cls, inplace)
            pairs = 44 if cls == "twoshot" else 52
            assert len(cases) == pairs + 8 + (2 if inplace and cls != "unaligned" else 0), (cls, inplace, len(cases))
            # the jobs by type group hold each of them once
            split = [c for g in M.GROUPS for c in M.matrix_cases(cls, inplace, g)]
            key = lambda c: (c["op"], c["dtype"], c.get("order"), str(c["sets"]))   # noqa: E731
            assert sorted(map(key, split), key=str) == sorted(map(key, cases), key=str), (cls, inplace)
            assert {(cls, inplace, g) for g in M.GROUPS if M.matrix_cases(cls, inplace, g)} <= set(M.MATRIX_JOBS)


def test_fixture_settings_reach_every_schedule():
    """the three settings' expectations, which the GPU runs assert case by case"""
    names = set()
    for f, o in M.FIXTURE_SETTINGS:
        cases = M.fixture_cases(f, o)
        assert len(cases) == 44 * 5 + 8 * 3 + 8
        assert all(c["sets"][0][2] <= 5 for c in cases)
        names |= {c["expect"] for c in cases}
        split = [c for g in M.GROUPS if g != "half-bfloat16" for c in M.fixture_cases(f, o, g)]
        key = lambda c: (c["op"], c["dtype"], c["golden"], c.get("family"), c.get("inplace"))   # noqa: E731
        assert sorted(map(key, split), key=str) == sorted(map(key, cases), key=str)
    assert names == {M.ONESHOT, M.TWOSHOT, M.P2P}, names


def test_no_case_runs_on_more_than_five_pes():
    seq, mixed = M.sequence_cases("2M")
    cases = [seq] + mixed + M.graph_pair_cases() + M.rounds_cases()
    for cls in M.CLASSES:
        cases += M.matrix_cases(cls, True)
    for c in cases:
        for s in c["sets"]:
            assert max(M.members(*s)) < 5, c
