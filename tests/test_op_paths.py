"""CPU: the catalogue of operator branches (tests/_op_paths.py) -- its tables
reach every branch, its classifier names the branch the reference's compiled
operator took, its tables tell one-rule mutations of the operators from the
reference, and a census of which branches the committed fixtures and the
ordinary seeded generator reach."""
import numpy as np
import pytest

import _half_ref
import _inputs
import _op_paths as P
import oracle
from test_oracle_golden import NAN_PAIRS, load_cases, load_nan_cases


@pytest.mark.parametrize("op,dtype", P.PAIRS)
def test_table_covers_its_catalogue_exactly(op, dtype):
    acc, src = P.table(op, dtype)
    assert len(acc) == len(src) <= 600
    got = set(P.paths(op, dtype, acc, src).tolist())
    want = set(P.CATALOGUE[(op, dtype)])
    assert len(want) == len(P.CATALOGUE[(op, dtype)])
    assert got == want, (sorted(want - got), sorted(got - want))


def test_tables_hold_both_operand_orders():
    """with a row (a, b) every table holds the row (b, a)"""
    for op, dtype in P.PAIRS:
        acc, src = P.table(op, dtype)
        there = {(a.tobytes(), b.tobytes()) for a, b in zip(acc.reshape(-1, 1), src.reshape(-1, 1))}
        assert all((b, a) in there for a, b in there), (op, dtype)


def _assert_rules(op, dtype, acc, src, res, ctx):
    bad, names = P.rule_violations(op, dtype, acc, src, res)
    assert len(bad) == 0, (f"{ctx} {op}/{dtype}: {len(bad)} results do not look as their branch says; first: "
                           f"[{names[bad[0]]}] {acc[bad[0]:bad[0] + 1].tobytes().hex()} op "
                           f"{src[bad[0]:bad[0] + 1].tobytes().hex()} -> {res[bad[0]:bad[0] + 1].tobytes().hex()}")


@pytest.mark.parametrize("op,dtype", P.PAIRS)
def test_classifier_names_what_the_reference_did_on_the_table(op, dtype):
    acc, src = P.table(op, dtype)
    _assert_rules(op, dtype, acc, src, P.reference(op, dtype, acc, src), "table")


def fold_steps(op, dtype, srcs, me):
    """(acc, src, result) of every step of member `me`'s fold, by the arbiter"""
    acc = np.ascontiguousarray(srcs[me]).copy()
    for i, s in enumerate(srcs):
        if i != me:
            res = P.reference(op, dtype, acc, s)
            yield acc, np.ascontiguousarray(s), res
            acc = res


def fixture_families(op, dtype):
    fam = {"golden": [(npes, ins, outs) for npes, ins, outs in load_cases(op, dtype) if ins.shape[1]]}
    if (op, dtype) in NAN_PAIRS:
        fam["nan"] = load_nan_cases(op, dtype)
    return fam


@pytest.mark.parametrize("op,dtype", oracle.PAIRS)
def test_classifier_names_what_the_reference_did_on_the_fixtures(op, dtype):
    """every step of every member's fold of every committed fixture: the
    chain of steps ends in the fixture's reference-built output, and every
    step's result looks as its branch says"""
    for family, cases in fixture_families(op, dtype).items():
        for npes, ins, outs in cases:
            for me in range(npes):
                res = np.ascontiguousarray(ins[me])
                for acc, src, res in fold_steps(op, dtype, [ins[i] for i in range(npes)], me):
                    _assert_rules(op, dtype, acc, src, res, f"{family} npes={npes} me={me}")
                assert P.same_bits(dtype, res, outs[me]).all(), (family, npes, me)


def test_the_model_behind_the_mutations_is_the_reference_on_the_tables():
    for op, dtype in sorted({pair for pairs in P.WRONG_OPERATORS.values() for pair in pairs}):
        acc, src = P.table(op, dtype)
        assert P.same_bits(dtype, P.model(op, dtype, acc, src), P.reference(op, dtype, acc, src)).all(), (op, dtype)


@pytest.mark.parametrize("name", list(P.WRONG_OPERATORS))
def test_table_tells_a_wrong_operator_from_the_reference(name):
    for op, dtype in P.WRONG_OPERATORS[name]:
        acc, src = P.table(op, dtype)
        wrong = P.wrong_operator(name, op, dtype, acc, src)
        differ = int((~P.same_bits(dtype, wrong, P.reference(op, dtype, acc, src))).sum())
        assert differ > 0, f"{op}/{dtype}: no table row tells '{name}' from the reference"


def test_layouts_place_every_row_and_keep_the_rest_plain():
    for op, dtype in (("prod", "complexf"), ("sum", "short"), ("min", "longdouble"), ("sum", "bfloat16")):
        acc_t, src_t = P.table(op, dtype)
        V = 16 // P.ES[dtype]
        body0 = 128 // P.ES[dtype] - 1 if V > 1 else 0
        (a, b, c), where = P.wave_layout(op, dtype, body0=body0)
        assert len(a) == len(b) == len(c) and (len(a) - body0) % V == V - 1
        kinds = {k for k, _, _ in where}
        assert kinds >= {"sparse", "uniform", "packed"} and (V == 1 or kinds >= {"head", "tail"})
        for kind, row, at in where:
            assert P.same_bits(dtype, a[at:at + 1], acc_t[row:row + 1]).all()
            assert P.same_bits(dtype, b[at:at + 1], src_t[row:row + 1]).all()
        assert {row for k, row, _ in where if k == "packed"} == set(range(len(acc_t)))
        # a sparse row is the only table row of its wave, at a lane and a vector element of its own
        sparse = [at - body0 for k, _, at in where if k == "sparse"]
        assert len({at // (64 * V) for at in sparse}) == len(sparse)
        assert len({(at // V) % 64 for at in sparse}) == min(len(sparse), 64)
        assert V == 1 or len({at % V for at in sparse}) == min(len(sparse), V)
        # a uniform row fills one whole wave, aligned to the waves of the vector body
        for k, row in enumerate(P.representatives(op, dtype)):
            ats = sorted(at - body0 for kk, r, at in where if kk == "uniform" and r == row)
            assert len(ats) == 64 * V and ats[0] % (64 * V) == 0 and ats[-1] - ats[0] == 64 * V - 1
        # over all rotations every row falls into a head or a tail
        if V > 1:
            edge = set()
            for rot in range(P.rotations(op, dtype, body0)):
                edge |= {row for k, row, _ in P.wave_layout(op, dtype, body0, rot, full=False)[1] if k in ("head", "tail")}
            assert edge == set(range(len(acc_t)))
        x = P.spaced_layout(op, dtype, 13 * len(acc_t) + 7, 13, 0)
        assert len(x) == 13 * len(acc_t) + 7
        assert set(P.paths(op, dtype, x, P.spaced_layout(op, dtype, len(x), 13, 1)).tolist()) == set(P.CATALOGUE[(op, dtype)])


@pytest.mark.parametrize("name", list(P.WRONG_OPERATORS))
def test_sparse_and_uniform_rows_tell_a_wrong_operator_from_the_reference(name):
    """not only the whole table: the rows that wave_layout places alone in a
    wave (the divergent redo) and over a whole wave (the uniform case) tell
    every wrong operator from the reference, and hold each row's transpose"""
    for op, dtype in P.WRONG_OPERATORS[name]:
        acc_t, src_t = P.table(op, dtype)
        where = P.wave_layout(op, dtype)[1]
        for kind in ("sparse", "uniform"):
            rows = sorted({row for k, row, _ in where if k == kind})
            acc, src = acc_t[rows], src_t[rows]
            differ = ~P.same_bits(dtype, P.wrong_operator(name, op, dtype, acc, src), P.reference(op, dtype, acc, src))
            assert differ.any(), f"{op}/{dtype}: no {kind} row tells '{name}' from the reference"
            there = {(acc[i:i + 1].tobytes(), src[i:i + 1].tobytes()) for i in range(len(rows))}
            assert all((b, a) in there for a, b in there), (op, dtype, kind)
            if name == "the second NaN taken before the first" and dtype in ("float", "double"):
                F = P.FMT[dtype]
                bits = np.concatenate([acc[differ].view(F.u), src[differ].view(F.u)])
                assert ((bits & F.quiet) == 0).any() and ((bits & F.quiet) != 0).any(), (op, dtype, kind)
                assert (acc[differ].view(F.u) != src[differ].view(F.u)).all()


def test_the_spread_tables_reach_every_branch():
    """the collectives' inputs (tests/test_gpu_op_paths_pes.py): both sizes and spacings of every pair"""
    import test_gpu_op_paths_pes as T
    for op, dtype in T.PAIRS:
        for n, spacing in T.sizes(op, dtype):
            a, b = (_inputs.paths_source(op, dtype, n, spacing, m) for m in (0, 1))
            assert set(P.paths(op, dtype, a, b).tolist()) == set(P.CATALOGUE[(op, dtype)]), (op, dtype, n)
            assert not set(P.paths(op, dtype, b, _inputs.paths_source(op, dtype, n, spacing, 2)).tolist()) - \
                set(P.CATALOGUE[(op, dtype)])


# ---------------------------------------------------------------------------
# the census: which branches do the suite's inputs reach
# ---------------------------------------------------------------------------
def multipe_generator_cases():
    """(op, dtype, n, PEs, seed) of every case of test_gpu_multipe.py::test_four_pes_all_44_pairs_p2p_and_exact"""
    import test_gpu_multipe as M
    return [(c["op"], c["dtype"], c["n"], M.members(*c["sets"][0]), c["seed"]) for c in M.four_pes_cases()]


def count(counts, op, dtype, srcs):
    for me in range(len(srcs)):
        for acc, src, _ in fold_steps(op, dtype, srcs, me):
            names, k = np.unique(P.paths(op, dtype, acc, src).astype(str), return_counts=True)
            for name, c in zip(names, k):
                counts[name] = counts.get(name, 0) + int(c)


@pytest.fixture(scope="module")
def census():
    """{(op, dtype): {family: {branch: steps}}}"""
    out = {pair: {} for pair in P.PAIRS}
    for op, dtype in oracle.PAIRS:
        for family, cases in fixture_families(op, dtype).items():
            counts = out[(op, dtype)].setdefault(family, {})
            for npes, ins, _ in cases:
                count(counts, op, dtype, [ins[i] for i in range(npes)])
    for op, dtype, n, pes, seed in multipe_generator_cases():
        count(out[(op, dtype)].setdefault("generator", {}), op, dtype,
              [_inputs.source(op, dtype, n, seed, pe) for pe in pes])
    for op, dtype in P.PAIRS:
        if dtype in P.HALF:     # no fixtures: the model's special-value sources, as the 16-bit suites draw them
            count(out[(op, dtype)].setdefault("generator", {}), op, dtype, _half_ref.sources(dtype, 4, 1000, 11))
    return out


def census_lines(census):
    lines = ["pair | family | branches reached / catalogue | steps | never reached"]
    for (op, dtype), fams in census.items():
        cat = P.CATALOGUE[(op, dtype)]
        for family, counts in fams.items():
            missing = [c for c in cat if c not in counts]
            lines.append(f"{op} {dtype} | {family} | {len(cat) - len(missing)}/{len(cat)} | {sum(counts.values())} | "
                         f"{'; '.join(missing) if len(missing) <= 12 else f'{len(missing)} entries'}")
    return lines


def test_census_of_the_fixtures_and_the_ordinary_generator(census):
    print("\n".join(census_lines(census)))
    for (op, dtype), fams in census.items():
        cat = set(P.CATALOGUE[(op, dtype)])
        for family, counts in fams.items():
            assert set(counts) <= cat, (op, dtype, family, sorted(set(counts) - cat))
    # true today, and to stay true: the fixtures of a pair that has a NaN family reach every branch of its
    # catalogue (a complex sum's entries pair one outcome per part: every outcome of either part)
    for op, dtype in NAN_PAIRS:
        def branches(names):
            return {b for name in names for b in P.components(op, dtype, name)}
        reached = branches(set(census[(op, dtype)]["golden"]) | set(census[(op, dtype)]["nan"]))
        want = branches(P.CATALOGUE[(op, dtype)])
        assert reached == want, (op, dtype, sorted(want - reached))
    # what the ordinary generator never reaches is printed above and not asserted: the directed
    # tables (tests/test_gpu_op_paths.py, tests/test_gpu_op_paths_pes.py) are there for it
