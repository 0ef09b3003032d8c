"""GPU: the stream-ordered reductions (shmemx_<T>_<op>_to_all_on_stream) over
the matrix the blocking calls are held to (tests/test_gpu_multipe.py).

  pairs      all 44 pairs and the 8 half / bfloat16 ones at 4 PEs, at one size
             per schedule (sizes derived from the thresholds the job sets and
             the worker asserts), not in place and in place, a chain of two;
             PE_start's order; two strided two-member sets at once
  fixtures   every golden and NaN-payload row of 2 to 5 members
  NaN word   two members alternating NaN-rich, NaN-free and tiny calls on one
             stream with no host wait, beside a blocking call on the other
             channel; a pair call captured into a graph (one parity of the NaN
             word baked in) replayed on NaN-rich, NaN-free, NaN-rich data
  rounds     version areas too small for one round: ordered pairs in several
             rounds, in place, captured; a non-ordered pair beside them

Every case asserts each member's bits (the oracle per member through
chain_want, the fixtures' rows, tests/_half_ref.py for the 16-bit floats) AND
the schedule the library reported, so a threshold change cannot quietly send
every case down one path. The case builders are plain functions:
tests/test_stream_matrix_cases.py runs them against the oracle alone, on the
CPU, to show the expectations are not vacuous.

Nothing here runs on more than 5 PEs: the stream-ordered calls have no
host-barrier fallback, and 8 and more members on a stream are not covered
(DESIGN.md section 2).
"""
import functools
import json
import os

import numpy as np
import pytest

import _half_ref as R
import _inputs
import oracle
from _compare import assert_match
from test_gpu_multipe import SOME as MULTIPE_SOME
from test_gpu_multipe import members, run_pes
from test_gpu_stream import chain_want, check_stream, stream_case

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = [pytest.mark.gpu, pytest.mark.multipe]

HALF_PAIRS = [(op, t) for t in R.TYPES for op in R.OPS]
ALL_PAIRS = list(oracle.PAIRS) + HALF_PAIRS
MANIFEST = json.load(open(os.path.join(HERE, "golden", "manifest.json")))
GOLDEN_ROWS, NAN_ROWS = MANIFEST["cases"], MANIFEST["nan_cases"]

# one job per type group, so that no test takes longer than the blocking calls' 9-process fixture job
GROUPS = {"short-int": ("short", "int"), "long-longlong": ("long", "longlong"), "float-double": ("float", "double"),
          "longdouble": ("longdouble",), "complex": ("complexf", "complexd"), "half-bfloat16": R.TYPES}

ONESHOT, TWOSHOT, P2P, ROUNDS = "stream-fused-oneshot", "stream-fused-twoshot", "stream-p2p", "stream-p2p-rounds"


def elem_size(dtype):
    return 2 if dtype in R.TYPES else np.dtype(oracle.NP[dtype]).itemsize


def size_bytes(text):
    return int(text[:-1]) << {"K": 10, "M": 20}[text[-1]] if text[-1] in "KM" else int(text)


# ---------------------------------------------------------------------------
# 1. every pair, every schedule, in place and not
# ---------------------------------------------------------------------------
MATRIX_ENV = {"SHMEM_FUSED_MAX_BYTES": "64K", "SHMEM_ONESHOT_MAX_BYTES": "16K"}
MATRIX_THRESHOLDS = [64 << 10, 16 << 10]
CLASSES = ("oneshot", "twoshot", "multi", "unaligned")
FULL4 = [[0, 0, 4]]
STRIDED = [[0, 1, 2], [1, 1, 2]]


def class_size(cls, dtype):
    """Elements of a size class for a type, None where the type does not run
    it: under the one-shot limit; between it and the fused limit; above the
    fused limit with a partial last vector and a partial shard; 3001 elements
    one element off 16-byte alignment (the multi-launch schedule, but for the
    16-byte types, which one element leaves aligned). The 16-bit floats are never fused: they run
    the first and third (257 and 33025 elements) and the unaligned one."""
    es = elem_size(dtype)
    if cls == "oneshot":
        return 257
    if cls == "twoshot":
        return None if dtype in R.TYPES else 24576 // es + 1
    if cls == "multi":
        return 65536 // es + 257
    return 3001


def class_schedule(cls, dtype, inplace):
    """The fused kernel takes a type it has, 16-byte aligned offsets and up to
    the fused limit; its one-shot fold up to the one-shot limit and never in
    place. One element off alignment leaves the 16-byte types aligned: their
    3001 elements are a fused two-shot."""
    es = elem_size(dtype)
    nbytes = class_size(cls, dtype) * es
    if dtype in R.TYPES or nbytes > MATRIX_THRESHOLDS[0] or (cls == "unaligned" and es % 16 != 0):
        return P2P
    return ONESHOT if nbytes <= MATRIX_THRESHOLDS[1] and not inplace else TWOSHOT


def matrix_cases(cls, inplace, group=None):
    """one size class, in place or not, for one type group (None: all of them)"""
    cases = []

    def add(op, dtype, sets, **kw):
        n = class_size(cls, dtype)
        if n is None or (group is not None and dtype not in GROUPS[group]):
            return
        cases.append(stream_case(len(cases), op, dtype, n, sets, chain=2, inplace=inplace, cls=cls,
                                 thresholds=MATRIX_THRESHOLDS, expect=class_schedule(cls, dtype, inplace),
                                 **dict({"offset": 1} if cls == "unaligned" else {}, **kw)))

    for op, dtype in ALL_PAIRS:
        add(op, dtype, FULL4)
    for op, dtype in MULTIPE_SOME:
        add(op, dtype, FULL4, order="pe_start")
    if inplace and cls != "unaligned":
        add("prod", "float", STRIDED)      # two members: the pair path
        add("max", "double", STRIDED)
    return cases


# ---------------------------------------------------------------------------
# expected values and the check
# ---------------------------------------------------------------------------
def golden_rows(c, which):
    g = np.load(os.path.join(HERE, "golden", f"golden_{c.get('family', '')}{c['op']}_{c['dtype']}.npz"))
    return [np.ascontiguousarray(r) for r in g[f"{which}_{c['golden']}"]]


def first_sources(c, mem, kind, seed):
    """The members' first sources, as tests/pe_worker.py stream_input builds them."""
    if "golden" in c:
        return golden_rows(c, "in")
    if c["dtype"] in R.TYPES:
        return R.sources(c["dtype"], len(mem), c["n"], seed)
    return [_inputs.by_kind(kind, c["op"], c["dtype"], c["n"], seed, q) for q in mem]


def chain_steps(c, mem, xs, k=None):
    """steps[i][j]: member j's target after call i + 1 of the chain. The
    reference's types: chain_want (oracle.reduce_pe per member and step); the
    16-bit floats: the per-member model the public calls are held to."""
    op, dtype, order = c["op"], c["dtype"], c.get("order", "reference")
    k = c["chain"] if k is None else k
    if dtype in R.TYPES:
        steps = []
        for _ in range(k):
            xs = [R.fold(op, dtype, xs, j if order == "reference" else 0) for j in range(len(mem))]
            steps.append(xs)
        return steps
    per_pe = [chain_want(op, dtype, c["n"], None, mem, k, pe, order, xs=xs) for pe in mem]
    return [[per_pe[j][i] for j in range(len(mem))] for i in range(k)]


@functools.lru_cache(maxsize=None)
def _steps_cached(key, k, kind, seed):
    c = json.loads(key)
    mem = members(*c["set"])
    return chain_steps(c, mem, first_sources(c, mem, kind, seed), k)


def steps_of(c, s, kind, seed, k=None):
    key = json.dumps(dict({f: c[f] for f in ("op", "dtype", "n") if f in c}, set=list(s),
                          order=c.get("order", "reference"),
                          **{f: c[f] for f in ("golden", "family") if f in c}), sort_keys=True)
    return _steps_cached(key, c["chain"] if k is None else k, kind, seed)


def assert_bits(got, want, c, ctx):
    if c["dtype"] in R.TYPES:
        got, want = np.asarray(got).view(np.uint16), np.asarray(want).view(np.uint16)
        assert got.shape == want.shape, (ctx, got.shape, want.shape)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"{ctx} {c['op']}/{c['dtype']}: {bad.size} of {want.size} elements differ, first at "
                               f"{int(bad[0])}: got {int(got[bad[0]]):#06x}, want {int(want[bad[0]]):#06x}")
    else:
        assert_match(got, want, c["op"], c["dtype"], ctx=ctx, strict=True)


def plain(c):
    """check_stream's kind of case: every step saved, the seeded sources, the
    reference's types (it computes the whole chain again for every PE, so the
    large sizes go through the cached steps_of instead; both are chain_want)"""
    return c["n"] <= 3001 and not (c.get("inplace") or c["dtype"] in R.TYPES or "inputs" in c or "golden" in c or
                                   "eager_after" in c)


def check_cases(results, cases, schedules=None):
    """Every member's bits and the reported schedule of every case; the
    schedule names seen are counted into `schedules`."""
    check_stream(results, [c for c in cases if plain(c)])
    for c in cases:
        k = c["chain"]
        kinds = c.get("inputs", ["default"])
        for s in c["sets"]:
            for j, pe in enumerate(members(*s)):
                res = results[pe]
                ctx = f"case {c['id']} {c.get('cls', '')}{' in place' if c.get('inplace') else ''} set {s} PE {pe}"
                sched = str(res[f"{c['id']}_schedule"][0])
                assert sched == c["expect"], f"{ctx}: schedule {sched}, expected {c['expect']}"
                if schedules is not None and j == 0 and s == c["sets"][0]:
                    schedules[sched] = schedules.get(sched, 0) + 1
                if plain(c):
                    continue
                if c.get("graph"):
                    for r in range(c["graph"]):
                        want = steps_of(c, s, kinds[r % len(kinds)], c["seed"] + r)[-1][j]
                        assert_bits(res[f"{c['id']}_r{r}"], want, c, f"{ctx} replay {r} ({kinds[r % len(kinds)]}):")
                    for e, kind in enumerate(c.get("eager_after", [])):
                        want = steps_of(c, s, kind, c["seed"] + c["graph"] + e)[-1][j]
                        assert_bits(res[f"{c['id']}_e{e}"], want, c, f"{ctx} eager call {e} after the replays ({kind}):")
                    continue
                steps = steps_of(c, s, kinds[0], c["seed"])
                for i in range(k if c.get("inplace") else 1, k + 1):
                    assert_bits(res[f"{c['id']}_{i}"], steps[i - 1][j], c, f"{ctx} step {i}:")
                if c.get("mixed"):
                    want = steps_of(c, s, kinds[0], c["seed"] + 1, 1)[0][j]
                    assert_bits(res[f"{c['id']}_host"], want, c, f"{ctx} blocking call beside the chain:")


def report(name, schedules):
    print(f"{name}: " + ", ".join(f"{k} x {v}" for k, v in sorted(schedules.items())))


MATRIX_JOBS = [(cls, inplace, group) for cls in CLASSES for inplace in (False, True) for group in GROUPS
               if matrix_cases(cls, inplace, group)]


@pytest.mark.parametrize("cls,inplace,group", MATRIX_JOBS,
                         ids=[f"{cls}-{'inplace' if inplace else 'apart'}-{group}" for cls, inplace, group in MATRIX_JOBS])
def test_every_pair_on_a_stream(tmp_path, cls, inplace, group):
    """52 pairs x one size class, a chain of two on 4 PEs; in place the n = 257
    calls are the fused two-shot (the one-shot fold would read what peers
    overwrite), the large ones the plain and the every-member shard folds
    writing into the shard that the peers' folds read around, and the strided
    two-member prod float the pair fold with its NaN-patched gather."""
    cases = matrix_cases(cls, inplace, group)
    seen = {}
    check_cases(run_pes(4, cases, tmp_path, extra_env=MATRIX_ENV), cases, seen)
    report(f"pairs {cls}{' in place' if inplace else ''} {group}", seen)


# ---------------------------------------------------------------------------
# 2. golden and NaN fixtures
# ---------------------------------------------------------------------------
FIXTURE_SETTINGS = [("1M", "64K"), ("2M", "0"), ("0", "0")]


def fixture_schedule(fused_max, oneshot_max, n, es, inplace):
    if n * es > size_bytes(fused_max):
        return P2P
    return ONESHOT if n * es <= size_bytes(oneshot_max) and not inplace else TWOSHOT


def fixture_cases(fused_max, oneshot_max, group=None):
    """every `cases` row of 2 to 5 members with n > 0 for the 44 pairs, every
    `nan_cases` row of 2, 3 and 5 members (the two-member ones in place too);
    for one type group, or (None) all"""
    cases = []
    thresholds = [size_bytes(fused_max), size_bytes(oneshot_max)]

    def add(op, dtype, row, k, **kw):
        if group is not None and dtype not in GROUPS[group]:
            return
        cases.append(stream_case(len(cases), op, dtype, row["n"], [[0, 0, row["npes"]]], chain=1, golden=k,
                                 thresholds=thresholds, **kw))
        c = cases[-1]
        c["expect"] = fixture_schedule(fused_max, oneshot_max, c["n"], elem_size(dtype), c.get("inplace"))

    for op, dtype in oracle.PAIRS:
        for k, row in enumerate(GOLDEN_ROWS[f"{op}_{dtype}"]):
            if 2 <= row["npes"] <= 5 and row["n"] > 0:
                add(op, dtype, row, k)
    for key, rows in NAN_ROWS.items():
        op, dtype = key.split("_")
        for k, row in enumerate(rows):
            if row["npes"] in (2, 3, 5):
                add(op, dtype, row, k, family="nan_", nan_claim=True)
                if row["npes"] == 2:
                    add(op, dtype, row, k, family="nan_", nan_claim=True, inplace=True)
    return cases


@pytest.mark.parametrize("group", [g for g in GROUPS if g != "half-bfloat16"])
@pytest.mark.parametrize("fused_max,oneshot_max", FIXTURE_SETTINGS,
                         ids=["fused-oneshot", "fused-twoshot-2M", "multi-launch"])
def test_fixtures_on_a_stream(tmp_path, fused_max, oneshot_max, group):
    """Member i's target must equal the fixture's row i, NaN payloads
    included; across the three settings the fused one-shot, the fused two-shot
    (ordered: through the stream channel's version areas) and the multi-launch
    schedule (ordered, and the two-member NaN word) each deliver every row."""
    cases = fixture_cases(fused_max, oneshot_max, group)
    results = run_pes(5, cases, tmp_path, extra_env={"SHMEM_FUSED_MAX_BYTES": fused_max,
                                                     "SHMEM_ONESHOT_MAX_BYTES": oneshot_max})
    seen = {}
    for c in cases:
        outs = golden_rows(c, "out")
        for i in range(c["sets"][0][2]):
            sched = str(results[i][f"{c['id']}_schedule"][0])
            assert sched == c["expect"], (c, i, sched)
            assert_match(results[i][f"{c['id']}_1"], outs[i], c["op"], c["dtype"], strict=True,
                         ctx=f"{c.get('family', '')}golden {c['op']}/{c['dtype']} case {c['golden']}"
                             f"{' in place' if c.get('inplace') else ''} PE {i}:")
        seen[c["expect"]] = seen.get(c["expect"], 0) + 1
    report(f"fixtures {fused_max}/{oneshot_max} {group}", seen)


# ---------------------------------------------------------------------------
# 3. the two-member NaN word, call after call on one stream
# ---------------------------------------------------------------------------
PAIR = [[0, 0, 2]]
SEQ_ONESHOT = "16K"


def sequence_cases(fused_max):
    """The stream twin of test_gpu_multipe.two_member_nan_sequence: sum and
    prod of float and double, in place and not, each a NaN golden row (515
    elements), a NaN-free call of 70001 + id elements and a tiny one whose
    second shard is empty (member 1 only clears the next call's NaN word),
    the whole sequence twice; then a NaN chain with a blocking NaN call on the
    other channel while it is in flight."""
    thresholds = [size_bytes(fused_max), size_bytes(SEQ_ONESHOT)]
    calls = []

    def add(op, dtype, n, inplace, **kw):
        q = {"id": len(calls), "op": op, "dtype": dtype, "n": n, "inplace": inplace, "seed": 900 + len(calls),
             "chain": 1, "sets": PAIR}
        q.update(kw)
        q["expect"] = fixture_schedule(fused_max, SEQ_ONESHOT, n, elem_size(dtype), inplace)
        calls.append(q)

    for rep in range(2):
        for op in ("sum", "prod"):
            for dtype in ("double", "float"):
                for inplace in (False, True):
                    add(op, dtype, NAN_ROWS[f"{op}_{dtype}"][0]["n"], inplace, golden=0, family="nan_",
                        nan_claim=True)
                    add(op, dtype, 70001 + len(calls), inplace, inputs=["finite"])
                    add(op, dtype, 3 + rep, inplace, inputs=["nan"])
    seq = {"id": 5000, "kind": "stream_seq", "sets": PAIR, "calls": calls, "thresholds": thresholds}
    mixed = [stream_case(5001 + i, op, dtype, 515, PAIR, chain=2, mixed=True, inputs=["nan"], nan_claim=True,
                         expect=fixture_schedule(fused_max, SEQ_ONESHOT, 515, elem_size(dtype), False))
             for i, (op, dtype) in enumerate((("sum", "float"), ("prod", "double")))]
    return seq, mixed


@pytest.mark.parametrize("fused_max", ["0", "2M"], ids=["multi-launch", "fused"])
def test_two_member_nan_word_sequence_on_a_stream(tmp_path, fused_max):
    """The stream channel keeps its own pair counter and NaN words: 48 calls
    queued with no host wait take each parity's word from set to clear and
    back, and a blocking pair call (host channel) runs beside a stream chain."""
    seq, mixed = sequence_cases(fused_max)
    results = run_pes(2, [seq] + mixed, tmp_path, extra_env={"SHMEM_FUSED_MAX_BYTES": fused_max,
                                                             "SHMEM_ONESHOT_MAX_BYTES": SEQ_ONESHOT})
    seen = {}
    for q in seq["calls"]:
        want = steps_of(q, PAIR[0], q.get("inputs", ["default"])[0], q["seed"])[0]
        for pe in range(2):
            sched = str(results[pe][f"{q['id']}_schedule"][0])
            assert sched == q["expect"], (q, pe, sched)
            assert_bits(results[pe][str(q["id"])], want[pe], q,
                        f"call {q['id']} n {q['n']}{' in place' if q['inplace'] else ''} PE {pe}:")
        seen[q["expect"]] = seen.get(q["expect"], 0) + 1
    check_cases(results, mixed, seen)
    report(f"pair sequence, fused limit {fused_max}", seen)


# ---------------------------------------------------------------------------
# 4. a pair call captured in a graph
# ---------------------------------------------------------------------------
GRAPH_INPUTS = ["nan", "finite", "nan", "finite"]


def graph_pair_cases():
    """float sum and double prod over two members, multi-launch: a chain of 1
    and of 3 pair calls bakes one parity of the NaN word into the graph (an odd
    count), so every replay sets the same word and clears only the other one;
    replays on NaN-rich, NaN-free, NaN-rich, NaN-free data, then an eager call
    on NaN-free and one on NaN-rich data over the same pair."""
    cases = []
    for op, dtype in (("sum", "float"), ("prod", "double")):
        for n in (65, 16384 // elem_size(dtype) + 65):
            for chain, inplace in ((1, False), (3, False), (1, True)):
                cases.append(stream_case(len(cases), op, dtype, n, PAIR, chain=chain, graph=4, inputs=GRAPH_INPUTS,
                                         eager_after=["finite", "nan"], inplace=inplace, nan_claim=True,
                                         thresholds=[0, 16 << 10], expect=P2P))
    return cases


def test_pair_call_captured_in_a_graph(tmp_path):
    cases = graph_pair_cases()
    seen = {}
    check_cases(run_pes(2, cases, tmp_path, extra_env={"SHMEM_FUSED_MAX_BYTES": "0",
                                                       "SHMEM_ONESHOT_MAX_BYTES": "16K"}), cases, seen)
    report("captured pair calls", seen)


# ---------------------------------------------------------------------------
# 5. rounds
# ---------------------------------------------------------------------------
ROUNDS_ENV = {"SHMEM_DEVICE_ORDER_SIZE": "128K", "SHMEM_FUSED_MAX_BYTES": "0", "SHMEM_ONESHOT_MAX_BYTES": "16K"}
# 64 KiB per channel, two slots of 32 KiB at 3 PEs, 512 + 4096 bytes of each alignment and stagger
ROUND_BYTES = ((64 << 10) // 2 - 512 - 4096) // 256 * 256 * 3
FULL3 = [[0, 0, 3]]
# (op, type, n, ordered: delivers every member's order through the version areas)
ROUNDS_TABLE = [("sum", "double", 40000, True), ("prod", "complexf", 40000, True), ("max", "float", 40000, True),
                ("sum", "bfloat16", 100000, True), ("sum", "longdouble", 3000, True),
                ("xor", "longlong", 40000, False)]


def rounds_schedule(dtype, n, ordered):
    return ROUNDS if ordered and n * elem_size(dtype) > ROUND_BYTES else P2P


def rounds_cases():
    cases = []
    for inplace in (False, True):
        for op, dtype, n, ordered in ROUNDS_TABLE:
            cases.append(stream_case(len(cases), op, dtype, n, FULL3, chain=2, inplace=inplace, ordered=ordered,
                                     thresholds=[0, 16 << 10], expect=rounds_schedule(dtype, n, ordered)))
        cases.append(stream_case(len(cases), "sum", "float", 40000, FULL3, chain=2, graph=3, inplace=inplace,
                                 ordered=True, thresholds=[0, 16 << 10], expect=ROUNDS))
    return cases


def test_rounds_on_a_stream(tmp_path):
    """3 PEs, version areas of 64 KiB per channel: one round is 3 x 28160
    bytes. Ordered pairs above that run in rounds (sum double in 4, the last
    one partial), in place too -- each round's fold writes into the shard the
    peers' folds of that round read around -- and captured; long double fits
    one round; xor is not ordered and takes none at any size."""
    assert ROUND_BYTES == 84480
    cases = rounds_cases()
    assert {c["expect"] for c in cases} == {ROUNDS, P2P}
    seen = {}
    check_cases(run_pes(3, cases, tmp_path, extra_env=ROUNDS_ENV), cases, seen)
    assert set(seen) == {ROUNDS, P2P}, seen
    report("rounds", seen)
