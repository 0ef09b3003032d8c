"""GPU: the directed operand tables (tests/_op_paths.py) through the
collective schedules on 2 and 3 PE processes: member 0 holds the table's
accumulators, member 1 its incoming operands (so the two meet in the order
the table names, and in the other order on member 1), a third member plain
finite elements. Float, double and complex sums and products; the one-shot,
two-shot and multi-launch settings of the fixture tests; a size below the
one-shot limit and one above it (the table spread at two spacings and
repeated); out of place and in place; every PE's target bit for bit against
the oracle. The two-member inclusive scan runs on the same inputs."""
import numpy as np
import pytest

import _inputs
import _op_paths as P
import oracle
from _compare import assert_match
from test_gpu_multipe import run_pes
from test_gpu_scan import run_pes as run_scan_pes

pytestmark = [pytest.mark.gpu, pytest.mark.multipe]

PAIRS = [(op, t) for op in ("sum", "prod") for t in ("float", "double", "complexf", "complexd")]
ONESHOT = 64 << 10      # the one-shot limit of the first threshold setting below


def sizes(op, dtype):
    """(n, spacing): every row once below the one-shot limit; above it the wider spacing, twice over"""
    rows, es = len(P.table(op, dtype)[0]), P.ES[dtype]
    small, large = (13 * rows + 7, 13), (2 * 61 * rows + 5, 61)
    assert small[0] * es < ONESHOT < large[0] * es <= 1 << 20, (op, dtype)
    return [small, large]


def path_cases(npes):
    cases = []
    for op, dtype in PAIRS:
        for n, spacing in sizes(op, dtype):
            for mode in ("dev", "inplace"):
                cases.append({"id": len(cases), "op": op, "dtype": dtype, "n": n, "sets": [[0, 0, npes]], "mode": mode,
                              "algorithm": "p2p", "seed": 0, "inputs": "paths", "spacing": spacing})
    return cases


def expected_schedule(c, fused_max, oneshot_max):
    """what csrc/sched_plan.h plans for a case under a threshold setting: the fused kernel up
    to fused_max bytes, one-shot up to oneshot_max when not in place, else its two-shot form;
    beyond fused_max the multi-launch shard schedules (their names start with "p2p")"""
    size = {"0": 0, "64K": 64 << 10, "1M": 1 << 20, "2M": 2 << 20}
    nbytes = c["n"] * P.ES[c["dtype"]]
    if nbytes > size[fused_max]:
        return "p2p"
    return "fused-oneshot" if nbytes <= size[oneshot_max] and c["mode"] != "inplace" else "fused-twoshot"


@pytest.mark.parametrize("npes", [2, 3])
@pytest.mark.parametrize("fused_max,oneshot_max", [("1M", "64K"), ("2M", "0"), ("0", "0")],
                         ids=["fused-oneshot", "fused-twoshot-2M", "multi-launch"])
def test_tables_through_the_collective_schedules(tmp_path, fused_max, oneshot_max, npes):
    cases = path_cases(npes)
    results = run_pes(npes, cases, tmp_path, extra_env={"SHMEM_FUSED_MAX_BYTES": fused_max,
                                                        "SHMEM_ONESHOT_MAX_BYTES": oneshot_max})
    seen = set()
    for c in cases:
        op, dtype = c["op"], c["dtype"]
        want_sched = expected_schedule(c, fused_max, oneshot_max)
        for pe in range(npes):
            sched = str(results[pe][str(c["id"]) + "_schedule"][0])
            assert sched == want_sched or (want_sched == "p2p" and sched.startswith("p2p")), (c, pe, sched)
        seen.add(want_sched)
        srcs = [_inputs.paths_source(op, dtype, c["n"], c["spacing"], m) for m in range(npes)]
        want = oracle.reduce_all(op, dtype, srcs)
        for pe in range(npes):
            assert_match(results[pe][str(c["id"])], want[pe], op, dtype, strict=True,
                         ctx=f"paths case {c['id']} {c['mode']} n {c['n']} PE {pe} "
                             f"({str(results[pe][str(c['id']) + '_schedule'][0])}):")
    assert seen == {("1M", "64K"): {"fused-oneshot", "fused-twoshot"}, ("2M", "0"): {"fused-twoshot"},
                    ("0", "0"): {"p2p"}}[(fused_max, oneshot_max)], seen


def test_tables_through_the_two_member_scan(tmp_path):
    cases = []
    for op, dtype in PAIRS:
        for n, spacing in sizes(op, dtype):
            for mode in ("dev", "inplace"):
                cases.append({"id": len(cases), "op": op, "dtype": dtype, "n": n, "set": [0, 0, 2], "mode": mode,
                              "excl": False, "seed": 0, "inputs": "paths", "spacing": spacing})
    run_scan_pes(2, cases, tmp_path)
