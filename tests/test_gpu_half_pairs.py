"""GPU: the half and bfloat16 arithmetic of every kernel form on every 16-bit
pattern, bit for bit against the model (tests/_half_ref.py).

The compiler selects instructions separately for each form the operator is
compiled into (ops.h apply / apply_fast + chain_end, the every-member fold,
the prefix fold, each in a vector and an element-wise kernel), so each form
runs the two pair sets the model itself is pinned on (tests/test_half_ref.py):

  exhaustive  every pattern x 64 partners, half of them near in exponent
  product     every pattern x 64 partners aimed at the product's edges
              (subnormal results, underflow, the last binades, overflow)

4,194,304 pairs per run, whole targets compared, the sentinel guards around
every target checked unchanged.

  two sources    combine aligned / everything one element off / sources at two
                 phases / in place; combine_orders (the one place the operands
                 meet swapped); combine_prefix
  three sources  sum and prod chains through combine, combine_orders and
                 combine_prefix: the intermediate is rounded to the type, an
                 intermediate NaN ends canonical
  nine sources   chained launches and the per-member fold, n = 524,288
  2 PEs          the public reductions and inscan on the same sets
"""
import numpy as np
import pytest

import _half_ref as R
import test_gpu_half as H
import test_gpu_scan as SC

pytestmark = pytest.mark.gpu

N = 64 << 16
GUARD = H.GUARD
SETS = sorted(R.PAIR_SETS)


@pytest.fixture(scope="module")
def arena(shm):
    a = H.Arena(shm, 100 << 20)
    yield a
    shm.sync()
    shm.free_device(a.base)


def run_form(shm, arena, what, call, op, dtype, srcs, wants, dst_off=0, src_off=lambda k: 0, inplace=False):
    """one launch sequence of `call` (combine, orders or prefix) on srcs;
    wants[j] is output j's expected bits (combine has one output). In place:
    output j is source j's buffer."""
    n, nsrc, nout = srcs[0].size, len(srcs), len(wants)
    stride = H.stride_for(n)
    slots = arena.slots(nsrc + nout, stride)
    for s in slots:
        H.poison(shm, s, stride)
    ptrs = H.upload_sources(shm, slots[:nsrc], srcs, src_off)
    where = [(slots[j], src_off(j)) if inplace else (slots[nsrc + j], dst_off) for j in range(nout)]
    dsts = [s + GUARD + o for s, o in where]
    if call == "combine":
        rc = shm.combine(op, dtype, dsts[0], ptrs, n)
    elif call == "orders":
        rc = shm.combine_orders(op, dtype, dsts, ptrs, n)
    else:
        rc = shm.combine_prefix(op, dtype, dsts, ptrs, n)
    assert rc == 0, (what, rc)
    shm.sync()
    for j, want in enumerate(wants):
        tag = f"{call} {dtype} {op} {what}" + (f" output {j}" if nout > 1 else "")
        H.assert_bits(H.read_target(shm, where[j][0], where[j][1], n, tag), want, tag)


@pytest.mark.parametrize("pairs", SETS)
@pytest.mark.parametrize("dtype", R.TYPES)
@pytest.mark.parametrize("op", R.OPS)
def test_two_sources_every_form(shm, arena, op, dtype, pairs):
    a, b = R.pair_set(pairs, dtype)
    ab, ba = R.step(op, dtype, a, b), R.step(op, dtype, b, a)
    srcs = [a, b]
    # the packed fast path
    run_form(shm, arena, f"{pairs} aligned", "combine", op, dtype, srcs, [ab])
    # a scalar head and tail, shifted vectors
    run_form(shm, arena, f"{pairs} all off by one element", "combine", op, dtype, srcs, [ab],
             dst_off=2, src_off=lambda k: 2)
    run_form(shm, arena, f"{pairs} sources at two phases", "combine", op, dtype, srcs, [ab],
             src_off=lambda k: (0, 4)[k])
    run_form(shm, arena, f"{pairs} in place", "combine", op, dtype, srcs, [ab], inplace=True)
    # member 1 folds (b op a): for min, max and NaN operands not member 0's bits
    run_form(shm, arena, pairs, "orders", op, dtype, srcs, [ab, ba])
    # prefix 0 is a's bits unchanged (a NaN's payload included)
    run_form(shm, arena, pairs, "prefix", op, dtype, srcs, [a, ab])


@pytest.mark.parametrize("pairs", SETS)
@pytest.mark.parametrize("dtype", R.TYPES)
@pytest.mark.parametrize("op", ["sum", "prod"])
def test_three_source_chains(shm, arena, op, dtype, pairs):
    """(a op b) op c: the intermediate rounded to the type (not kept in
    binary32), an intermediate NaN canonical at the chain's end"""
    a, b = R.pair_set(pairs, dtype)
    srcs = [a, b, R.third_operand(dtype, a, b)]
    folds = [R.fold(op, dtype, srcs, q) for q in range(3)]
    if op == "sum" and pairs == "exhaustive":
        assert (folds[0] != folds[2]).sum() >= 1000     # an order mistake cannot pass
    run_form(shm, arena, f"{pairs} chain of 3", "combine", op, dtype, srcs, [folds[0]])
    run_form(shm, arena, f"{pairs} chain of 3", "orders", op, dtype, srcs, folds)
    run_form(shm, arena, f"{pairs} chain of 3", "prefix", op, dtype, srcs,
             [a, R.step(op, dtype, a, b), folds[0]])


@pytest.mark.parametrize("dtype", R.TYPES)
@pytest.mark.parametrize("op", ["sum", "prod"])
def test_nine_sources(shm, arena, op, dtype):
    """past one launch's 8 sources: chained launches (combine) and a fold per
    member (combine_orders). Every 8th pair of the exhaustive set: every
    pattern still occurs as a, with 8 partners."""
    a, b = (x[::8].copy() for x in R.pair_set("exhaustive", dtype))
    assert a.size == 524288
    srcs = [a, b] + [R.third_operand(dtype, a, b, seed) for seed in range(1, 8)]
    run_form(shm, arena, "chain of 9", "combine", op, dtype, srcs, [R.left_fold(op, dtype, srcs)])
    run_form(shm, arena, "chain of 9", "orders", op, dtype, srcs, [R.fold(op, dtype, srcs, q) for q in range(9)])


# ---------------------------------------------------------------------------
# 2 PEs, the public calls
# ---------------------------------------------------------------------------
@pytest.mark.multipe
@pytest.mark.parametrize("pairs", SETS)
@pytest.mark.parametrize("dtype", R.TYPES)
def test_public_calls_two_pes(tmp_path, dtype, pairs):
    """shmemx_<T>_<op>_to_all on the pair sets, PE 0's source a and PE 1's b:
    four ops to another buffer, sum and prod in place, min in PE_start's
    order, a stream-ordered prod"""
    cases = []
    full = (0, 0, 2)
    for op in R.OPS:
        H.case(cases, op, dtype, N, full, "dev", inputs=pairs)
    for op in ("sum", "prod"):
        H.case(cases, op, dtype, N, full, "inplace", inputs=pairs)
    H.case(cases, "min", dtype, N, full, "dev", inputs=pairs, order="pe_start")
    H.case(cases, "prod", dtype, N, full, "dev", inputs=pairs, stream=True)
    for rec in H.run_pes(2, cases, tmp_path):
        assert len(rec["schedules"]) == len(cases) - 1    # every blocking call reported one
        for cid, sched in rec["schedules"].items():
            assert "fused" not in sched, (cases[int(cid)], sched)


@pytest.mark.multipe
@pytest.mark.parametrize("dtype", R.TYPES)
def test_inscan_two_pes(tmp_path, dtype):
    """shmemx_<T>_<op>_inscan on the pair sets: PE 0 receives a, PE 1 a op b"""
    cases = []
    for pairs in SETS:
        for op in R.OPS:
            SC.case(cases, op, dtype, N, (0, 0, 2), "dev", inputs=pairs)
    # the worker sizes its four buffers for 16-byte elements
    SC.run_pes(2, cases, tmp_path, extra_env={"SHMEM_DEVICE_HEAP_SIZE": "160M", "SHMEM_SYMMETRIC_HEAP_SIZE": "160M"})
