"""CPU: the byte-exact data-movement model (tests/_datamove_ref.py), its case
tables and its wrong movers, and the tables run on the symmetric host heap by
1, 2 and 3 PE processes without a GPU (SHMEM_BOOTSTRAP_ONLY=1): put / get
through put_bytes' and get_bytes' memmove route, the collectives through
pull_host (csrc/coll.c). The worker (tests/_datamove_worker.py), the model and
the tables are the ones tests/test_gpu_datamove.py runs on the device heap.
"""
import json
import os
import sys

import numpy as np
import pytest

import _datamove_ref as ref
import oracle
from _pes import launch

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_64K = {"gpu": True, "fused_max": 65536, "scratch_chunk": 256 << 20}
ENV_CHUNK = {"gpu": True, "fused_max": 2 << 20, "scratch_chunk": 1 << 20}
CHUNK_PAIR = ((1 << 20) - 8, 1 << 20, (1 << 20) + 8)


def gpu_tables(npes=4):
    """every table of the GPU tests, with the setting each runs under"""
    ids = ref.Ids()
    chunk = ref.collective_table(ids, npes, 2 << 20, extra_bytes=CHUNK_PAIR, limits=False)
    return [(ref.gpu_putget_tables(), 3, ENV_64K), (ref.gpu_inprocess_tables(), 1, ENV_64K),
            (ref.collective_table(ref.Ids(), npes, 65536), npes, ENV_64K), (chunk, npes, ENV_CHUNK)]


def test_tables_hold_what_the_issue_lists():
    pgt = ref.gpu_putget_tables()
    full = [c for c in pgt if (c["op"], c["sym"], c["loc"], c["peer"]) == ("put", "dev", "dev", "next")]
    sizes = {c["es"] * c["nelems"] for c in full}
    assert sizes == {0, 1, 3, 15, 16, 17, 127, 128, 129, 4095, 4096, 4097, 16383, 16384, 16385, (1 << 20) + 5}
    for n in ref.SMALL_SIZES:
        pairs = {(c["roff"], c["loff"]) for c in full if c["nelems"] == n}
        assert pairs == set(ref.PHASE_PAIRS) and len(pairs) == 17
        assert sum(1 for r, l in pairs if r and l and r != l) >= 2
    for n in ref.LARGE_SIZES:
        assert len({(c["roff"], c["loff"]) for c in full if c["nelems"] == n}) == 3
    ep = ref.entry_point_table(ref.Ids(), "dev", "dev", "self")
    assert len({c["fn"] for c in ep}) == 2 * 8 + 6 + 2 and len(ep) == 24 * 3
    assert all(c["roff"] == c["loff"] == c["es"] and c["nelems"] in (0, 1, 5) for c in ep)
    assert {c["es"] for c in ep if "longdouble" in c["fn"]} == {16}
    coll = ref.collective_table(ref.Ids(), 4, 65536)
    for bits in (32, 64):
        es = bits // 8
        b = [c for c in coll if c["op"] == "broadcast" and c["bits"] == bits]
        assert {0, 1, 3, 4, 5, 1023, 1024, 1025, 65536 // es, 65536 // es + 1} <= {c["n"] for c in b}
        for n in {c["n"] for c in b}:
            assert {(c["toff"], c["soff"]) for c in b if c["n"] == n} == \
                {(t, s) for t in range(0, 16, es) for s in range(0, 16, es)}
        assert {c["root"] for c in b if c["sets"] == [[0, 0, 4]]} == {0, 1, 2, 3}
        for op in ("broadcast", "fcollect", "collect"):
            mine = [c for c in coll if c["op"] == op and c["bits"] == bits]
            assert {c["tgt"] for c in mine} == {"dev", "host", "page", "mixed"}, op
            assert {json.dumps(c["sets"]) for c in mine} == {json.dumps(s) for s in ref.active_sets(4)}, op
        f = [c for c in coll if c["op"] == "fcollect" and c["bits"] == bits]
        assert {1, 3, 5, 1023, 1025} <= {c["n"] for c in f}
        assert any(c["n"] * es * c["sets"][0][2] == 65536 for c in f)
        assert any(c["n"] * es * c["sets"][0][2] == 65536 + es * c["sets"][0][2] for c in f)
        k = [c for c in coll if c["op"] == "collect" and c["bits"] == bits]
        assert {c["pattern"] for c in k} == set(ref.COLLECT_PATTERNS)
        assert all(c["toff"] % 16 != 0 for c in k)
    whole = [c for c in coll if c["op"] == "collect" and c["sets"] == [[0, 0, 4]]]
    by = {c["pattern"]: c["counts"][:4] for c in whole}
    assert by["zero_first"][0] == 0 and by["zero_last"][3] == 0 and 0 in by["zero_middle"][1:3]
    assert not any(by["all_zero"]) and sum(1 for v in by["one_non_zero"] if v) == 1
    assert all(v % 2 for v in by["unequal_odd"]) and len(set(by["unequal_odd"])) == 4


@pytest.mark.parametrize("bits", [32, 64])
def test_model_agrees_with_the_oracle_on_element_aligned_cases(bits):
    """oracle.broadcast / fcollect / collect restate the reference in
    elements; the model counts bytes: on every collective case of the tables
    the target bytes from the pointer on are the oracle's elements."""
    dt = np.int32 if bits == 32 else np.int64
    es = bits // 8
    for npes in (1, 3, 4):
        cases = [c for c in ref.collective_table(ref.Ids(), npes, 65536) if c["bits"] == bits]
        assert cases
        for c in cases:
            for s in c["sets"]:
                mem = ref.members(*s)
                srcs = [ref.content(c["id"], pe, ref.src_len(c, pe)).view(dt) for pe in mem]
                cap = max(ref.tgt_len(c, pe) for pe in mem) // es
                before = [np.full(cap, int.from_bytes(bytes([ref.SENT_T]) * es, "little"), dtype=dt)] * len(mem)
                if c["op"] == "broadcast":
                    want = oracle.broadcast(srcs, c["root"] % len(mem), before)
                else:
                    want = (oracle.fcollect if c["op"] == "fcollect" else oracle.collect)(srcs)
                for i, pe in enumerate(mem):
                    tgt, src = ref.images(c, npes, pe)
                    at = ref.GUARD + c["toff"]
                    got = tgt[at:at + len(want[i]) * es]
                    assert got.tobytes() == np.ascontiguousarray(want[i], dtype=dt).tobytes(), (c, pe)
                    # nothing but the result is written, and the source stays
                    assert (tgt[:at] == ref.SENT_T).all() and (tgt[at + len(got):] == ref.SENT_T).all(), (c, pe)
                    assert (src == ref.source_image(c, npes, pe)).all()


def test_every_wrong_mover_fails_a_case_and_the_model_fails_none():
    tables = gpu_tables()
    for cases, npes, env in tables:
        for c in cases[::7]:    # the model against itself, recomputed
            assert not ref.differs(c, npes, ref.Mover(), env)
    for wrong in ref.WRONG_MOVERS:
        caught = sum(1 for cases, npes, env in tables for c in cases
                     if ref.es_of(c) * c.get("nelems", 1) < 70000 and c.get("n", 0) < 70000
                     and ref.differs(c, npes, wrong, env))
        print(f"wrong mover {wrong.name}: fails {caught} cases")
        assert caught >= 1, wrong.name


def test_first_difference_names_result_guard_and_source():
    c = ref.pg(ref.Ids(), "put", 17, 1, 4, "dev", "dev")
    t, s = ref.images(c, 2, 0)
    assert ref.first_difference(c, 2, 0, t, s, t, s) is None
    for at, where, off in ((ref.GUARD + 1 + 16, "result", 16), (ref.GUARD + 1 + 17, "guard", 17),
                           (ref.GUARD, "guard", -1)):
        g = t.copy()
        g[at] ^= 1
        assert ref.first_difference(c, 2, 0, g, s, t, s) == {"id": c["id"], "pe": 0, "where": where, "offset": off}
    g = s.copy()
    g[ref.GUARD + 4 + 3] ^= 1
    assert ref.first_difference(c, 2, 0, t, g, t, s) == {"id": c["id"], "pe": 0, "where": "source", "offset": 3}


@pytest.mark.parametrize("npes", [1, 2, 3])
def test_tables_on_the_host_heap(tmp_path, npes):
    """every table on shmem_malloc's host heap, local sides in the host heap
    and in pageable memory, then 100 calls of all kinds mixed in one batch"""
    t = ref.cpu_tables(npes)
    rng = np.random.default_rng(npes)
    pool = [c for c in t["putget"] + t["collectives"] if ref.slot_bytes(c, npes) < 100000]
    mixed = [pool[i] for i in rng.choice(len(pool), 100, replace=False)]
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"batches": [t["putget"], t["collectives"], mixed]}))
    job = launch(npes, [sys.executable, os.path.join(HERE, "_datamove_worker.py"), str(spec)], gpu=False, timeout=120,
                 env={"SHMEM_BARRIER_TIMEOUT": "60", "TMPDIR": str(tmp_path)})
    print(f"datamove-cpu | {npes} PEs | put/get {ref.count_by_op(t['putget'])} | "
          f"collectives {ref.count_by_op(t['collectives'])} | {job.elapsed:.1f} s")
    for rec in job.records():
        assert rec["failures"] == [], rec["failures"][:10]
