"""Byte-exact model of the contiguous data movement of csrc/coll.c -- put / get
and the pull collectives broadcast, fcollect and collect -- with the case
tables the CPU tests (test_datamove_cpu.py) and the GPU tests
(test_gpu_datamove.py) share, and a list of wrong movers. Pure numpy: no GPU,
no library.

A case is a dict (it travels to the worker as JSON). Every case owns one slot
in each arena it may touch:

    slot = [ GUARD sentinel bytes | phase | the bytes of the call | sentinel ... ]

The pointer a call receives is slot + GUARD + phase; slots start on 128-byte
lines, so `phase` is the pointer's offset within its line. Byte k of PE pe's
source of case id is content(id, pe)[k]: a byte that lands at a wrong place, or
comes from a wrong PE, differs. The model counts in bytes throughout.

A mover turns a case into moves (dst_pe, dst_off, src_pe, src_off, nbytes):
bytes [src_off, src_off + nbytes) from src_pe's source pointer land at dst_off
from dst_pe's target pointer. images() applies them to the slots. Mover() is
the true model; WRONG_MOVERS are the mistakes the tables must catch.
"""
import functools

import numpy as np

GUARD = 128          # sentinel bytes before the pointer's line and at least as many after the data
SENT_T, SENT_S = 0x5A, 0xA5   # untouched target / source bytes
LINE = 128

TYPES = {"char": 1, "short": 2, "int": 4, "long": 8, "longlong": 8, "longdouble": 16, "double": 8, "float": 4}
# every contiguous put / get symbol and its element size in bytes
ENTRY_POINTS = {f"shmem_{t}_{d}": es for t, es in TYPES.items() for d in ("put", "get")}
ENTRY_POINTS.update({f"shmem_{d}{b}": b // 8 for d in ("put", "get") for b in (32, 64, 128)})
ENTRY_POINTS.update({"shmem_putmem": 1, "shmem_getmem": 1})

SMALL_SIZES = [0, 1, 3, 15, 16, 17, 127, 128, 129, 4095, 4096, 4097]
LARGE_SIZES = [16383, 16384, 16385, (1 << 20) + 5]   # 16 KiB: one block pass of the copy kernel at 4 vectors per lane
OFFSETS = [0, 1, 4, 8, 15]
PHASE_PAIRS = [(0, 0)] + [p for k in OFFSETS[1:] for p in ((0, k), (k, 0), (k, k))] + [(1, 4), (4, 1), (8, 15), (15, 8)]
LARGE_PAIRS = [(0, 0), (8, 8), (1, 4)]
ROUTE_SIZES = [0, 1, 17, 4097, 16385]   # the sub-table of the local-memory kinds that only choose a route


def members(start, logstride, size):
    return [start + i * (1 << logstride) for i in range(size)]


@functools.lru_cache(maxsize=512)
def content(cid, pe, n):
    return np.random.default_rng([int(cid), int(pe), 77]).integers(0, 256, n, dtype=np.uint8)


# ---------------------------------------------------------------------------
# geometry of a case
# ---------------------------------------------------------------------------
def my_set(c, pe):
    """the active set of c that holds pe, or None"""
    for s in c["sets"]:
        if pe in members(*s):
            return s
    return None


def peer_of(c, pe, npes):
    return pe if c["peer"] in ("self", "same") else (pe + 1) % npes


def es_of(c):
    return c["es"] if c["op"] in ("put", "get") else c["bits"] // 8


def src_len(c, pe):
    """bytes of PE pe's source"""
    if c["op"] in ("put", "get"):
        return c["es"] * c["nelems"]
    s = my_set(c, pe)
    if s is None:
        return 0
    if c["op"] == "collect":
        return c["counts"][members(*s).index(pe)] * es_of(c)
    return c["n"] * es_of(c)


def tgt_len(c, pe):
    """bytes the call may write from PE pe's target pointer"""
    if c["op"] in ("put", "get"):
        return c["es"] * c["nelems"]
    s = my_set(c, pe)
    if s is None:
        return 0
    if c["op"] == "broadcast":
        return c["n"] * es_of(c)
    if c["op"] == "fcollect":
        return c["n"] * es_of(c) * s[2]
    return sum(c["counts"][:s[2]]) * es_of(c)


def phases(c):
    """(target phase, source phase) in bytes"""
    if c["op"] == "put":
        return c["roff"], c["loff"]
    if c["op"] == "get":
        return c["loff"], c["roff"]
    return c["toff"], c["soff"]


def tgt_kind(c, pe):
    k = c["sym"] if c["op"] == "put" else c["loc"] if c["op"] == "get" else c["tgt"]
    if k == "mixed":           # pageable on odd PEs
        k = "page" if pe % 2 else "dev"
    return k


def src_kind(c):
    return c["loc"] if c["op"] == "put" else c["sym"]


def arenas(c, pe):
    """(target arena, source arena) of PE pe; a put onto its own source
    (peer "same") has its target pointer in the source arena"""
    s = "S" + src_kind(c)
    return (s if c.get("peer") == "same" else "T" + tgt_kind(c, pe)), s


def slot_bytes(c, npes):
    cap = max(max(tgt_len(c, pe), src_len(c, pe)) for pe in range(npes))
    return (2 * GUARD + 32 + cap + LINE - 1) // LINE * LINE


def layout(cases, npes):
    """({arena: bytes}, {(arena, id): slot offset}): the same on every PE"""
    size, at = {}, {}
    for c in cases:
        names = sorted({a for pe in range(npes) for a in arenas(c, pe)})
        for a in names:
            at[(a, c["id"])] = size.get(a, 0)
            size[a] = size.get(a, 0) + slot_bytes(c, npes)
    return size, at


# ---------------------------------------------------------------------------
# the movers
# ---------------------------------------------------------------------------
class Mover:
    """The true semantics (coll.c's header names the reference's lines)."""
    name = "true"

    def collect_offsets(self, c, size):
        es, off, out = es_of(c), 0, []
        for i in range(size):
            out.append(off)
            off += c["counts"][i] * es
        return out

    def source_member(self, i, size):
        return i

    def moves(self, c, npes):
        op, out = c["op"], []
        if op in ("put", "get"):
            if c["peer"] == "same":
                return out        # target == source: the bytes stay what they are
            n = c["es"] * c["nelems"]
            for me in range(npes):
                pe = peer_of(c, me, npes)
                out.append((pe, 0, me, 0, n) if op == "put" else (me, 0, pe, 0, n))
            return out
        es = es_of(c)
        for s in c["sets"]:
            mem = members(*s)
            size = len(mem)
            for dst in mem:
                if op == "broadcast":
                    root = mem[c["root"] % size]
                    if dst != root:      # a single-member broadcast writes nothing
                        out.append((dst, 0, root, 0, c["n"] * es))
                    continue
                offs = [i * c["n"] * es for i in range(size)] if op == "fcollect" else self.collect_offsets(c, size)
                for i in range(size):
                    nb = (c["n"] if op == "fcollect" else c["counts"][i]) * es
                    if nb:
                        out.append((dst, offs[i], mem[self.source_member(i, size)], 0, nb))
        return self.adjust(c, out)

    def adjust(self, c, moves):
        return moves

    # --- which code moves the bytes: put / get routes, collective schedules
    def fused_ok(self, total, size, env):
        return size >= 2 and env["fused_max"] != 0 and total <= env["fused_max"] and total <= env["scratch_chunk"]

    def route(self, c, pe, npes, env):
        """What PE pe's call runs. put / get: "memmove", "copy", "shift",
        "memcpy" or "noop"; collectives: "fused_pull", "copy", "shift",
        "host_wait" (host barriers; host or DMA copies, if any) or "none" (DMA
        copies between device barriers, or nothing at all). env: {"gpu",
        "fused_max", "scratch_chunk"}."""
        op = c["op"]
        tp, sp = phases(c)
        if op in ("put", "get"):
            n = c["es"] * c["nelems"]
            if n == 0:
                return "noop"
            if not env["gpu"]:
                return "memmove"
            kernel = "shift" if (sp - tp) % 16 else "copy"
            if c["sym"] == "host":
                return "memmove" if c["loc"] in ("host", "page") else "memcpy"
            if c["peer"] == "same":
                return "noop"
            if op == "put":   # the copy kernel reads device memory and page-locked host memory
                return kernel if c["loc"] in ("dev", "hip", "host") else "memcpy"
            return kernel if c["loc"] in ("dev", "hip") else "memcpy"
        s = my_set(c, pe)
        if s is None or not env["gpu"]:
            return "none"
        mem, es = members(*s), es_of(c)
        size, me = len(mem), mem.index(pe)
        # host barriers around the copies: on a GPU the entry waits on the host for the caller's queued work
        idle = "host_wait" if op == "collect" or (c["sym"] == "host" and size > 1) else "none"
        if c["sym"] == "host":
            return idle
        dev_target = tgt_kind(c, pe) in ("dev", "hip")
        if op == "broadcast":
            if size == 1:
                return "none"
            if self.fused_ok(c["n"] * es, size, env):
                return "fused_pull"     # the root launches it too, with nothing to pull
            if me == c["root"] % size or c["n"] == 0 or not dev_target:
                return "none"
            return "shift" if (sp - tp) % 16 else "copy"
        if op == "fcollect":
            nb = c["n"] * es
            if size > 1 and nb != 0 and self.fused_ok(nb * size, size, env):
                return "fused_pull"
            segs = [(i * nb, nb) for i in range(size)]
        else:
            segs = list(zip(Mover.collect_offsets(self, c, size), [c["counts"][i] * es for i in range(size)]))
        segs = [(o, n) for o, n in segs if n]
        if not segs or not dev_target:
            return idle
        return "shift" if any((sp - tp - o) % 16 for o, _ in segs) else "copy"


class ElementOffsets(Mover):
    """offsets counted in elements where bytes are meant"""
    name = "offsets_in_elements"

    def adjust(self, c, moves):
        return [(d, do // es_of(c), s, so, n) for d, do, s, so, n in moves]


class TailDropped(Mover):
    """the byte tail after the last whole 16-byte vector dropped"""
    name = "tail_dropped"

    def moves(self, c, npes):
        return [(d, do, s, so, n // 16 * 16) for d, do, s, so, n in Mover.moves(self, c, npes)]


class ToffTwice(Mover):
    """the copy-out of a pageable target adds the segment's offset twice"""
    name = "toff_twice"

    def adjust(self, c, moves):
        return [(d, do * 2 if tgt_kind(c, d) == "page" else do, s, so, n) for d, do, s, so, n in moves]


class ZeroNotSkipped(Mover):
    """a zero-count member of a collect takes the room of one element, so later offsets shift"""
    name = "zero_count_not_skipped"

    def collect_offsets(self, c, size):
        es, off, out = es_of(c), 0, []
        for i in range(size):
            out.append(off)
            off += max(c["counts"][i], 1) * es
        return out


class RootWritten(Mover):
    """broadcast writes the root's target too"""
    name = "root_target_written"

    def adjust(self, c, moves):
        if c["op"] != "broadcast":
            return moves
        roots = [mem[c["root"] % len(mem)] for mem in (members(*s) for s in c["sets"])]
        return moves + [(r, 0, r, 0, c["n"] * es_of(c)) for r in roots]


class LessForLessEqual(Mover):
    """the fused thresholds compared with < for <=: the bytes are the same, the schedule at the limit is not"""
    name = "threshold_lt_for_le"

    def fused_ok(self, total, size, env):
        return size >= 2 and env["fused_max"] != 0 and total < env["fused_max"] and total < env["scratch_chunk"]


class NextMember(Mover):
    """a collective's segment taken from member i + 1"""
    name = "segment_from_next_member"

    def source_member(self, i, size):
        return (i + 1) % size

    def adjust(self, c, moves):
        if c["op"] != "broadcast":
            return moves
        out = []
        for d, do, s, so, n in moves:
            mem = members(*my_set(c, d))
            out.append((d, do, mem[(mem.index(s) + 1) % len(mem)], so, n))
        return out


WRONG_MOVERS = [ElementOffsets(), TailDropped(), ToffTwice(), ZeroNotSkipped(), RootWritten(), LessForLessEqual(),
                NextMember()]


# ---------------------------------------------------------------------------
# expected images
# ---------------------------------------------------------------------------
def source_image(c, npes, pe):
    """PE pe's source slot as the test fills it -- and as it must still be afterwards"""
    _, sp = phases(c)
    img = np.full(slot_bytes(c, npes), SENT_S, dtype=np.uint8)
    n = src_len(c, pe)
    img[GUARD + sp:GUARD + sp + n] = content(c["id"], pe, n)
    return img


def images(c, npes, pe, mover=None, moves=None):
    """(target slot, source slot) of PE pe after the call, whole slots: the
    guards on both sides keep the sentinel, the source is unchanged"""
    mover = mover or Mover()
    tp, sp = phases(c)
    if moves is None:
        moves = mover.moves(c, npes)
    src = source_image(c, npes, pe)
    if c.get("peer") == "same":
        return src.copy(), src
    tgt = np.full(slot_bytes(c, npes), SENT_T, dtype=np.uint8)
    for d, do, s, so, n in moves:
        if d != pe or n <= 0:
            continue
        from_ = source_image(c, npes, s)
        a, b = GUARD + tp + do, GUARD + sp + so
        n = max(0, min(n, len(tgt) - a, len(from_) - b))   # a wrong mover may run off the slot
        tgt[a:a + n] = from_[b:b + n]
    return tgt, src


def differs(c, npes, wrong, env):
    """does `wrong` give case c other bytes, or another schedule, than the true model, on any PE"""
    true = Mover()
    if any(wrong.route(c, pe, npes, env) != true.route(c, pe, npes, env) for pe in range(npes)):
        return True
    mt, mw = true.moves(c, npes), wrong.moves(c, npes)
    if mt == mw:
        return False
    return any((images(c, npes, pe, moves=mt)[0] != images(c, npes, pe, moves=mw)[0]).any() for pe in range(npes))


def first_difference(c, npes, pe, got_t, got_s, want_t, want_s):
    """None, or {"id", "pe", "where": "result" | "guard" | "source", "offset"}:
    the first differing byte, counted from the target (or source) pointer"""
    tp, sp = phases(c)
    bad = np.flatnonzero(got_t != want_t)
    if len(bad):
        off = int(bad[0]) - GUARD - tp
        where = "source" if c.get("peer") == "same" else "result" if 0 <= off < tgt_len(c, pe) else "guard"
        return {"id": c["id"], "pe": pe, "where": where, "offset": off}
    bad = np.flatnonzero(got_s != want_s)
    if len(bad):
        return {"id": c["id"], "pe": pe, "where": "source", "offset": int(bad[0]) - GUARD - sp}
    return None


# ---------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------
class Ids:
    def __init__(self, first=0):
        self.n = first

    def __call__(self):
        self.n += 1
        return self.n - 1


def pg(ids, op, nbytes, roff, loff, sym, loc, peer="next", fn=None, es=1):
    return {"id": ids(), "op": op, "fn": fn or f"shmem_{op}mem", "es": es, "nelems": nbytes // es, "roff": roff,
            "loff": loff, "sym": sym, "loc": loc, "peer": peer}


def putget_table(ids, full, routes, peer="next"):
    """full / routes: lists of (op, symmetric side, local side). `full` runs
    every size at every phase pair (three pairs at the large sizes), `routes`
    the sub-table ROUTE_SIZES x LARGE_PAIRS."""
    out = []
    for op, sym, loc in full:
        out += [pg(ids, op, n, r, l, sym, loc, peer) for n in SMALL_SIZES for r, l in PHASE_PAIRS]
        out += [pg(ids, op, n, r, l, sym, loc, peer) for n in LARGE_SIZES for r, l in LARGE_PAIRS]
    for op, sym, loc in routes:
        out += [pg(ids, op, n, r, l, sym, loc, peer) for n in ROUTE_SIZES for r, l in LARGE_PAIRS]
    return out


def entry_point_table(ids, sym, loc, peer="next"):
    """every contiguous put / get symbol at 0, 1 and 5 elements, both pointers
    one element off a 16-byte boundary"""
    return [pg(ids, "put" if "put" in fn else "get", n * es, es, es, sym, loc, peer, fn, es)
            for fn, es in sorted(ENTRY_POINTS.items()) for n in (0, 1, 5)]


def self_table(ids, sym, loc):
    """pe == my_pe: other, non-overlapping addresses, and the same address"""
    out = putget_table(ids, [], [("put", sym, loc), ("get", sym, loc)], peer="self")
    out += [pg(ids, op, n, r, r, sym, sym, "same") for op in ("put", "get") for n in (1, 17, 4097) for r in (0, 4)]
    return out


def active_sets(npes):
    """the whole set; PE_start 1; logPE_stride 1; two disjoint sets calling at
    once; every PE alone (a single-member call)"""
    out = [[[0, 0, npes]]]
    if npes >= 2:
        out.append([[1, 0, npes - 1]])
        out.append([[0, 1, (npes + 1) // 2]])
        out.append([[0, 1, (npes + 1) // 2], [1, 1, npes // 2]])
        out.append([[p, 0, 1] for p in range(npes)])
    return out


def element_phases(es):
    return list(range(0, 16, es))


def bcast_counts(es, fused_max):
    edge = {511, 512, 513} if es == 8 else set()    # 4,096 bytes +- one element: one block's share of fused_pull
    lim = {fused_max // es, fused_max // es + 1} if fused_max else set()
    return sorted({0, 1, 3, 4, 5, 1023, 1024, 1025} | edge | lim)


def fcollect_counts(es, size, fused_max):
    lim = {fused_max // (es * size), fused_max // (es * size) + 1} if fused_max else set()
    return sorted({1, 3, 5, 1023, 1025} | lim)


COLLECT_PATTERNS = {
    "zero_first": [0, 3, 5, 7, 1, 9, 11, 13],
    "zero_middle": [3, 0, 5, 0, 7, 1, 0, 9],
    "zero_last": None,       # built per set size
    "all_zero": [0] * 8,
    "one_non_zero": [0, 5, 0, 0, 0, 0, 0, 0],
    "unequal_odd": [1, 3, 5, 7, 9, 11, 13, 15],
    "unequal_odd_large": [1023, 1, 1025, 3, 5, 1027, 7, 9],
}


def collect_counts(pattern, size):
    v = COLLECT_PATTERNS[pattern]
    if v is None:
        v = [2 * i + 3 for i in range(8)]
        v[size - 1] = 0
    elif pattern == "one_non_zero" and size == 1:
        v = [5] + [0] * 7
    return list(v)


def collective_table(ids, npes, fused_max, sym="dev", targets=("dev", "host", "page", "mixed"), extra_bytes=(),
                     limits=True):
    """broadcast, fcollect and collect cases for a job of npes PEs whose
    library runs with `fused_max`: every count at every pair of element-aligned
    phases, with roots, active sets and target kinds rotating so that each
    occurs with each count. extra_bytes: further broadcast sizes in bytes (the
    scratch_chunk pair), at phase 0 and one other, into every kind of
    target. limits=False: without the counts at the fused_max limit."""
    sets, out, k = active_sets(npes), [], 0
    lim = fused_max if limits else 0

    def rot():
        nonlocal k
        k += 1
        return sets[k % len(sets)], targets[(k // len(sets)) % len(targets)], k // 3

    for bits in (32, 64):
        es = bits // 8
        for n in bcast_counts(es, lim):
            for tp in element_phases(es):
                for sp in element_phases(es):
                    s, t, r = rot()
                    out.append({"id": ids(), "op": "broadcast", "bits": bits, "n": n, "root": r % s[0][2], "sets": s,
                                "toff": tp, "soff": sp, "sym": sym, "tgt": t})
        for nb in extra_bytes:
            for tp, sp in ((0, 0), (es, 8)):
                for t in targets:
                    out.append({"id": ids(), "op": "broadcast", "bits": bits, "n": nb // es, "root": k % npes,
                                "sets": sets[0], "toff": tp, "soff": sp, "sym": sym, "tgt": t})
        for tp in element_phases(es):
            for sp in element_phases(es):
                for j in range(7 if lim else 5):
                    s, t, _ = rot()
                    n = fcollect_counts(es, s[0][2], lim)[j]
                    out.append({"id": ids(), "op": "fcollect", "bits": bits, "n": n, "sets": s, "toff": tp,
                                "soff": sp, "sym": sym, "tgt": t})
        for pattern in COLLECT_PATTERNS:
            for s in sets:
                _, t, _ = rot()
                tp = (es, 16 - es)[k % 2]     # off the 16-byte phase
                counts = collect_counts(pattern, s[0][2])
                out.append({"id": ids(), "op": "collect", "bits": bits, "counts": counts, "pattern": pattern,
                            "sets": s, "toff": tp, "soff": (0, es)[k % 2], "sym": sym, "tgt": t})
    return out


def cpu_tables(npes):
    """everything a job without a GPU can run: the symmetric host heap, local
    sides in the host heap or in pageable memory"""
    ids = Ids()
    pgt = putget_table(ids, [("put", "host", "page"), ("get", "host", "page")],
                       [("put", "host", "host"), ("get", "host", "host")])
    pgt += entry_point_table(ids, "host", "page")
    pgt += self_table(ids, "host", "page")
    coll = collective_table(ids, npes, 65536, sym="host", targets=("host", "page"))
    return {"putget": pgt, "collectives": coll}


GPU_FULL = [("put", "dev", "dev"), ("get", "dev", "dev")]
GPU_ROUTES = [("put", "dev", "host"), ("put", "dev", "page"), ("put", "host", "dev"), ("put", "host", "page"),
              ("get", "dev", "hip"), ("get", "dev", "host"), ("get", "dev", "page"), ("get", "host", "dev"),
              ("get", "host", "page")]


def gpu_putget_tables():
    ids = Ids()
    return putget_table(ids, GPU_FULL, GPU_ROUTES) + self_table(ids, "dev", "dev")


def gpu_inprocess_tables():
    """PE 0 of 1: the self-targeted calls and every entry point"""
    ids = Ids()
    return self_table(ids, "dev", "dev") + entry_point_table(ids, "dev", "dev", "self") + \
        entry_point_table(ids, "dev", "hip", "self")


def mixed_sequence(npes, fused_max, ncalls=100, seed=20240607):
    """about `ncalls` calls drawn from all tables with a fixed seed, renumbered in order"""
    ids = Ids()
    pool = putget_table(ids, GPU_FULL, GPU_ROUTES) + collective_table(ids, npes, fused_max)
    pool = [c for c in pool if c["op"] not in ("put", "get") or c["es"] * c["nelems"] <= 16385]
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(pool), ncalls, replace=False)
    return [dict(pool[i], id=j) for j, i in enumerate(pick)]


def count_by_op(cases):
    out = {}
    for c in cases:
        out[c["op"]] = out.get(c["op"], 0) + 1
    return out
