"""GPU: every streaming kernel of the combine layer beyond its first grid pass.

The hot-path kernels are grid-stride loops over a capped grid; one sweep of
the whole grid over the data is a grid pass ("Grid passes").
The rest of the suite probes the first-order edges at sizes where a block
makes one trip round its loop. Here every launch takes at least two full
passes and a partial last one, so what a loop carries from pass to pass is
exercised: prefetched registers, the `i < nvec` guards inside a partial
unrolled pass, blocks with no share of the last pass.

The rule, asserted for every case from the grid the library REPORTS
(mi355_last_launch_grid), never from the launch shape tables:

    units > 2 * 4 * 256 * gx

units: 16-byte vectors for the vector kernels, elements for the element-wise
ones; 4: the deepest per-lane unroll of this layer; 256: lanes per block. A
case that fails the rule no longer reaches a second pass: resize it.

Sizing: a call is launched once over the module's arena at full length to
learn its saturated grid (nothing uploaded, nothing read), then the real case
runs at 9 * 256 * gx + 256 + 37 vectors (+ V - 1 tail elements): the last pass
is partial, most blocks have nothing in it, one has a partly filled unroll.

Every comparison is of bits: oracle.reduce_pe through _compare.assert_match
(strict where NaNs are planted), numpy for byte copies. Targets are pre-filled
with a sentinel and compared with 256 guard bytes on both sides.

Inputs are gen_golden.values, drawn as a pool of 2^14 values per source and
spread over the array by random index (the long double generator is a Python
loop per element); the min/max cases take the sparse-specials data of
test_combine_orders_minmax_sparse_specials.

Left out: the x87 every-member sum/product and the float-complex every-member
product queue one block per 256 vectors (an uncapped grid), so they never
take a second pass.
"""
import ctypes

import numpy as np
import pytest

import gen_golden
import oracle
from _compare import assert_match
from shmem_reduce import DTYPES

pytestmark = pytest.mark.gpu

LANES = 256            # kBlock
DEEPEST_UNROLL = 4     # vectors per lane per pass, at most
GUARD = 256
SENT = 0xA5
ARENA_BYTES = 1 << 30
POOL = 1 << 14
LINE_OFF = 48          # the off-line layouts: 48 bytes past a 128-byte line


def rule_units(gx):
    return 2 * DEEPEST_UNROLL * LANES * gx


def sized_units(gx):
    return 9 * LANES * gx + LANES + 37


class Arena:
    def __init__(self, shm):
        self.shm = shm
        self.base = shm.malloc_device(ARENA_BYTES)
        assert self.base and self.base % 4096 == 0, self.base
        self._sent = np.zeros(0, np.uint8)

    def slots(self, k):
        size = (ARENA_BYTES // k) & ~4095
        return [self.base + i * size for i in range(k)], size

    def sentinel(self, nbytes):
        if len(self._sent) < nbytes:
            self._sent = np.full(nbytes, SENT, np.uint8)
        return self._sent[:nbytes]

    def poison(self, slot, off, nbytes):
        """sentinel over a target and its guards: [slot, slot + GUARD + off + nbytes + GUARD)"""
        self.shm.put(slot, self.sentinel(GUARD + off + nbytes + GUARD))

    def upload(self, slot, off, arr):
        """arr at slot + GUARD + off, sentinel guards around it"""
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.shm.put(slot, self.sentinel(GUARD + off))
        self.shm.put(slot + GUARD + off, raw)
        self.shm.put(slot + GUARD + off + raw.nbytes, self.sentinel(GUARD))

    def read(self, slot, off, nbytes, ctx):
        """the target's bytes, after checking the guards on both sides"""
        got = self.shm.get(slot, GUARD + off + nbytes + GUARD, np.uint8)
        lo = GUARD + off
        assert (got[:lo] == SENT).all(), f"{ctx}: bytes below the target were written"
        assert (got[lo + nbytes:] == SENT).all(), f"{ctx}: bytes above the target were written"
        return got[lo:lo + nbytes].copy()


@pytest.fixture(scope="module")
def arena(shm):
    a = Arena(shm)
    yield a
    _PREPARED.clear()
    shm.sync()
    shm.free_device(a.base)


# one prepared case (inputs uploaded, reference computed) is kept at a time and
# shared by that case's layouts, which pytest runs one after another
_PREPARED = {}


def prepared(key, build):
    if key not in _PREPARED:
        _PREPARED.clear()
        _PREPARED[key] = build()
    return _PREPARED[key]


def kernel_name(shm):
    L = shm.lib
    L.mi355_last_kernel.restype = ctypes.c_void_p
    L.mi355_kernel_name.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    buf = ctypes.create_string_buffer(512)
    assert L.mi355_kernel_name(L.mi355_last_kernel(), buf, 512) == 0
    return buf.value.decode()


def check_rule(shm, units, what, expect_kernel):
    """the module's rule, from the grid the library reports for the launch just made"""
    gx, gy = shm.last_launch_grid()
    name = kernel_name(shm)
    print(f"grid-pass | {what} | {name.split('(')[0]} | {gx} x {gy} | units {units} | "
          f"{units / (DEEPEST_UNROLL * LANES * gx):.2f} passes at unroll {DEEPEST_UNROLL}, "
          f"{units / (LANES * gx):.2f} at unroll 1")
    assert expect_kernel in name, (what, name)
    assert gx > 0 and units > rule_units(gx), \
        f"{what}: {units} units do not pass twice over a grid of {gx} x {gy} blocks: resize the case"
    return gx


def probe_grid(shm):
    gx, _ = shm.last_launch_grid()
    assert gx > 0
    return gx


def elem(dtype):
    es = np.dtype(oracle.NP[dtype]).itemsize
    return es, 16 // es


def spread(rng, pool, n):
    return pool[rng.integers(0, len(pool), n)]


def inputs(rng, op, dtype, n):
    return spread(rng, gen_golden.values(rng, op, dtype, POOL), n)


def sparse_minmax(rng, dtype, n, nsrc, late):
    """test_combine_orders_minmax_sparse_specials' data: full-mantissa values
    without NaN or zero, and a few NaNs, +-0 and equal-value ties planted, per
    source and at common positions of every source; a share of each from
    element `late` on (the last, partial pass)."""
    t = oracle.NP[dtype]
    pool = ((rng.uniform(-1, 1, POOL) + 2.0 ** -30) * np.exp2(rng.integers(-4, 4, POOL))).astype(t)
    pool[pool == 0] = t(1.5)

    def positions(k):
        return np.concatenate([rng.integers(0, n, k), rng.integers(late, n, k)])

    srcs = []
    for _ in range(nsrc):
        x = spread(rng, pool, n)
        x[positions(16)] = t(np.nan)
        x[positions(16)] = t(0.0)
        x[positions(8)] = t(-0.0)
        x[positions(8)] = t(0.25)
        srcs.append(x)
    zeros, nans, ties = positions(16), positions(8), positions(8)
    for k, x in enumerate(srcs):
        x[zeros] = t(0.0) if k % 2 else t(-0.0)
        x[nans] = t(np.nan) if k == nsrc - 1 else t(0.5)
        x[ties] = t(0.25)
    return srcs


def plant_nans(rng, dtype, srcs, late):
    """about 200 values of gen_golden.nan_values per source, 80 of them from element `late` on"""
    n = len(srcs[0])
    for s in srcs:
        pos = np.concatenate([rng.integers(0, n, 120), rng.integers(late, n, 80)])
        s[pos] = gen_golden.nan_values(rng, dtype, len(pos))


def has_nan(a):
    return np.isnan(a.real) | np.isnan(a.imag) if np.iscomplexobj(a) else np.isnan(a)


# ---------------------------------------------------------------------------
# the fold, mi355_combine
# ---------------------------------------------------------------------------
FOLD_CASES = ([("sum", "double", k) for k in (2, 3, 4, 5, 8)] + [("xor", "int", k) for k in (2, 3, 4, 5, 8)] +
              [("max", "float", 2), ("prod", "complexf", 2), ("sum", "longdouble", 3)])
# line: every pointer on its 128-byte line. head48: target and sources 48 bytes
# off it (a line head peeled before the multi-pass body). shift: target on its
# line, sources one element on (unaligned source loads).
FOLD_LAYOUTS = ["line", "head48", "shift"]


def fold_pointers(layout, es, tslot, sslots):
    """(target, sources, target offset in its slot, first element used): the
    sources lie at +LINE_OFF in their slots, so the layouts on the line start
    at the element that sits on the next line"""
    skip = (128 - LINE_OFF) // es
    if layout == "head48":
        return tslot + GUARD + LINE_OFF, [s + GUARD + LINE_OFF for s in sslots], LINE_OFF, 0
    if layout == "line":
        return tslot + GUARD, [s + GUARD + 128 for s in sslots], 0, skip
    return tslot + GUARD, [s + GUARD + 128 + es for s in sslots], 0, skip + 1


def prepare_fold(shm, arena, op, dtype, nsrc):
    es, V = elem(dtype)
    slots, ssize = arena.slots(nsrc + 1)
    cap = (ssize - 2 * GUARD - 256) // es
    layouts = [x for x in FOLD_LAYOUTS if not (x == "shift" and dtype == "longdouble")]
    grids = {}
    for layout in layouts:
        d, s, _, first = fold_pointers(layout, es, slots[0], slots[1:])
        assert shm.combine(op, dtype, d, s, cap - first) == 0
        grids[layout] = probe_grid(shm)
    shm.sync()
    gmax = max(grids.values())
    skip = (128 - LINE_OFF) // es
    ntot = sized_units(gmax) * V + V - 1 + skip + 1
    assert ntot <= cap, f"the arena's slots hold {cap} elements, the case needs {ntot}"
    rng = np.random.default_rng(9000 + 17 * nsrc + len(op) + es)
    srcs = [inputs(rng, op, dtype, ntot) for _ in range(nsrc)]
    planted = dtype in ("float", "double")
    if planted:
        plant_nans(rng, dtype, srcs, rule_units(gmax) * V + 2 * skip + 2)
    for slot, x in zip(slots[1:], srcs):
        arena.upload(slot, LINE_OFF, x)
    nan_in = np.logical_or.reduce([has_nan(x) for x in srcs]) if planted else None
    return {"slots": slots, "grids": grids, "want": oracle.reduce_pe(op, dtype, srcs, 0), "planted": planted,
            "nan_in": nan_in}


@pytest.mark.parametrize("layout", FOLD_LAYOUTS)
@pytest.mark.parametrize("op,dtype,nsrc", FOLD_CASES)
def test_fold_past_one_pass(shm, arena, op, dtype, nsrc, layout):
    if layout == "shift" and dtype == "longdouble":
        return   # long double has no shifted kernel: off the target's phase it runs element-wise (below)
    es, V = elem(dtype)
    st = prepared(("fold", op, dtype, nsrc), lambda: prepare_fold(shm, arena, op, dtype, nsrc))
    d, s, doff, first = fold_pointers(layout, es, st["slots"][0], st["slots"][1:])
    n = sized_units(st["grids"][layout]) * V + V - 1
    peeled = 0 if V == 1 else ((128 - doff) % 128) // es
    arena.poison(st["slots"][0], doff, n * es)
    assert shm.combine(op, dtype, d, s, n) == 0
    shm.sync()
    what = f"fold {op}/{dtype} x{nsrc} {layout}"
    gx = check_rule(shm, (n - peeled) // V, what, "combine_vec")
    assert ("true>" in kernel_name(shm).split("(")[0]) == (layout == "shift"), kernel_name(shm)
    want = st["want"][first:first + n]
    if st["planted"]:
        late = rule_units(gx) * V + peeled
        assert int(st["nan_in"][first + late:first + n].sum()) >= 20, "too few NaN operands on the late passes"
    got = arena.read(st["slots"][0], doff, n * es, what).view(oracle.NP[dtype])
    assert_match(got, want, op, dtype, ctx=what, strict=st["planted"])


# ---------------------------------------------------------------------------
# the every-member fold, mi355_combine_orders
# ---------------------------------------------------------------------------
ORDERS_CASES = [("sum", "double", 8), ("min", "float", 8), ("max", "double", 3), ("prod", "complexd", 3),
                ("sum", "complexd", 5), ("xor", "short", 2)]
# all: every output written. skip_inplace: member 1 skipped, another member's
# output its own source. shift: outputs one element on against the sources
# (complex double, whose elements fill a vector: sources 8 bytes on instead).
ORDERS_LAYOUTS = ["all", "skip_inplace", "shift"]


def orders_offsets(layout, es):
    """(outputs' byte offset, sources' byte offset) from the line"""
    if layout != "shift":
        return 0, 0
    return (0, 8) if es == 16 else (es, 0)


def orders_sources(arena, st, soff):
    """the sources on the device at byte offset soff, whole (an in-place output overwrote one)"""
    for k, (slot, x) in enumerate(zip(st["sslots"], st["srcs"])):
        if st["soff"] != soff or st["dirty"] == k:
            arena.upload(slot, soff, x)
    st["soff"], st["dirty"] = soff, None


def prepare_orders(shm, arena, op, dtype, nsrc):
    es, V = elem(dtype)
    slots, ssize = arena.slots(2 * nsrc)
    sslots, dslots = slots[:nsrc], slots[nsrc:]
    cap = (ssize - 2 * GUARD - 256) // es
    grids = {}
    for layout in ORDERS_LAYOUTS:
        doff, soff = orders_offsets(layout, es)
        dp = [d + GUARD + doff for d in dslots]
        if layout == "skip_inplace":
            dp[1], dp[0 if nsrc == 2 else nsrc - 1] = None, sslots[0 if nsrc == 2 else nsrc - 1] + GUARD
        assert shm.combine_orders(op, dtype, dp, [s + GUARD + soff for s in sslots], cap) == 0
        grids[layout] = probe_grid(shm)
    shm.sync()
    gmax, gmin = max(grids.values()), min(grids.values())
    ntot = sized_units(gmax) * V + V - 1
    assert ntot <= cap, f"the arena's slots hold {cap} elements, the case needs {ntot}"
    rng = np.random.default_rng(9500 + 17 * nsrc + len(op) + es)
    planted = False
    if op in ("min", "max"):
        srcs = sparse_minmax(rng, dtype, ntot, nsrc, 9 * LANES * gmin * V)
    else:
        srcs = [inputs(rng, op, dtype, ntot) for _ in range(nsrc)]
        planted = dtype in ("float", "double")
        if planted:
            plant_nans(rng, dtype, srcs, rule_units(gmax) * V + 128)
    st = {"sslots": sslots, "dslots": dslots, "srcs": srcs, "grids": grids, "soff": None, "dirty": None,
          "want": oracle.reduce_all(op, dtype, srcs), "planted": planted or op in ("min", "max")}
    return st


@pytest.mark.parametrize("layout", ORDERS_LAYOUTS)
@pytest.mark.parametrize("op,dtype,nsrc", ORDERS_CASES)
def test_every_member_fold_past_one_pass(shm, arena, op, dtype, nsrc, layout):
    es, V = elem(dtype)
    st = prepared(("orders", op, dtype, nsrc), lambda: prepare_orders(shm, arena, op, dtype, nsrc))
    doff, soff = orders_offsets(layout, es)
    orders_sources(arena, st, soff)
    n = sized_units(st["grids"][layout]) * V + V - 1
    skipped, inplace = (1, 0 if nsrc == 2 else nsrc - 1) if layout == "skip_inplace" else (None, None)
    # (slot, offset in the slot) of every output
    outs = [None if q == skipped else (st["sslots"][q], soff) if q == inplace else (st["dslots"][q], doff)
            for q in range(nsrc)]
    for q, o in enumerate(outs):
        if o is not None and q != inplace:
            arena.poison(o[0], o[1], n * es)
    dp = [None if o is None else o[0] + GUARD + o[1] for o in outs]
    assert shm.combine_orders(op, dtype, dp, [s + GUARD + soff for s in st["sslots"]], n) == 0
    shm.sync()
    if inplace is not None:
        st["dirty"] = inplace
    what = f"every-member {op}/{dtype} x{nsrc} {layout}"
    peeled = 0 if V == 1 else ((128 - doff) % 128) // es
    check_rule(shm, (n - peeled) // V, what, "combine_orders_vec")
    flags = kernel_name(shm).split("(")[0].rstrip(">").split(", ")[-2:]   # ALL, SHIFT
    assert flags == [str(layout != "skip_inplace").lower(), str(layout == "shift").lower()], kernel_name(shm)
    for q, o in enumerate(outs):
        if o is None:
            continue
        got = arena.read(o[0], o[1], n * es, f"{what} member {q}").view(oracle.NP[dtype])
        assert_match(got, st["want"][q][:n], op, dtype, ctx=f"{what} member {q}", strict=st["planted"])


# ---------------------------------------------------------------------------
# the element-wise fallbacks, combine_scalar / combine_orders_scalar
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("api", ["combine", "combine_orders"])
@pytest.mark.parametrize("dtype", ["complexd", "longdouble"])
def test_element_wise_fallback_past_one_pass(shm, arena, dtype, api):
    """16-byte elements the vector kernels cannot take. complex double: the
    target (and the sources) 8 bytes off 16. long double: mi355_combine with
    the sources 8 bytes off the target's phase; mi355_combine_orders with its
    outputs at different phases (a 16-byte element has no other phase 16 bytes
    on). units: elements."""
    nsrc, es, op = 3, 16, "sum"
    nout = 1 if api == "combine" else nsrc
    slots, ssize = arena.slots(nsrc + nout)
    sslots, dslots = slots[:nsrc], slots[nsrc:]
    cap = (ssize - 2 * GUARD - 256) // es
    if dtype == "complexd":
        soff, doffs = 8, [8] * nout
    elif api == "combine":
        soff, doffs = 8, [0]
    else:
        soff, doffs = 0, [8 * (q % 2) for q in range(nout)]
    sp = [s + GUARD + soff for s in sslots]
    dp = [d + GUARD + o for d, o in zip(dslots, doffs)]

    def launch(n):
        rc = shm.combine(op, dtype, dp[0], sp, n) if api == "combine" else shm.combine_orders(op, dtype, dp, sp, n)
        assert rc == 0, rc

    launch(cap)
    n = sized_units(probe_grid(shm))
    shm.sync()
    assert n <= cap
    rng = np.random.default_rng(9700 + len(dtype) + len(api))
    srcs = [inputs(rng, op, dtype, n) for _ in range(nsrc)]
    for slot, x in zip(sslots, srcs):
        arena.upload(slot, soff, x)
    for d, o in zip(dslots, doffs):
        arena.poison(d, o, n * es)
    launch(n)
    shm.sync()
    what = f"element-wise {api} {op}/{dtype} x{nsrc}"
    check_rule(shm, n, what, "combine_scalar" if api == "combine" else "combine_orders_scalar")
    for q, (d, o) in enumerate(zip(dslots, doffs)):
        got = arena.read(d, o, n * es, f"{what} member {q}").view(oracle.NP[dtype])
        assert_match(got, oracle.reduce_pe(op, dtype, srcs, q), op, dtype, ctx=f"{what} member {q}")


# ---------------------------------------------------------------------------
# mi355_nan_patch_copy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["line", "head48", "shift"])
@pytest.mark.parametrize("dtype", ["float", "double"])
def test_nan_patch_copy_past_one_pass(shm, arena, dtype, layout):
    """dst[i] = isnan(own[i]) ? quiet(own[i]) : peer[i] with the NaN word
    absent, clear (a plain copy of peer) and set; dst and peer on their line,
    48 bytes off it, or on it with own one element on (read unaligned). own
    holds NaNs in every pass."""
    es, V = elem(dtype)
    ut = np.uint32 if es == 4 else np.uint64
    quiet = ut(1 << 22) if es == 4 else ut(1 << 51)
    (dslot, pslot, oslot, wslot), ssize = arena.slots(4)
    cap = (ssize - 2 * GUARD - 256) // es
    doff = LINE_OFF if layout == "head48" else 0
    ooff = doff + (es if layout == "shift" else 0)
    d, pp, po = dslot + GUARD + doff, pslot + GUARD + doff, oslot + GUARD + ooff
    call = shm.lib.mi355_nan_patch_copy
    assert call(DTYPES.index(dtype), d, pp, po, cap, None, None) == 0
    n = sized_units(probe_grid(shm)) * V + V - 1
    shm.sync()
    assert n <= cap
    rng = np.random.default_rng(9800 + es + len(layout))
    peer, own = inputs(rng, "sum", dtype, n), inputs(rng, "sum", dtype, n)
    plant_nans(rng, dtype, [own], n // 2)
    peeled = ((128 - doff) % 128) // es
    step = DEEPEST_UNROLL * LANES * V   # elements of one block's pass: a NaN in each
    own[peeled + np.arange(0, n - peeled, step)] = np.nan
    arena.upload(pslot, doff, peer)
    arena.upload(oslot, ooff, own)
    shm.put(wslot, np.array([0, 0, 1, 0], np.uint64))
    words = {None: None, 0: wslot, 1: wslot + 16}
    pb, ob = peer.view(ut), own.view(ut)
    for flag in (None, 0, 1):
        arena.poison(dslot, doff, n * es)
        assert call(DTYPES.index(dtype), d, pp, po, n, words[flag], None) == 0
        shm.sync()
        what = f"nan_patch_copy {dtype} {layout} flag {flag}"
        check_rule(shm, (n - peeled) // V, what, "nan_patch_copy")
        assert kernel_name(shm).split("(")[0].endswith(f"{'true' if layout == 'shift' else 'false'}>")
        got = arena.read(dslot, doff, n * es, what).view(ut)
        want = pb if flag == 0 else np.where(np.isnan(own), ob | quiet, pb)
        assert (got == want).all(), (what, int(np.argmax(got != want)))


# ---------------------------------------------------------------------------
# mi355_copy_segments, several segments in one launch
# ---------------------------------------------------------------------------
# (target offset, source offset) from a 128-byte line, taken in turn
COALIGNED = [(0, 0), (48, 48), (3, 3), (16, 16), (72, 8)]
MIXED = [(0, 8), (48, 3), (0, 0), (16, 16), (5, 30), (64, 1), (8, 0)]


@pytest.mark.parametrize("longest", ["first", "last"])
@pytest.mark.parametrize("phases", ["coaligned", "mixed"])
@pytest.mark.parametrize("nseg", [64, 7])
def test_copy_segments_past_one_pass(shm, arena, nseg, phases, longest):
    """nseg segments of 0.3, 1, 2.6 and 9.1 grid passes (+ 0-15 odd bytes) in
    one launch, whose grid is sized by the longest: blocks of the shorter
    segments run out of work passes earlier. coaligned: every source at its
    target's 16-byte phase (copy_segments); mixed: some at another one, so
    copy_segments_shift carries the launch, targets on and off their line.
    Every target whole, with the bytes around it."""
    offs = COALIGNED if phases == "coaligned" else MIXED
    half = ARENA_BYTES // 2
    pitch = (half // nseg) & ~4095
    sbase, dbase = arena.base, arena.base + half

    def segment(i):
        doff, soff = offs[i % len(offs)]
        return dbase + i * pitch + GUARD + doff, sbase + i * pitch + GUARD + soff

    def launch(nbytes):
        ptrs = [segment(i) for i in range(nseg)]
        rc = shm.lib.mi355_copy_segments((ctypes.c_void_p * nseg)(*[p[0] for p in ptrs]),
                                         (ctypes.c_void_p * nseg)(*[p[1] for p in ptrs]),
                                         (ctypes.c_size_t * nseg)(*nbytes), nseg, None)
        assert rc == 0, rc

    launch([pitch - 2 * GUARD - 256] * nseg)
    gx = probe_grid(shm)
    shm.sync()
    pass_bytes = DEEPEST_UNROLL * LANES * gx * 16
    rng = np.random.default_rng(9900 + nseg + len(phases) + len(longest))
    fracs = [float(f) for f in rng.choice([0.3, 1.0, 2.6], nseg)]
    fracs[0 if longest == "first" else nseg - 1] = 9.1
    nbytes = [int(f * pass_bytes) + int(rng.integers(0, 16)) for f in fracs]
    assert max(nbytes) <= pitch - 2 * GUARD - 256, (max(nbytes), pitch)
    span = (nseg - 1) * pitch + GUARD + 128 + max(nbytes) + GUARD
    assert span <= half
    src = rng.integers(0, 256, span, dtype=np.uint8)
    want = np.full(span, SENT, np.uint8)
    for i, nb in enumerate(nbytes):
        d, s = segment(i)
        want[d - dbase:d - dbase + nb] = src[s - sbase:s - sbase + nb]
    shm.put(sbase, src)
    shm.put(dbase, arena.sentinel(span))
    launch(nbytes)
    shm.sync()
    what = f"copy_segments x{nseg} {phases}, longest {longest}"
    check_rule(shm, (max(nbytes) - 128) // 16, what, "copy_segments_shift" if phases == "mixed" else "copy_segments<")
    assert shm.last_launch_grid()[1] == nseg
    got = shm.get(dbase, span, np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{what}: {bad.size} bytes differ, first at {int(bad[0])} (segment {int(bad[0]) // pitch}, "
                           f"byte {int(bad[0]) % pitch - GUARD} of its slot)")
