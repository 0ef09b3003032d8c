"""GPU: mi355_combine_prefix (the scan collectives' kernel) through
Shmem.combine_prefix, in this process: every one of the 52 (op, type) pairs,
every output bit for bit against tests/_scan_ref.py, the bytes around every
output and every source checked unchanged.

  sources  1, 2, 3, 5, 8, and 9 and 17 (chained launches)
  sizes    0, 1, V - 1, V, V + 1, 257, 4099 elements, V = 16 / element size
  layouts  aligned; target one element off the sources (unaligned source
           loads); sources at mixed phases; outputs at mixed phases (element
           by element); in place (dsts[j] is srcs[j]); NULL outputs: the last,
           the first, and a sparse pattern (dsts[2] and dsts[6] of 8; beyond 8
           sources also the last one, which then carries the chain)
"""
import numpy as np
import pytest

import _scan_ref as S

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = 0xA5
NSRC = [1, 2, 3, 5, 8, 9, 17]
ES = {"short": 2, "int": 4, "long": 8, "longlong": 8, "float": 4, "double": 8, "longdouble": 16, "complexf": 8,
      "complexd": 16, "half": 2, "bfloat16": 2}
LANES = 256   # kBlock
U = 4         # the deepest unroll of combine_prefix_vec (prefix_kernels.h kPrefixMaxUnroll)


def sizes(es):
    v = 16 // es
    return sorted({0, 1, v - 1, v, v + 1, 257, 4099})


def layouts(nsrc, es):
    """(name, dst byte offset of j, src byte offset of k, the outputs set, in place)"""
    every = set(range(nsrc))
    out = [("aligned", lambda j: 0, lambda k: 0, every, False),
           ("target one element off", lambda j: es, lambda k: 0, every, False),
           ("sources at mixed phases", lambda j: 0, lambda k: (k * es) % 16 if es < 16 else (k % 2) * 8, every, False),
           ("outputs at mixed phases", lambda j: (j % 2) * es, lambda k: 0, every, False),
           ("in place", lambda j: 0, lambda k: 0, every, True),
           ("in place, one element off", lambda j: es, lambda k: es, every, True)]
    if nsrc >= 2:
        out.append(("last NULL", lambda j: 0, lambda k: 0, every - {nsrc - 1}, False))
        out.append(("first NULL", lambda j: 0, lambda k: es, every - {0}, False))
    if nsrc >= 8:
        sparse = {2, 6} | ({nsrc - 1} if nsrc > 8 else set())
        out.append(("sparse", lambda j: 0, lambda k: 0, sparse, False))
        out.append(("sparse in place", lambda j: 0, lambda k: 0, {2, 6}, True))
    return out


@pytest.fixture(scope="module")
def arena(shm):
    nbytes = 40 << 20
    base = shm.malloc_device(nbytes)
    assert base and base % 256 == 0
    yield base, nbytes
    shm.sync()
    shm.free_device(base)


_SOURCES = {}


def sources_for(op, dtype, n):
    key = (op, dtype, n)
    if key not in _SOURCES:
        _SOURCES[key] = S.sources(op, dtype, max(NSRC), n, 4000 + n)
    return _SOURCES[key]


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def run_case(shm, arena, op, dtype, nsrc, n, layout, prefixes):
    name, dst_off, src_off, outs, inplace = layout
    es = ES[dtype]
    what = f"{dtype} {op} nsrc {nsrc} n {n} {name}"
    base, cap = arena
    stride = (2 * GUARD + 32 + n * es + 255) // 256 * 256
    assert 2 * nsrc * stride <= cap
    srcs = sources_for(op, dtype, n)[:nsrc]
    image = np.full(2 * nsrc * stride, SENT, dtype=np.uint8)
    src_at = [k * stride + GUARD + src_off(k) for k in range(nsrc)]
    dst_at = [src_at[j] if inplace else (nsrc + j) * stride + GUARD + dst_off(j) for j in range(nsrc)]
    for k in range(nsrc):
        image[src_at[k]:src_at[k] + n * es] = as_bytes(srcs[k])
    shm.put(base, image)
    dsts = [base + dst_at[j] if j in outs else None for j in range(nsrc)]
    rc = shm.combine_prefix(op, dtype, dsts, [base + a for a in src_at], n)
    assert rc == 0, (what, rc)
    shm.sync()
    got = shm.get(base, image.size, np.uint8)
    want = image.copy()
    for j in sorted(outs):
        want[dst_at[j]:dst_at[j] + n * es] = as_bytes(prefixes[j])
    for j in sorted(outs):
        g = got[dst_at[j]:dst_at[j] + n * es].view(S.NP[dtype])
        bad = S.differing(g, prefixes[j], op, dtype)
        assert len(bad) == 0, (f"{what}: output {j}: {len(bad)} of {n} elements differ, first at {bad[0]}: got "
                               f"{g[bad[0]:bad[0] + 1].tobytes().hex()} want "
                               f"{np.ascontiguousarray(prefixes[j])[bad[0]:bad[0] + 1].tobytes().hex()}")
        # the value bits match: take the padding of a long double from what came back
        want[dst_at[j]:dst_at[j] + n * es] = got[dst_at[j]:dst_at[j] + n * es]
    # everything else -- guards, unaliased sources, the slots of NULL outputs -- is as it was
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} bytes outside the outputs changed, first at arena offset {bad[0]}"


@pytest.mark.parametrize("op,dtype", S.PAIRS)
def test_every_prefix_bit_for_bit(shm, arena, op, dtype):
    es = ES[dtype]
    for n in sizes(es):
        srcs = sources_for(op, dtype, n)
        prefixes = [S.prefix(op, dtype, srcs, j) for j in range(max(NSRC))]
        for nsrc in NSRC:
            for layout in layouts(nsrc, es):
                run_case(shm, arena, op, dtype, nsrc, n, layout, prefixes)
        _SOURCES.pop((op, dtype, n), None)


def test_prefix_zero_keeps_a_16_bit_nan_payload(shm, arena):
    """prefix 0 is the source's bits: a non-canonical NaN stays as it is there
    and is canonical from the first sum on"""
    base, _ = arena
    for dtype, nan, one, canon in (("half", 0x7D01, 0x3C00, 0x7E00), ("bfloat16", 0xFF81, 0x3F80, 0x7FC0)):
        a = np.full(64, nan, dtype=np.uint16)
        b = np.full(64, one, dtype=np.uint16)
        shm.put(base, a)
        shm.put(base + 4096, b)
        assert shm.combine_prefix("sum", dtype, [base + 8192, base + 12288], [base, base + 4096], 64) == 0
        shm.sync()
        assert (shm.get(base + 8192, 64, np.uint16) == nan).all()
        assert (shm.get(base + 12288, 64, np.uint16) == canon).all()


def test_rejected_arguments_launch_nothing(shm, arena):
    base, _ = arena
    srcs = [base + 4096 * k for k in range(17)]
    # beyond 8 sources a NULL output at a launch's end needs a later output that is no source's buffer
    dsts = [None] * 17
    dsts[16] = srcs[16]
    assert shm.combine_prefix("sum", "double", dsts, srcs, 8) == -1
    assert shm.combine_prefix("xor", "double", srcs[:2], srcs[:2], 8) == -2
    assert shm.combine_prefix("sum", "double", [None] * 3, srcs[:3], 8) == 0   # no output: nothing to do


# Beyond one grid pass ("Grid passes"). The x87 sum/prod and
# the float complex product launch uncapped grids (one pass whatever the size),
# so no size takes them past it: left out.
@pytest.mark.parametrize("op,dtype", [("sum", "double"), ("sum", "bfloat16"), ("max", "float")])
def test_beyond_one_grid_pass(shm, op, dtype):
    nsrc, es = 8, ES[dtype]
    v = 16 // es
    probe_vecs = LANES * U * 8 * shm.device_cus()      # past any capped grid's one pass
    slot = 40 << 20
    base = shm.malloc_device(2 * nsrc * slot)
    assert base
    try:
        ptrs = [base + k * slot for k in range(nsrc)]
        outs = [base + (nsrc + k) * slot for k in range(nsrc)]
        assert probe_vecs * 16 <= slot
        assert shm.combine_prefix(op, dtype, outs, ptrs, probe_vecs * v) == 0
        shm.sync()
        gx, _ = shm.last_launch_grid()
        assert gx > 0
        units = 9 * LANES * gx + LANES + 37
        n = units * v + (v - 1)
        assert units > 2 * U * LANES * gx and n * es + 2 * GUARD <= slot, (gx, n)
        srcs = S.sources(op, dtype, nsrc, n, 97)
        sent = np.full(GUARD, SENT, dtype=np.uint8)
        for k in range(nsrc):
            shm.put(ptrs[k], srcs[k])
            shm.put(outs[k] + n * es, sent)
        assert shm.combine_prefix(op, dtype, outs, ptrs, n) == 0
        shm.sync()
        assert shm.last_launch_grid()[0] == gx
        for j in range(nsrc):
            got = shm.get(outs[j], n, S.NP[dtype])
            bad = S.differing(got, S.prefix(op, dtype, srcs, j), op, dtype)
            assert len(bad) == 0, f"{dtype} {op} past one pass: output {j}: {len(bad)} differ, first at {bad[0]}"
            assert (shm.get(outs[j] + n * es, GUARD, np.uint8) == SENT).all(), f"output {j}: bytes above it written"
            assert (as_bytes(shm.get(ptrs[j], n, S.NP[dtype])) == as_bytes(srcs[j])).all(), f"source {j} changed"
    finally:
        shm.sync()
        shm.free_device(base)
