"""GPU: every branch of the element operators (tests/_op_paths.py's catalogue)
through every form of the streaming kernels, in this process through the C
ABI: mi355_combine, mi355_combine_orders and mi355_combine_prefix over the
directed tables, every element's value bits against the oracle (the model for
the 16-bit floats), the bytes around every output, every source and the slot
of a NULL output checked unchanged, the kernel that ran checked by its name.

The table is laid out three ways in one array (_op_paths.wave_layout): each
representative row alone in a wave of plain elements (the divergent redo),
filling a whole wave (the uniform case), and the whole table packed, with
V - 1 tail elements and, where the target is one element off its line, a head;
further small launches rotate the table through the head and the tail.

  forms    aligned; shift (target one element off the sources: unaligned
           source loads; 16-byte elements: sources 8 bytes off); elements
           (16-byte elements: every pointer 8 bytes off; smaller ones: outputs
           at two phases, which only the several-output calls can have)
  calls    combine with 2 and 3 sources (the third plain finite: the special
           result is carried one more step); combine_orders with 2 and 3
           sources, every member, and with one output skipped and one in
           place; combine_prefix with 3 sources, every output, in place, and
           the middle output NULL (float, double and long double min/max: no
           prefix calls)
"""
import numpy as np
import pytest

import _op_paths as P
import _scan_ref as S

pytestmark = pytest.mark.gpu

GUARD = 128     # keeps an "aligned" pointer on its 128-byte line: no head
SENT = 0xA5
CASES = [pair for pair in P.PAIRS if len(P.CATALOGUE[pair]) > 1]
KERNEL = {"fold": "combine", "orders": "combine_orders", "prefix": "combine_prefix"}


def forms(dtype):
    """(name, output j's byte offset, source byte offset, head elements, vector kernel, shifted loads)"""
    es = P.ES[dtype]
    out = [("aligned", lambda j: 0, 0, 0, True, False)]
    if es < 16:
        out.append(("shift", lambda j: es, 0, 128 // es - 1, True, True))
        out.append(("elements", lambda j: (j % 2) * es, 0, 0, False, False))
    else:
        if dtype != "longdouble":
            out.append(("shift", lambda j: 0, 8, 0, True, True))
        out.append(("elements", lambda j: 8, 8, 0, False, False))
    return out


@pytest.fixture(scope="module")
def arena(shm):
    nbytes = 8 << 20
    base = shm.malloc_device(nbytes)
    assert base and base % 256 == 0
    yield base, nbytes
    shm.sync()
    shm.free_device(base)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Laid:
    """one wave_layout and the expected results of the calls over it"""

    def __init__(self, op, dtype, body0, rotation=0, full=True):
        self.op, self.dtype = op, dtype
        self.arrays, where = P.wave_layout(op, dtype, body0, rotation, full)
        self.where = {at: (kind, row) for kind, row, at in where}
        self.names = P.paths(op, dtype, *P.table(op, dtype))
        self._want = {}

    def want(self, call, nsrc, j):
        key = (call, nsrc, j)
        if key not in self._want:
            srcs = self.arrays[:nsrc]
            if call == "orders":
                order = [srcs[j]] + [s for k, s in enumerate(srcs) if k != j]
                self._want[key] = S.prefix(self.op, self.dtype, order, nsrc - 1)
            else:
                self._want[key] = S.prefix(self.op, self.dtype, srcs, j)
        return self._want[key]

    def describe(self, i):
        kind, row = self.where.get(int(i), ("plain", None))
        return f"{kind} element" if row is None else f"{kind}, table row {row}: [{self.names[row]}]"


def run_call(shm, arena, laid, call, nsrc, form, outs=None, inplace=()):
    """one kernel-layer call over laid.arrays[:nsrc]; outs: the outputs set
    (orders, prefix; default all), inplace: outputs that are their own source"""
    op, dtype = laid.op, laid.dtype
    fname, dst_off, src_off, _, vec, shift = form
    es = P.ES[dtype]
    n = len(laid.arrays[0])
    base, cap = arena
    nout = 1 if call == "fold" else nsrc
    outs = set(range(nout)) if outs is None else set(outs)
    what = f"{dtype} {op} {call} nsrc {nsrc} n {n} {fname} outs {sorted(outs)} in place {sorted(inplace)}"
    stride = (2 * GUARD + 32 + n * es + 255) // 256 * 256
    assert (nsrc + nout) * stride <= cap, what
    image = np.full((nsrc + nout) * stride, SENT, dtype=np.uint8)
    src_at = [k * stride + GUARD + src_off for k in range(nsrc)]
    dst_at = [src_at[j] if j in inplace else (nsrc + j) * stride + GUARD + dst_off(j) for j in range(nout)]
    for k in range(nsrc):
        image[src_at[k]:src_at[k] + n * es] = as_bytes(laid.arrays[k])
    shm.put(base, image)
    sp = [base + a for a in src_at]
    dp = [base + dst_at[j] if j in outs else None for j in range(nout)]
    if call == "fold":
        rc = shm.combine(op, dtype, dp[0], sp, n)
    elif call == "orders":
        rc = shm.combine_orders(op, dtype, dp, sp, n)
    else:
        rc = shm.combine_prefix(op, dtype, dp, sp, n)
    assert rc == 0, (what, rc)
    name = shm.last_kernel_name()
    shm.sync()
    family = f"{KERNEL[call]}_{'vec' if vec else 'scalar'}<"
    assert f"::{family}" in name, (what, name)
    if vec:
        assert name.split(">(")[0].endswith("true" if shift else "false"), (what, name)
    got = shm.get(base, image.size, np.uint8)
    want_image = image.copy()
    for j in sorted(outs):
        g = got[dst_at[j]:dst_at[j] + n * es].view(S.NP[dtype])
        want = laid.want(call, nsrc, nsrc - 1 if call == "fold" else j)
        bad = S.differing(g, want, op, dtype)
        assert len(bad) == 0, (f"{what}: output {j}: {len(bad)} of {n} elements differ, first at {bad[0]} "
                               f"({laid.describe(bad[0])}); by kind "
                               f"{sorted({laid.where.get(int(i), ('plain', 0))[0] for i in bad})}: got "
                               f"{g[bad[0]:bad[0] + 1].tobytes().hex()} want "
                               f"{np.ascontiguousarray(want)[bad[0]:bad[0] + 1].tobytes().hex()}")
        # the value bits match: take a long double's padding from what came back
        want_image[dst_at[j]:dst_at[j] + n * es] = got[dst_at[j]:dst_at[j] + n * es]
    # guards, the sources that are no output, the slots of NULL outputs: as they were
    bad = np.nonzero(got != want_image)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} bytes outside the outputs changed, first at arena offset {bad[0]}"


def calls_of(op, dtype, fname):
    """(call, sources, outputs set or None, in place) run on the full layout in form `fname`"""
    out = [("fold", 2, None, ()), ("fold", 3, None, ()), ("orders", 2, None, ()), ("orders", 3, None, ())]
    if fname == "elements" and P.ES[dtype] < 16:
        out = out[2:]       # one output has one phase: the fold of a small type is never element-wise
    prefix = not (op in ("min", "max") and dtype in ("float", "double", "longdouble"))
    if prefix:
        out.append(("prefix", 3, None, ()))
    if fname == "aligned":
        out.append(("orders", 3, {0, 2}, (2,)))         # one output skipped, one in place
        out.append(("orders", 2, {0, 1}, (0,)))
        if prefix:
            out.append(("prefix", 3, None, (0, 1, 2)))   # in place
            out.append(("prefix", 3, {0, 2}, ()))        # the middle output NULL
            out.append(("prefix", 3, {0, 2}, (0, 2)))    # both
    return out


@pytest.mark.parametrize("op,dtype", CASES)
def test_every_branch_in_every_kernel_form(shm, arena, op, dtype):
    assert len(P.wave_layout(op, dtype)[0][0]) <= 21000
    for form in forms(dtype):
        laid = Laid(op, dtype, form[3])
        kinds = {k for k, _ in laid.where.values()}
        assert kinds >= {"sparse", "uniform", "packed"}, kinds
        for call, nsrc, outs, inplace in calls_of(op, dtype, form[0]):
            run_call(shm, arena, laid, call, nsrc, form, outs, inplace)


@pytest.mark.parametrize("op,dtype", [pair for pair in CASES if P.ES[pair[1]] < 16])
def test_every_row_in_a_head_or_a_tail(shm, arena, op, dtype):
    """the element-wise head and tail of the vector kernels: the table rotated
    through them, target one element off its line (head and V - 1 tail
    elements) -- small arrays, the packed table between head and tail"""
    form = [f for f in forms(dtype) if f[0] == "shift"][0]
    seen = set()
    prefix = not (op in ("min", "max") and dtype in ("float", "double"))
    for rot in range(P.rotations(op, dtype, form[3])):
        laid = Laid(op, dtype, form[3], rot, full=False)
        seen |= {row for kind, row in laid.where.values() if kind in ("head", "tail")}
        run_call(shm, arena, laid, "fold", 2 + rot % 2, form)
        run_call(shm, arena, laid, "orders", 3 - rot % 2, form)
        if prefix:
            run_call(shm, arena, laid, "prefix", 3, form)
    assert seen == set(range(len(P.table(op, dtype)[0])))
