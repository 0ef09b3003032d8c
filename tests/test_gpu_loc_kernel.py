"""GPU: mi355_combine_loc (the value-and-location fold, csrc/loc.hip) called
directly in this process, every output pair bit for bit against
tests/_loc_ref.py: both operators and the eight types at the sizes around a
vector, 1 to 32 sources, explicit, implicit and mixed locations with a
non-zero loc_base, in place, pointers off the 16-byte phase (the element
form, asserted by the recorded kernel's name), one element past the first full
grid pass, and a 40-source fold as two chained calls. Targets are pre-filled
with a sentinel and read back with their guards."""
import numpy as np
import pytest

import _loc_ref as L

pytestmark = pytest.mark.gpu

GUARD = 256           # bytes on both sides of every array
SENT = 0xA5
VEC, ELEM = "loc_fold_vec", "loc_fold_elem"


def up(x, a=256):
    return (x + a - 1) // a * a


class Case:
    """One call's device arrays, carved from one allocation: array k of
    `nbytes` bytes lies at a 256-byte aligned slot plus GUARD plus its offset."""

    def __init__(self, shm, sizes):
        self.shm = shm
        self.slots, total = [], 0
        for nbytes in sizes:
            self.slots.append(total)
            total += up(GUARD + 64 + nbytes + GUARD)
        self.total = max(total, 256)
        self.base = shm.malloc_device(self.total)
        assert self.base and self.base % 256 == 0
        shm.put(self.base, np.full(self.total, SENT, np.uint8))

    def ptr(self, k, off_bytes=0):
        return self.base + self.slots[k] + GUARD + off_bytes

    def put(self, k, arr, off_bytes=0):
        if arr.nbytes:
            self.shm.put(self.ptr(k, off_bytes), arr)

    def image(self):
        return self.shm.get(self.base, self.total, np.uint8)

    def free(self):
        self.shm.free_device(self.base)


def run_case(shm, op, dtype, n, nsrc, locmode="explicit", inplace=None, val_off=None, loc_off=None, loc_base=0,
             seed=1, counts=None, expect=None):
    """Sources 0 .. nsrc-1 in arrays 2j (values) and 2j+1 (locations), the
    output in arrays 2nsrc and 2nsrc+1 (or on source `inplace`). val_off /
    loc_off: {array index: elements} pointer offsets. Returns the kernel name."""
    st = np.dtype(L.STORE[dtype])
    es = st.itemsize
    vals, locs = L.inputs(dtype, nsrc, n, seed)
    explicit = [locmode == "explicit" or (locmode == "mixed" and j % 2 == 0) for j in range(nsrc)]
    c = Case(shm, [n * es, n * 8] * (nsrc + 1))
    voff = lambda k: (val_off or {}).get(k, 0) * es     # noqa: E731
    loff = lambda k: (loc_off or {}).get(k, 0) * 8      # noqa: E731
    for j in range(nsrc):
        c.put(2 * j, vals[j], voff(2 * j))
        c.put(2 * j + 1, locs[j], loff(2 * j + 1))
    dv, dl = (2 * nsrc, 2 * nsrc + 1) if inplace is None else (2 * inplace, 2 * inplace + 1)
    before = c.image()
    src_vals = [c.ptr(2 * j, voff(2 * j)) for j in range(nsrc)]
    src_locs = None if locmode == "implicit" else [c.ptr(2 * j + 1, loff(2 * j + 1)) if explicit[j] else None
                                                    for j in range(nsrc)]
    rc = shm.combine_loc(op, dtype, c.ptr(dv, voff(dv)), c.ptr(dl, loff(dl)), src_vals, src_locs, loc_base, n)
    assert rc == 0, rc
    shm.sync()
    name = shm.last_kernel_name() if n else ""
    after = c.image()
    want_v, want_l = L.fold(op, dtype, vals, [locs[j] if explicit[j] else None for j in range(nsrc)], loc_base,
                            counts=counts)
    # the whole image: the two outputs hold the model's pair, every other byte is what it was
    image = before.copy()
    a = c.slots[dv] + GUARD + voff(dv)
    image[a:a + n * es] = want_v.view(np.uint8)
    b = c.slots[dl] + GUARD + loff(dl)
    image[b:b + n * 8] = want_l.view(np.uint8)
    ctx = f"{dtype} {op} n {n} nsrc {nsrc} {locmode} inplace {inplace} offsets {val_off} {loc_off} ({name})"
    if not (after == image).all():
        got_v = after[a:a + n * es].view(st)
        got_l = after[b:b + n * 8].view(np.int64)
        bad = np.flatnonzero((got_v != want_v) | (got_l != want_l))
        if len(bad):
            i = int(bad[0])
            raise AssertionError(f"{ctx}: {len(bad)} of {n} pairs differ, first at {i}: got ({got_v[i]:#x}, {got_l[i]}) "
                                 f"want ({want_v[i]:#x}, {want_l[i]})")
        raise AssertionError(f"{ctx}: bytes outside the outputs were written (a source, a guard or past the end)")
    c.free()
    if n and expect is not None:
        assert expect in name, f"{ctx}: expected {expect}"
    return name


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("op", L.OPS)
def test_both_operators_every_type_around_a_vector(shm, op, dtype):
    V = 16 // np.dtype(L.STORE[dtype]).itemsize
    counts = {}
    for n in (0, 1, V - 1, 257, 40000):
        run_case(shm, op, dtype, n, 3, seed=100 + n, counts=counts if n == 40000 else None, expect=VEC)
    for rule in L.rules_of(dtype):     # a condition on the inputs: every rule of the model fired
        assert counts.get(rule, 0) > 0, (rule, counts)


@pytest.mark.parametrize("nsrc", [1, 2, 8, 9, 32])
def test_source_counts_and_location_forms(shm, nsrc):
    for k, (op, dtype) in enumerate((("max", "float"), ("min", "short"), ("max", "double"), ("min", "bfloat16"))):
        for locmode, base in (("explicit", 0), ("implicit", 11), ("mixed", -5)):
            for n in (259, 4099):
                run_case(shm, op, dtype, n, nsrc, locmode, loc_base=base, seed=200 + 10 * k + nsrc, expect=VEC)


def test_in_place_on_the_first_and_on_a_middle_source(shm):
    for op, dtype in (("max", "float"), ("min", "long"), ("max", "half")):
        for inplace in (0, 2):
            for n in (1, 261, 40000):
                run_case(shm, op, dtype, n, 5, "explicit", inplace=inplace, seed=300 + n, expect=VEC)
            run_case(shm, op, dtype, 1031, 5, "mixed", inplace=inplace, loc_base=3, seed=310, expect=VEC)


def test_pointers_off_the_vector_phase_take_the_element_form(shm):
    nsrc = 3
    dst_v, dst_l = 2 * nsrc, 2 * nsrc + 1
    for op, dtype in (("max", "float"), ("min", "short"), ("max", "bfloat16"), ("min", "int")):
        es = np.dtype(L.STORE[dtype]).itemsize
        per16 = 16 // es
        for n in (1, 263, 5000):
            # one value pointer, one location pointer, the outputs, and everything at once
            for off in (1, 2, 3):
                if off % per16 == 0:
                    continue
                run_case(shm, op, dtype, n, nsrc, val_off={2: off}, seed=400 + off, expect=ELEM)
                run_case(shm, op, dtype, n, nsrc, val_off={dst_v: off}, seed=410 + off, expect=ELEM)
            run_case(shm, op, dtype, n, nsrc, loc_off={3: 1}, seed=420, expect=ELEM)
            run_case(shm, op, dtype, n, nsrc, loc_off={dst_l: 1}, seed=421, expect=ELEM)
            run_case(shm, op, dtype, n, nsrc, "mixed", loc_base=9, val_off={0: 1, 2: 2, 4: 3, dst_v: 1},
                     loc_off={1: 1, 3: 1, 5: 1, dst_l: 1}, seed=422, expect=ELEM)
            # an offset location array that the call does not read (implicit) does not matter
            run_case(shm, op, dtype, n, nsrc, "implicit", loc_off={1: 1, 3: 1}, seed=423, expect=VEC)
    # double: 8-byte elements have one off-phase position
    run_case(shm, "max", "double", 263, nsrc, val_off={0: 1}, seed=430, expect=ELEM)
    run_case(shm, "min", "double", 263, nsrc, val_off={0: 2}, seed=431, expect=VEC)


@pytest.mark.parametrize("dtype", ["double", "bfloat16"])
def test_one_element_past_the_first_full_grid_pass(shm, dtype):
    """n from the grid the library reports for a saturating launch: every lane
    of every block takes one vector and exactly one more element remains"""
    es = np.dtype(L.STORE[dtype]).itemsize
    V = 16 // es
    cus = shm.device_cus()
    big = cus * 8 * 256 * V * 2
    c = Case(shm, [big * es, big * 8] * 2)
    rc = shm.combine_loc("max", dtype, c.ptr(2), c.ptr(3), [c.ptr(0)], [c.ptr(1)], 0, big)
    assert rc == 0
    shm.sync()
    gx, gy = shm.last_launch_grid()
    c.free()
    assert gy == 1 and gx == cus * 8, (gx, gy, cus)
    n = gx * 256 * V + 1
    assert VEC in run_case(shm, "max", dtype, n, 2, seed=500)
    assert shm.last_launch_grid() == (gx, 1)
    assert ELEM in run_case(shm, "min", dtype, gx * 256 + 1, 2, val_off={0: 1} if es > 2 else {0: 3}, seed=501)
    assert shm.last_launch_grid() == (gx, 1)


def test_forty_sources_as_two_chained_calls(shm):
    """loc_plan.h's chain by hand: sources 0 .. 31, then the output as entry 0
    with its location array and sources 32 .. 39 implicit with loc_base + 31"""
    for op, dtype, locmode in (("max", "float", "implicit"), ("min", "bfloat16", "mixed"), ("max", "int", "explicit")):
        n, nsrc, base = 3001, 40, 17
        st = np.dtype(L.STORE[dtype])
        vals, locs = L.inputs(dtype, nsrc, n, seed=600)
        explicit = [locmode == "explicit" or (locmode == "mixed" and j % 3 == 0) for j in range(nsrc)]
        c = Case(shm, [n * st.itemsize, n * 8] * (nsrc + 1))
        for j in range(nsrc):
            c.put(2 * j, vals[j])
            c.put(2 * j + 1, locs[j])
        sv = [c.ptr(2 * j) for j in range(nsrc)]
        sl = [c.ptr(2 * j + 1) if explicit[j] else None for j in range(nsrc)]
        dv, dl = c.ptr(2 * nsrc), c.ptr(2 * nsrc + 1)
        assert shm.combine_loc(op, dtype, dv, dl, sv[:32], sl[:32], base, n) == 0
        assert shm.combine_loc(op, dtype, dv, dl, [dv] + sv[32:], [dl] + sl[32:], base + 31, n) == 0
        shm.sync()
        want_v, want_l = L.fold(op, dtype, vals, [locs[j] if explicit[j] else None for j in range(nsrc)], base)
        got_v = shm.get(dv, n, st)
        got_l = shm.get(dl, n, np.int64)
        c.free()
        assert (got_v == want_v).all() and (got_l == want_l).all(), (op, dtype, locmode)
