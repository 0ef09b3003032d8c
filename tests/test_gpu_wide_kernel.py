"""GPU: mi355_combine_wide (the widening fold, csrc/wide.hip) called directly
in this process, every output bit for bit against tests/_wide_ref.py: both
types and both outputs at the sizes around a vector, 1 to 32 sources, every
source and target element phase against a 16-byte line (the vector form, the
unaligned-load form and the element form, asserted by the recorded kernel's
name), in place on the first and on a middle source, and a size past the first
full grid pass. The arrays sit between guard bytes in one allocation whose
whole image is compared: the output holds the model's bits and every other
byte -- guards and sources -- is what it was."""
import numpy as np
import pytest

import _wide_ref as W

pytestmark = pytest.mark.gpu

GUARD = 256           # bytes on both sides of every array
SENT = 0xA5
VEC, UNAL, ELEM = "mi355k::wide_fold_vec", "mi355k::wide_fold_unal", "mi355k::wide_fold_elem"
PAIRS = [(t, f) for t in W.TYPES for f in (False, True)]
PAIR_IDS = [f"{t}-{'float' if f else '16bit'}" for t, f in PAIRS]


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

    def image(self):
        return self.shm.get(self.base, self.total, np.uint8)

    def free(self):
        self.shm.free_device(self.base)


def expected_kernel(n, out_es, dst_phase, src_phases):
    """a lane's unit is one 16-byte store: 8 elements from a 16-byte load, or 4 floats from an 8-byte load"""
    per_lane = W.PER_LANE[out_es == 4]
    if (dst_phase * out_es) % 16 != 0 or n < per_lane:
        return ELEM
    return VEC if all((p * 2) % (2 * per_lane) == 0 for p in src_phases) else UNAL


def run_case(shm, dtype, out_float, n, nsrc, inplace=None, dst_phase=0, src_phases=None, seed=W.SEEDS[0],
             srcs=None):
    """Sources 0 .. nsrc-1 in arrays 0 .. nsrc-1, the output in array nsrc (or
    on source `inplace`). dst_phase / src_phases: pointer offsets in elements
    of the array's own type. Returns the kernel name."""
    out_es = 4 if out_float else 2
    src_phases = list(src_phases or [0] * nsrc)
    if inplace is not None:
        assert not out_float
        dst_phase = src_phases[inplace]
    srcs = srcs if srcs is not None else W.sources(dtype, *W.gpu_shape(nsrc, n), seed)
    c = Case(shm, [n * 2] * nsrc + [n * out_es])
    for j in range(nsrc):
        if n:
            shm.put(c.ptr(j, src_phases[j] * 2), srcs[j])
    d = nsrc if inplace is None else inplace
    before = c.image()
    rc = shm.combine_wide(dtype, "float" if out_float else dtype, c.ptr(d, dst_phase * out_es),
                          [c.ptr(j, src_phases[j] * 2) for j in range(nsrc)], n)
    assert rc == 0, rc
    shm.sync()
    name = shm.last_kernel_name() if n else ""
    after = c.image()
    want = W.result(dtype, out_float, srcs)
    image = before.copy()
    a = c.slots[d] + GUARD + dst_phase * out_es
    image[a:a + n * out_es] = want.view(np.uint8)
    ctx = (f"{dtype} -> {'float' if out_float else dtype} n {n} nsrc {nsrc} inplace {inplace} phases {dst_phase} "
           f"{src_phases} ({name})")
    if not (after == image).all():
        got = after[a:a + n * out_es].view(want.dtype)
        bad = np.flatnonzero(got != want)
        if len(bad):
            i = int(bad[0])
            raise AssertionError(f"{ctx}: {len(bad)} of {n} elements differ, first at {i}: got {int(got[i]):#x} want "
                                 f"{int(want[i]):#x} from {[hex(int(s[i])) for s in srcs]}")
        raise AssertionError(f"{ctx}: bytes outside the output were written (a source, a guard or past the end)")
    c.free()
    if n:
        assert expected_kernel(n, out_es, dst_phase, src_phases) in name, ctx
    return name


@pytest.mark.parametrize("dtype,out_float", PAIRS, ids=PAIR_IDS)
def test_source_counts_and_sizes_around_a_vector(shm, dtype, out_float):
    names = set()
    for k, nsrc in enumerate((1, 2, 3, 8, 9, 32)):
        for n in (1, 7, 8, 9, 257, 4099):
            name = run_case(shm, dtype, out_float, n, nsrc, seed=W.SEEDS[k % 2])
            names.update(form for form in (VEC, UNAL, ELEM) if form in name)
    assert names == {VEC, ELEM}, names       # less than a unit: the element form (run_case checks which case ran which)


@pytest.mark.parametrize("dtype,out_float", PAIRS, ids=PAIR_IDS)
def test_every_source_and_target_phase(shm, dtype, out_float):
    n, nsrc = 257, 3
    ran, want = {}, {}
    for t in range(8):
        for s in range(8):
            for phases in ((s, s, s), (0, s, (2 * s + 1) % 8)):
                name = run_case(shm, dtype, out_float, n, nsrc, dst_phase=t, src_phases=phases, seed=W.SEEDS[s % 2])
                for form in (VEC, UNAL, ELEM):
                    if form in name:
                        ran[form] = ran.get(form, 0) + 1
                form = expected_kernel(n, 4 if out_float else 2, t, phases)
                want[form] = want.get(form, 0) + 1
    # all three forms ran, and each case ran the one its phases call for (run_case)
    assert set(ran) == {VEC, UNAL, ELEM} and sum(ran.values()) == 128 and ran == want, (ran, want)
    aligned_targets = 2 if out_float else 1       # float phases 0 and 4 are 16-byte aligned
    assert ran[ELEM] == (8 - aligned_targets) * 16, ran


@pytest.mark.parametrize("dtype", W.TYPES)
def test_in_place_on_the_first_and_on_a_middle_source(shm, dtype):
    for inplace in (0, 2):
        for n in (1, 257, 4099):
            run_case(shm, dtype, False, n, 5, inplace=inplace, seed=W.SEEDS[inplace // 2])
        # the target (a source) aligned and another source off it; and the target itself off the phase
        run_case(shm, dtype, False, 4099, 5, inplace=inplace, src_phases=[0, 3, 0, 5, 0])
        run_case(shm, dtype, False, 4099, 5, inplace=inplace, src_phases=[3, 3, 3, 3, 3])


@pytest.mark.parametrize("dtype,out_float", PAIRS, ids=PAIR_IDS)
def test_the_second_grid_pass_and_its_tail(shm, dtype, out_float):
    """n = pass + 4099 from mi355_combine_wide_plan at this GPU's CU count: every
    lane of every block takes one unit, then a second pass of 4096 elements and
    3 tail elements remains"""
    cus = shm.device_cus()
    assert cus == W.GPU_CUS, "tests/_wide_ref.py asserts the input condition at the size this CU count gives"
    out = "float" if out_float else dtype
    grid, per_pass = shm.combine_wide_plan(1 << 40, out, cus)
    assert grid >= 1 and per_pass == grid * 256 * W.PER_LANE[out_float] == W.grid_pass(out_float)
    n = per_pass + W.PASS_EXTRA
    assert shm.combine_wide_plan(n, out, cus) == (grid, per_pass)
    assert VEC in run_case(shm, dtype, out_float, n, 3)
    assert shm.last_launch_grid() == (grid, 1)
    # the unaligned-load form takes the same grid
    assert UNAL in run_case(shm, dtype, out_float, n, 2, src_phases=[0, 1])
    assert shm.last_launch_grid() == (grid, 1)


def test_the_hand_written_rows_on_the_gpu(shm):
    """the rows of tests/test_wide_ref.py: 60000 + 60000 - 60000 in half, and
    a NaN through a one-source call, in every form"""
    h = lambda x: int(np.array([x], np.float16).view(np.uint16)[0])      # noqa: E731
    for n in (3, 257):
        srcs = [np.full(n, v, np.uint16) for v in (h(60000), h(60000), h(-60000))]
        assert (W.wsum("half", srcs) == h(60000)).all()
        run_case(shm, "half", False, n, 3, srcs=srcs)
        run_case(shm, "half", True, n, 3, srcs=srcs)
        for dtype in W.TYPES:
            nan = [np.full(n, W.INF[dtype] | 1, np.uint16)]
            assert (W.wsum(dtype, nan) == W.CANONICAL_NAN[dtype]).all()
            run_case(shm, dtype, False, n, 1, srcs=nan)
            run_case(shm, dtype, True, n, 1, srcs=nan)
            run_case(shm, dtype, False, n, 1, inplace=0, srcs=nan)
