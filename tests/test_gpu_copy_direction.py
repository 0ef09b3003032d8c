"""GPU: the single-segment copy's sweep direction (combine.hip copy_segments /
copy_segments_shift, mi355_copy_direction_next_launch).

The vector loop takes its grid passes first to last (ascending) or last to
first (descending); the library alternates between launches, a test pins the
next launch. Whatever the direction, every byte of the target equals the
source and nothing outside the target is written. On a 256-CU grid one block
pass is 16 KiB and one grid pass 4 MiB: the sizes sit below one vector, at one
block pass, at one grid pass (a descending loop's only pass), just under and
over it (the partial last pass some lanes have no share of), and at two and
three passes with a ragged tail.
"""
import ctypes

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SIZES = [1, 15, 16, 4095, 16384, 16384 + 16, 4 * MIB - 16, 4 * MIB, 4 * MIB + 16, 8 * MIB + 4096 + 24, 12 * MIB + 1]
# target offset from its 128-byte line; the source stays on its line:
# +0 aligned, +16 the line peel, +8 the shifted kernel
OFFSETS = [0, 16, 8]
GUARD = 256
MAXB = max(SIZES)


@pytest.fixture(scope="module")
def bufs(shm):
    """(source bytes on the host, source on the device, target buffer, its poison)"""
    x = np.random.default_rng(29).integers(0, 256, MAXB, dtype=np.uint8)
    poison = np.full(GUARD + max(OFFSETS) + MAXB + GUARD, 0xA5, dtype=np.uint8)
    s = shm.malloc_device(MAXB)
    d = shm.malloc_device(poison.nbytes)
    assert s % 128 == 0 and d % 128 == 0
    shm.put(s, x)
    yield x, s, d, poison
    shm.free_device(d)
    shm.free_device(s)


def _copy(shm, dst, src, nb, pin):
    if pin:
        shm.lib.mi355_copy_direction_next_launch(pin)
    rc = shm.lib.mi355_copy_segments((ctypes.c_void_p * 1)(dst), (ctypes.c_void_p * 1)(src),
                                     (ctypes.c_size_t * 1)(nb), 1, None)
    assert rc == 0, rc
    shm.sync()


@pytest.mark.parametrize("nb", SIZES)
def test_every_byte_lands_in_both_directions(shm, bufs, nb):
    x, s, d, poison = bufs
    span = GUARD + max(OFFSETS) + nb + GUARD
    for off in OFFSETS:
        tgt = d + GUARD + off
        # pinned ascending, pinned descending, four launches as the library alternates them
        for pin in (1, -1, 0, 0, 0, 0):
            shm.put(d, poison[:span])
            _copy(shm, tgt, s, nb, pin)
            got = shm.get(d, span, np.uint8)
            lo, hi = GUARD + off, GUARD + off + nb
            body = got[lo:hi]
            assert (body == x[:nb]).all(), (nb, off, pin, int(np.argmax(body != x[:nb])))
            assert (got[lo - GUARD:lo] == 0xA5).all(), ("guard below the target written", nb, off, pin)
            assert (got[hi:hi + GUARD] == 0xA5).all(), ("guard above the target written", nb, off, pin)


def test_request_is_consumed_and_cancelled(shm, bufs):
    """A pin holds for one launch: an error return cancels it, and a call that
    copies nothing consumes it, so the launches after it still alternate and
    still copy every byte."""
    x, s, d, poison = bufs
    nb = 4 * MIB + 16
    shm.lib.mi355_copy_direction_next_launch(-1)
    assert shm.lib.mi355_copy_segments(None, None, None, 65, None) != 0      # too many segments
    shm.lib.mi355_copy_direction_next_launch(-1)
    assert shm.lib.mi355_copy_segments(None, None, None, 0, None) == 0       # nothing to copy
    for _ in range(2):
        shm.put(d, poison[:nb])
        _copy(shm, d, s, nb, 0)
        assert (shm.get(d, nb, np.uint8) == x[:nb]).all()


def test_one_pe_sum_to_all_four_times_in_a_row(shm):
    """shmem_double_sum_to_all on a 1-PE set is the identity copy; consecutive
    calls sweep in alternating directions and each one gives the reference's
    result."""
    n = (MIB + 8) // 8
    src_h = np.random.default_rng(31).standard_normal(n) * np.exp2(np.random.default_rng(32).integers(-40, 40, n))
    want = oracle.reduce_pe("sum", "double", [src_h], 0)
    src, dst = shm.malloc_device(n * 8), shm.malloc_device(n * 8)
    try:
        shm.put(src, src_h)
        for call in range(4):
            shm.put(dst, np.full(n, np.nan))
            shm.to_all("sum", "double", dst, src, n, 0, 0, 1)
            shm.sync()
            got = shm.get(dst, n, "double")
            bad = int((got.view(np.uint64) != want.view(np.uint64)).sum())
            assert bad == 0, f"call {call}: {bad} of {n} elements differ from the oracle"
    finally:
        shm.free_device(dst)
        shm.free_device(src)


@pytest.mark.parametrize("up", [True, False], ids=["target_above_source", "target_below_source"])
def test_overlapping_target_through_scratch_twice(shm, up):
    """Overlapping target and source go through scratch chunk by chunk (two
    single-segment copies per chunk, each in its own direction); two calls in
    a row leave what two host memmoves leave."""
    n = (5 * MIB // 2 + 8) // 8          # several scratch chunks, a ragged last one
    shift = 4099                          # elements between target and source
    total = n + shift
    host = np.random.default_rng(37).integers(0, 1 << 63, total, dtype=np.int64).view(np.float64)
    buf = shm.malloc_device(total * 8)
    s_at, t_at = (0, shift) if up else (shift, 0)
    try:
        shm.put(buf, host)
        want = host.copy()
        for _ in range(2):
            shm.to_all("sum", "double", buf + t_at * 8, buf + s_at * 8, n, 0, 0, 1)
            want[t_at:t_at + n] = want[s_at:s_at + n].copy()
        shm.sync()
        got = shm.get(buf, total, "double")
        bad = int((got.view(np.uint64) != want.view(np.uint64)).sum())
        assert bad == 0, f"{bad} of {total} elements differ from the host memmove"
    finally:
        shm.free_device(buf)
