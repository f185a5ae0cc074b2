"""jpegx_probe_sizes_set_n beyond one turn per workgroup, against the road it stands for (tests/probe_set_device.py).  Every
comparison is exact.

Below 8193 turns every turn is the last of its run, and three things never happen: the plane comparison of `leave` decides,
the sums are cleared for a turn that follows, row 0 is carried into the next turn.  The strips here are just large enough for
runs of 2 and 3 turns, over planes of UNEQUAL block counts (tests/probe_set_schedule.py: SCALE), so that every one of those
happens where the plane of a block comes from the table:

   N  blocks/turn  blocks per plane, cycled                          planes   turns  run
   2      64       225 1 1 383 64 65 7 130 1 200 3 449                 4125    8209   2
   4      16       63 1 100 5 37 150 16 17 1 81                        5570   16397   3
  17       1       1 5 2 1 7 3 4                                       2496    8197   2

tests/test_probe_set_schedule.py holds these shapes against the host model without a device: the runs, the events at plane
ends off every turn boundary, and that the model's totals change under each of the two defects."""
import numpy as np
import pytest

import probe_set_device as psd
import probe_set_schedule as pss

pytestmark = pytest.mark.gpu

DIVISORS = [1.0, 3.0, -40.0, 64.0]                   # a multiply (1, 64), two true divisions, a negative one
BAD_DIVISORS = [1.0, 1000.0]
BAD_DC = 20000.3                                     # the DC of the one bad block: beyond 16383 under 1, 20 under 1000


def _content(n, nblk):
    """Noise blocks of unlike amplitudes with every fifth block flat zero, within the 15 bits of a code under divisor 1."""
    rng = np.random.default_rng(n)
    amp = min(128.0, 12000.0 / (n * n)) * rng.choice([1.0, 0.5, 0.1, 0.02], nblk)
    amp[::5] = 0.0
    return (np.round(rng.uniform(-1.0, 1.0, (nblk, n, n)) * amp[:, None, None], 2)).reshape(nblk * n, n)


@pytest.fixture(scope="module")
def strips(gpu):
    cache = {}

    def get(n):
        if n not in cache:
            s = pss.scale_schedule(n)
            strip = _content(n, s.nblk)
            strip.setflags(write=False)
            cache[n] = (s, strip, psd.SetStrip(gpu, strip, psd.sizes_for(pss.scale_counts(n), n), 1, n))
            assert cache[n][2].first.tolist() == s.starts
        return cache[n]
    yield get
    for _, _, d in cache.values():
        d.free()


@pytest.mark.parametrize("n", sorted(pss.SCALE))
def test_runs_of_two_and_three_turns(strips, n):
    s, _, d = strips(n)
    assert s.run == pss.SCALE[n][2] and s.nturns > 8192
    got = d.check("divide", DIVISORS)
    assert (got >= d.counts()[:, None].astype(np.uint64)).all()
    d.check("divide", DIVISORS[1:2])
    # a sub-range that starts inside what was a carried run of the whole set: its own turns, its own rows
    d.check("divide", DIVISORS[:2], 3, s.nplanes - 5)


def test_thirty_two_candidates_over_runs_of_three_turns(strips):
    from test_gpu_probe_set_kernel_n import MANY
    _, _, d = strips(4)
    d.check("divide", MANY)


@pytest.mark.parametrize("n", sorted(pss.SCALE))
def test_one_bad_amplitude_in_a_carried_turn(gpu, strips, n):
    """One flat block of DC 20000.3 in a turn whose sums are carried: bit 63 for exactly (its plane, divisor 1), and every other
    cell, that plane under 1000 among them, equal to the yardstick."""
    s, strip, _ = strips(n)
    plane, block = pss.carried_block(s)
    changed = strip.copy()
    changed[block * n:(block + 1) * n] = BAD_DC / (n * n)
    d = psd.SetStrip(gpu, changed, psd.sizes_for(pss.scale_counts(n), n), 1, n)
    try:
        d.check("divide", BAD_DIVISORS, expect_bad=[(plane, 0)])
    finally:
        d.free()
