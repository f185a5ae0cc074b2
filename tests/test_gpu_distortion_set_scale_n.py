"""jpegx_probe_distortion_set_n beyond one turn per workgroup, against the road it stands for (tests/distortion_set_device.py).
Every comparison is exact.

Below 8193 turns every turn is the last of its run, and three things never happen: the plane comparison of `leave` decides,
the sums are cleared for a turn that follows, row 0 is carried into the next turn.  The sets here are just large enough for
runs of 2 and 3 turns, over planes of UNEQUAL block counts (tests/distortion_set_schedule.py: SCALE):

   N  blocks/turn  blocks per plane, cycled                          planes   turns  run
   2      64       225 1 1 383 64 65 7 130 1 200 3 449                 4125    8209   2
   4      16       63 1 100 5 37 150 16 17 1 81                        5570   16397   3
   9       3       4 1 7 2 3 11 1 5                                    5788    8199   2
  17       1       1 5 2 1 7 3 4                                       2496    8197   2

Every picture is one band of one row of blocks at block_size 1, its width cropped by p mod N pixels.
tests/test_distortion_set_schedule.py holds these shapes against the host model without a device."""
import numpy as np
import pytest

import distortion_set_device as dsd
import distortion_set_schedule as dss
import probe_set_schedule as pss

pytestmark = pytest.mark.gpu

DIVISORS = [1.0, 3.0, -40.0, 64.0]                   # a multiply (1, 64), two true divisions, a negative one
BAD_DIVISORS = [1.0, 1000.0]
BAD_DC = 20000.3                                     # the DC of the one bad block: beyond 16383 under 1, 20 under 1000


def _pictures(n, counts):
    """Noise of unlike amplitudes, as bright as dct_size allows under divisor 1, every fifth picture flat."""
    rng = np.random.default_rng(n)
    peak = min(255, 16383 // (n * n))
    out = []
    for p, c in enumerate(counts):
        cols = c * n - p % n
        px = rng.integers(0, max(peak >> (p % 4), 1) + 1, (n, cols, 1), dtype=np.uint8)
        out.append(np.full_like(px, p % (peak + 1)) if p % 5 == 0 else px)
    return out


@pytest.fixture(scope="module")
def sets(gpu):
    cache = {}

    def get(n):
        if n not in cache:
            s = dss.scale_schedule(n)
            d = dsd.PictureSet(gpu, _pictures(n, dss.scale_counts(n)), 1, n)
            assert d.first.tolist() == s.starts
            cache[n] = (s, d)
        return cache[n]
    yield get
    for _, d in cache.values():
        d.free()


@pytest.mark.parametrize("n", sorted(dss.SCALE))
def test_runs_of_two_and_three_turns(sets, n):
    s, d = sets(n)
    assert s.run == dss.SCALE[n][2] and s.nturns > 8192
    got = d.check("divide", DIVISORS)
    assert (got[:, 2] > got[:, 0]).any()
    d.check("divide", DIVISORS[1:2])
    # a sub-range that starts inside what was a carried run of the whole set: its own turns, its own rows
    d.check("divide", DIVISORS[:2], 3, s.nplanes - 5)


def test_thirty_two_candidates_over_runs_of_three_turns(sets):
    from test_gpu_distortion_set_kernel_n import MANY
    _, d = sets(4)
    d.check("divide", MANY)


@pytest.mark.parametrize("n", sorted(dss.SCALE))
def test_one_bad_amplitude_in_a_carried_turn(gpu, sets, n):
    """One flat block of DC 20000.3 in a turn whose sums are carried: bit 63 for exactly (its plane, divisor 1), and every other
    cell, that plane under 1000 among them, equal to the yardstick."""
    s, d = sets(n)
    plane, block = pss.carried_block(s)
    strip = d.gather()[0][dsd.MARGIN:-dsd.MARGIN].reshape(-1, n).copy()
    strip[block * n:(block + 1) * n] = BAD_DC / (n * n)
    changed = dsd.PictureSet(gpu, d.pictures, 1, n, strip=strip)
    try:
        changed.check("divide", BAD_DIVISORS, expect_bad=[(plane, 0)])
    finally:
        changed.free()
