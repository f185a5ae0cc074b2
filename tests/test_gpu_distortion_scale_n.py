"""jpegx_probe_distortion_n beyond one turn per workgroup.  Every comparison is exact.

A workgroup of k_distort_n owns run = ceil(turns / DISTORT_MAX_WORKGROUPS) consecutive turns and keeps the sums of its current
plane in LDS from turn to turn, as k_probe_n does; below 8193 turns run is 1 and the carry, the clearing of sums that went out and
the plane comparison of `leave` are never exercised.  The stacks are those of tests/test_gpu_probe_scale_n.py -- 8195 and 16 388
turns at N = 2, 4, 9, 17, planes that are no multiple of a turn's blocks -- held against the same host model
(tests/probe_schedule.py): runs of 2 and 3, sums carried across turns, turns that cross plane ends.

The bands are constant per plane, seven levels cycled, one sample short of whole blocks on both axes: every block of a plane
then adds its error under the divisors used (steps of 7, 3, 40 and 64 grey levels), neighbouring planes differ, and the expected sums are those of the road
(tests/distortion_device.py) run once on the seven distinct planes."""
import numpy as np
import pytest

import probe_schedule as ps
from distortion_device import Stack
from test_gpu_probe_scale_n import SCALE

gpu_test = pytest.mark.gpu

LEVELS = [13, 250, 77, 1, 141, 201, 38]
STEPS = [7.0, 3.0, -40.0, 64.0]                      # the divisors are these times N^2: a flat block of level v decodes to the
#                                                      multiple of the step nearest to v (no level here lies halfway between two), so
#                                                      the seven planes have seven different rows of sums, none of them all zero


def constants():
    return ps.constant_of("jpegx_dctn_device.h", "DCTN_THREADS"), ps.constant_of("jpegx_distort_n.hip", "DISTORT_MAX_WORKGROUPS")


def test_the_premises():
    threads, max_wg = constants()
    for n, (hb, wb, nplanes, run) in SCALE.items():
        s = ps.Schedule(n, nplanes, hb * wb, threads, max_wg)
        assert s.run == run and s.nturns > max_wg and s.grid <= max_wg, (n, s.nturns, s.run)
        found = ps.events(s)
        for name in ["carry", "flush_then_on", "short_last"] + (["straddle_first", "straddle_later"] if s.bpw > 1 else []) \
                + (["carry_twice"] if run >= 3 else []):
            assert found[name], "N %d: no workgroup's run has the event %r" % (n, name)
        # the model's turn loop notices both defects on a weight per block that is constant per plane, as the bands here are
        weight = np.repeat(np.resize(np.arange(1, len(LEVELS) + 1), nplanes), hb * wb)
        want = weight.reshape(nplanes, hb * wb).sum(axis=1).tolist()
        assert ps.simulate(s, weight) == want
        assert ps.simulate(s, weight, clear=False) != want and ps.simulate(s, weight, leave_against=1) != want


def _bands(n, nplanes):
    hb, wb = SCALE[n][:2]
    rows, cols = hb * n - 1, wb * n - 1
    return np.broadcast_to(np.asarray(LEVELS, np.uint8)[np.arange(nplanes) % len(LEVELS), None, None], (nplanes, rows, cols))


@gpu_test
@pytest.mark.parametrize("n", sorted(SCALE))
def test_runs_of_two_and_three_turns(gpu, n):
    nplanes = SCALE[n][2]
    divisors = [c * n * n for c in STEPS]
    few = Stack(gpu, _bands(n, len(LEVELS)), 1, n)
    try:
        want, want_bad = few.road("divide", divisors)
    finally:
        few.free()
    assert not want_bad.any() and (want > 0).any(axis=1).all() and len({tuple(r) for r in want.tolist()}) == len(LEVELS)
    print("N %d: the road's sums of the seven planes %s" % (n, want.tolist()))
    cycle = np.arange(nplanes) % len(LEVELS)
    stack = Stack(gpu, _bands(n, nplanes), 1, n)
    try:
        stack.check("divide", divisors, (want[cycle], want_bad[cycle]), "scale")
        stack.check("divide", divisors[1:2], (want[cycle][:, 1:2], want_bad[cycle][:, 1:2]), "scale, one candidate")
    finally:
        stack.free()
