"""The shapes of tests/test_gpu_distortion_set_scale_n.py held against the host model of the ragged turn loop
(tests/probe_set_schedule.py; k_distort_n<true>'s turn loop is k_probe_n<true>'s).  No device: the constants are read from
jpegx_distort_n.hip and jpegx_dctn_device.h, so that a moved one fails here instead of sending the GPU test quietly back to
runs of one turn.

For every shape: more than DISTORT_MAX_WORKGROUPS turns and the run intended (2 and 3 turns); a carried run with a plane end
off a turn's boundary; and totals of the model that change under either of the two defects of probe_schedule.simulate (sums
never cleared, a wrong plane comparison in `leave`)."""
import numpy as np

import distortion_set_schedule as dss
import probe_set_schedule as pss
from test_probe_set_schedule import _irregular


def test_the_constants_are_the_size_probes():
    assert pss.constant_of("jpegx_distort_n.hip", "DISTORT_MAX_WORKGROUPS") == pss.constant_of("jpegx_probe_n.hip", "PROBE_MAX_WORKGROUPS")
    for n in pss.SCALE:
        assert dss.scale_schedule(n).runs() == pss.scale_schedule(n).runs()


def test_the_scale_shapes():
    max_wg = pss.constant_of("jpegx_distort_n.hip", "DISTORT_MAX_WORKGROUPS")
    threads = pss.constant_of("jpegx_dctn_device.h", "DCTN_THREADS")
    rng = np.random.default_rng(12)
    assert sorted(dss.SCALE) == [2, 4, 9, 17] and sorted(run for _, _, run in dss.SCALE.values()) == [2, 2, 2, 3]
    for n, (cycle, nplanes, run) in dss.SCALE.items():
        s = dss.scale_schedule(n)
        assert s.bpw == pss.blocks_per_wg(n, threads) and s.nturns > max_wg and s.run == run, (n, s.bpw, s.nturns, s.run)
        assert s.grid <= max_wg and (s.grid - 1) * s.run < s.nturns <= s.grid * s.run
        assert s.nblk * n * n * 8 <= 36 << 20
        found = pss.events(s)
        needed = ["carry", "flush_then_on", "short_last"] + (["straddle_first", "straddle_later"] if s.bpw > 1 else []) \
            + (["carry_twice"] if run >= 3 else [])
        for name in needed:
            assert found[name], "N %d: no workgroup's run has the event %r" % (n, name)
            if name != "short_last":
                assert _irregular(s, found[name]), "N %d: the event %r happens only at regular plane ends" % (n, name)
        # a plane end off a turn boundary INSIDE a carried run: the turn after a carried turn holds the end of the carried plane
        inside = 0
        for wg, turn in found["carry"]:
            nxt = s.turns_of(wg)[turn + 1 - wg * s.run]
            end = s.starts[nxt.plane0 + 1]
            inside += nxt.first < end < nxt.first + nxt.nlive and end % s.bpw != 0
        assert inside or s.bpw == 1, n
        weight = rng.integers(1, 40, s.nblk)
        want = [int(weight[a:b].sum()) for a, b in zip(s.starts, s.starts[1:])]
        assert pss.simulate(s, weight) == want
        assert pss.simulate(s, weight, clear=False) != want, "N %d would not notice sums that are never cleared" % n
        assert pss.simulate(s, weight, leave_against=1) != want, "N %d would not notice a wrong plane comparison" % n
        plane, block = pss.carried_block(s)
        assert 0 < plane < s.nplanes - 1 and s.starts[plane] <= block < s.starts[plane + 1]
