"""The shapes of tests/test_gpu_probe_set_scale_n.py held against the host model of the ragged turn loop
(tests/probe_set_schedule.py).  No device: the constants are read from the sources, so that a moved one fails here instead of
sending the GPU test quietly back to runs of one turn.

For every shape: more than PROBE_MAX_WORKGROUPS turns and the run intended; the model gives each plane the sum of its blocks
and, with either of the two defects of probe_schedule.simulate built in, does not; and every event a run of several turns can
have (carry, carry_twice at run 3, flush_then_on, straddle_first, straddle_later where a turn holds several blocks, short_last)
occurs at a plane whose end is NO multiple of a turn's blocks and whose neighbours have other block counts -- the ends of equal
planes are what the division of k_probe_n<false> already finds."""
from math import gcd

import numpy as np

import probe_set_schedule as pss


def _irregular(s, where):
    """The occurrences of an event whose plane ends off a turn's boundary (a block a turn: at an odd phase of the run) and
    between planes of other block counts."""
    out = []
    for wg, turn in where:
        t = s.turns_of(wg)[turn - wg * s.run]
        end = pss.plane_end_after(s, t)
        count = end - s.starts[t.plane0]
        off = end % s.bpw != 0 if s.bpw > 1 else end % s.run != 0
        after = s.starts[t.plane0 + 2] - end if t.plane0 + 2 <= s.nplanes else None
        before = s.starts[t.plane0] - s.starts[t.plane0 - 1] if t.plane0 > 0 else None
        if off and after != count and before != count:
            out.append((wg, turn))
    return out


def test_the_scale_shapes():
    max_wg = pss.constant_of("jpegx_probe_n.hip", "PROBE_MAX_WORKGROUPS")
    threads = pss.constant_of("jpegx_dctn_device.h", "DCTN_THREADS")
    rng = np.random.default_rng(11)
    for n, (cycle, nplanes, run) in pss.SCALE.items():
        counts = pss.scale_counts(n)
        s = pss.scale_schedule(n)
        assert s.bpw == pss.blocks_per_wg(n, threads) and s.nturns > max_wg and s.run == run, (n, s.bpw, s.nturns, s.run)
        assert s.grid <= max_wg and (s.grid - 1) * s.run < s.nturns <= s.grid * s.run
        assert s.nblk * n * n * 8 <= 36 << 20 and s.nblk * n * n <= 2 ** 31 - 1
        # no common block count: the counts share no divisor, and the cycle's length does not make the ends periodic in a turn
        g = 0
        for c in cycle:
            g = gcd(g, c)
        assert g == 1 and len(set(cycle)) > 3 and sum(cycle) % (s.bpw if s.bpw > 1 else s.run) != 0 and 1 in cycle
        found = pss.events(s)
        needed = ["carry", "flush_then_on", "short_last"] + (["straddle_first", "straddle_later"] if s.bpw > 1 else []) \
            + (["carry_twice"] if run >= 3 else [])
        for name in needed:
            assert found[name], "N %d: no workgroup's run has the event %r" % (n, name)
            if name != "short_last":
                assert _irregular(s, found[name]), "N %d: the event %r happens only at regular plane ends" % (n, name)
        assert s.nblk % s.bpw != 0 or s.bpw == 1               # short_last with a partial last turn where turns hold several blocks
        if s.bpw > 1:                                          # turns that hold many one-block planes
            assert max(t.rows for turns in s.runs() for t in turns) >= 3
        weight = rng.integers(1, 40, s.nblk)
        want = [int(weight[a:b].sum()) for a, b in zip(s.starts, s.starts[1:])]
        assert pss.simulate(s, weight) == want
        assert pss.simulate(s, weight, clear=False) != want, "N %d would not notice sums that are never cleared" % n
        assert pss.simulate(s, weight, leave_against=1) != want, "N %d would not notice a wrong plane comparison" % n
        plane, block = pss.carried_block(s)
        assert 0 < plane < s.nplanes - 1 and s.starts[plane] <= block < s.starts[plane + 1]
        assert counts[plane] == s.starts[plane + 1] - s.starts[plane]


def test_the_model_agrees_with_the_equal_model_on_equal_planes():
    """Equal planes through the list of starts: turn for turn the schedule of tests/probe_schedule.py."""
    import probe_schedule as ps
    for n, bpp, nplanes, max_wg in ((2, 35, 7, 8192), (4, 63, 50, 16), (17, 5, 40, 64)):
        a = ps.Schedule(n, nplanes, bpp, 256, max_wg)
        b = pss.SetSchedule(n, [p * bpp for p in range(nplanes + 1)], 256, max_wg)
        assert a.runs() == b.runs()
        weight = np.arange(1, nplanes * bpp + 1)
        for kw in ({}, {"clear": False}, {"leave_against": 1}):
            assert ps.simulate(a, weight, **kw) == pss.simulate(b, weight, **kw)


def test_the_model_on_runs_of_one_turn():
    """The small sets of the kernel test: run 1, every turn leaves, neither defect shows -- the scale test is what catches them."""
    counts = [1, 1, 1, 6, 35, 1, 2, 64, 65, 3]
    for n in (2, 4, 16):
        s = pss.SetSchedule(n, pss.starts_of(counts), 256, 8192)
        weight = np.arange(1, s.nblk + 1)
        want = [int(weight[a:b].sum()) for a, b in zip(s.starts, s.starts[1:])]
        assert s.run == 1 and all(t.leave for turns in s.runs() for t in turns)
        assert pss.simulate(s, weight) == pss.simulate(s, weight, clear=False) == pss.simulate(s, weight, leave_against=1) == want
