"""jpegx_probe_sizes_n beyond one turn per workgroup, against tests/codec_oracle_n.py.  Every comparison is exact.

A workgroup of k_probe_n owns run = ceil(turns / PROBE_MAX_WORKGROUPS) consecutive turns and keeps the byte sums of its current
plane in LDS from turn to turn; below 8193 turns run is 1, every turn is the last of its run, and three things never happen:
the plane comparison of `leave` decides, the sums are cleared for a turn that follows, row 0 is carried into the next turn.
The stacks here are just large enough for run 2 and 3, with planes that are no multiple of a turn's blocks:

   N  blocks/turn  blocks/plane  planes  turns  run
   2      64         15 x 15      2331    8195   2    16 blocks per wave step, steps and turns across plane ends
   4      16          7 x 9       4162   16388   3    a carry over two turns
   9       3          2 x 4       3073    8195   2    the path of 64 coefficients and more, two steps per block
  17       1          1 x 5       1639    8195   2    a block per turn, strided passes, plane ends at both phases of a run

Seven distinct planes are cycled (probe_oracle.distinct_planes), so the oracle runs on seven planes per case; the expected
total of plane p under divisor d is len(Forward(distinct[p % 7], 1, N, "divide", d, peak=amp + 1).blob()), and every one of
those cells is asserted to lie off the rounding ties (probe_oracle.expected).

test_the_premises needs no device: it reads PROBE_MAX_WORKGROUPS and DCTN_THREADS from the sources and holds every shape
against the model of tests/probe_schedule.py, so that a moved constant fails there instead of sending the GPU tests quietly
back to run 1.  It also runs the model's turn loop with each of two defects built in -- the sums not cleared after they went
out; `leave` comparing the next turn's plane against plane0 + 1 -- and asserts that every shape's totals change under each."""
import numpy as np
import pytest

import probe_oracle as po
import probe_schedule as ps

gpu_test = pytest.mark.gpu

DISTINCT = 7
# N -> (block rows, block columns, planes, the run intended)
SCALE = {2: (15, 15, 2331, 2), 4: (7, 9, 4162, 3), 9: (2, 4, 3073, 2), 17: (1, 5, 1639, 2)}
DIVISORS = [1.0, 3.0, -40.0, 64.0]                   # a multiply (1, 64), two true divisions, a negative one
MANY_N = 4                                           # the case with 32 candidates
MANY = [1, 2, 3, 4, 5, 6, 7, 8, -10, 12, 16, 20, 24, 32, -40, 48, 64, 80, 96, 128, 0.75, 0.5, -0.25, 0.3, 300, 400, 512, 640, -800, 1000,
        2000, 4096]
BAD_DIVISORS = [1.0, 1000.0]
BAD_DC = 20000.3                                     # the DC of the one bad block: beyond 16383 under 1, 20 under 1000
MAX_STACK_BYTES = 36 << 20
# the batch entry: one picture of three bands at dct_size 2 whose one group of planes is the smallest beyond 8192 turns
PICTURE = (837, 838)                                 # rows, cols: planes of 419 x 419 blocks, the last sample row is padding
PICTURE_N, PICTURE_DIVISORS = 2, [1, 3, 40]


def constants():
    return ps.constant_of("jpegx_dctn_device.h", "DCTN_THREADS"), ps.constant_of("jpegx_probe_n.hip", "PROBE_MAX_WORKGROUPS")


def schedule_of(n):
    hb, wb, nplanes, _ = SCALE[n]
    return ps.Schedule(n, nplanes, hb * wb, *constants())


def carried_block(n):
    """(plane P, block row, block column) of a block in a CARRIED turn of the middle of the grid: a turn inside plane P whose sums
    stay in LDS, to leave with a later turn of the same run."""
    hb, wb, _, _ = SCALE[n]
    s = schedule_of(n)
    carries = ps.events(s)["carry"]
    wg, turn = carries[len(carries) // 2]
    t = s.turns_of(wg)[turn - wg * s.run]
    assert t.turn == turn and not t.leave and t.rows == 1
    block = t.first + t.nlive // 2
    assert s.turn_of_block(block) == t and block // s.bpp == t.plane0
    return (t.plane0,) + divmod(block - t.plane0 * s.bpp, wb)


def test_the_premises():
    threads, max_wg = constants()
    assert len(MANY) == 32 and MANY_N in SCALE
    rng = np.random.default_rng(5)
    for n, (hb, wb, nplanes, run) in SCALE.items():
        s = schedule_of(n)
        bpp = hb * wb
        assert s.bpw == ps.blocks_per_wg(n, threads) and s.run == run and s.nturns > max_wg, (n, s.bpw, s.nturns, s.run)
        assert s.grid <= max_wg and (s.grid - 1) * s.run < s.nturns <= s.grid * s.run
        assert nplanes * bpp * n * n * 8 <= MAX_STACK_BYTES and nplanes > DISTINCT
        assert s.bpw == 1 or bpp % s.bpw != 0, "N %d: planes of whole turns, no turn lies across a plane's end" % n
        found = ps.events(s)
        needed = ["carry", "flush_then_on", "short_last"] + (["straddle_first", "straddle_later"] if s.bpw > 1 else []) \
            + (["carry_twice"] if run >= 3 else [])
        for name in needed:
            assert found[name], "N %d: no workgroup's run has the event %r" % (n, name)
        if s.bpw == 1:                                     # plane ends at both phases: behind the first and behind the last turn of a run
            ends = {t.turn - t.wg * s.run for turns in s.runs() for t in turns if (t.first + 1) % bpp == 0}
            assert ends == set(range(run)), (n, ends)
        # the turn loop of the model gives each plane the sum of its blocks; with either defect it does not
        weight = np.tile(rng.integers(1, 40, (DISTINCT, bpp)), (-(-nplanes // DISTINCT), 1))[:nplanes].ravel()
        want = weight.reshape(nplanes, bpp).sum(axis=1).tolist()
        assert ps.simulate(s, weight) == want
        assert ps.simulate(s, weight, clear=False) != want, "N %d would not notice sums that are never cleared" % n
        assert ps.simulate(s, weight, leave_against=1) != want, "N %d would not notice a wrong plane comparison" % n
        plane, by, bx = carried_block(n)
        assert 0 < plane < nplanes - 1 and 0 <= by < hb and 0 <= bx < wb
    # the picture of the batch case: its three planes are one group, the smallest square of blocks beyond max_wg turns
    rows, cols = PICTURE
    hb, wb = -(-rows // PICTURE_N), -(-cols // PICTURE_N)
    assert rows % PICTURE_N != 0 and hb == wb
    s = ps.Schedule(PICTURE_N, 3, hb * wb, threads, max_wg)
    assert s.nturns > max_wg and s.run == 2
    assert ps.Schedule(PICTURE_N, 3, (hb - 1) * (wb - 1), threads, max_wg).run == 1
    found = ps.events(s)
    assert found["carry"] and found["flush_then_on"]


def test_the_model_on_runs_of_one_turn():
    """The shapes of the older probe tests: run 1, every turn leaves, and neither defect shows in the model -- which is why those
    tests pass with either."""
    threads, max_wg = constants()
    for n, bpp, nplanes in ((2, 35, 7), (4, 35, 7), (7, 6, 3), (17, 35, 7)):
        s = ps.Schedule(n, nplanes, bpp, threads, max_wg)
        weight = np.arange(1, nplanes * bpp + 1)
        want = weight.reshape(nplanes, bpp).sum(axis=1).tolist()
        assert s.run == 1 and all(t.leave for turns in s.runs() for t in turns)
        assert ps.simulate(s, weight) == ps.simulate(s, weight, clear=False) == ps.simulate(s, weight, leave_against=1) == want


# ---- the device ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stacks(gpu):
    """(the seven distinct planes, the plane -> distinct index, the stack on the device) per dct_size, made once."""
    cache = {}

    def get(n):
        if n not in cache:
            hb, wb, nplanes, _ = SCALE[n]
            distinct = po.distinct_planes(n, hb, wb, DISTINCT)
            distinct.setflags(write=False)
            cycle = np.arange(nplanes) % DISTINCT
            cache[n] = (distinct, cycle, po.Stack(gpu, distinct[cycle], n))
        return cache[n]
    yield get
    for _, _, stack in cache.values():
        stack.free()


_expected = {}


def expected(n, distinct, divisors):
    """The oracle on the seven planes, once per (N, candidates); read-only."""
    key = (n, tuple(divisors))
    if key not in _expected:
        _expected[key] = po.expected(distinct, n, "divide", divisors, peak=po.amp_of(n) + 1.0)
        for a in _expected[key]:
            a.setflags(write=False)
    return _expected[key]


@gpu_test
@pytest.mark.parametrize("n", sorted(SCALE))
def test_runs_of_two_and_three_turns_against_the_oracle(gpu, stacks, n):
    distinct, cycle, stack = stacks(n)
    want, want_bad = expected(n, distinct, DIVISORS)
    assert not want_bad.any()
    print("N %d: the oracle's sizes of the seven planes %s" % (n, want.tolist()))
    stack.check("divide", DIVISORS, want[cycle], want_bad[cycle], "scale")
    stack.check("divide", DIVISORS[1:2], want[cycle][:, 1:2], want_bad[cycle][:, 1:2], "scale, one candidate")


@gpu_test
def test_thirty_two_candidates_over_runs_of_three_turns(gpu, stacks):
    distinct, cycle, stack = stacks(MANY_N)
    want, want_bad = expected(MANY_N, distinct, MANY)
    assert not want_bad.any()
    stack.check("divide", MANY, want[cycle], want_bad[cycle], "32 candidates")


@gpu_test
@pytest.mark.parametrize("n", sorted(SCALE))
def test_one_bad_amplitude_in_a_carried_turn(gpu, stacks, n):
    """One flat block of DC 20000.3 in plane P, in a turn whose sums are carried: bit 63 for exactly (P, divisor 1), and every
    other cell, P under 1000 among them, equal to the oracle."""
    distinct, cycle, _ = stacks(n)
    hb, wb, nplanes, _ = SCALE[n]
    plane, by, bx = carried_block(n)
    changed = distinct[cycle[plane]].copy()
    changed[by * n:(by + 1) * n, bx * n:(bx + 1) * n] = BAD_DC / (n * n)
    want, want_bad = (a[cycle] for a in expected(n, distinct, BAD_DIVISORS))
    assert not want_bad.any()
    own, own_bad = po.expected(changed[None], n, "divide", BAD_DIVISORS)
    assert own_bad.tolist() == [[True, False]]
    want[plane], want_bad[plane] = own[0], own_bad[0]
    planes = distinct[cycle]
    planes[plane] = changed
    stack = po.Stack(gpu, planes, n)
    try:
        _, bad = stack.check("divide", BAD_DIVISORS, want, want_bad, "bad amplitude in plane %d" % plane)
        assert np.argwhere(bad).tolist() == [[plane, 0]]
    finally:
        stack.free()


@gpu_test
def test_batch_entry_over_runs_of_two_turns(gpu):
    """jpegx.batch_probe_pictures_n on one picture whose three planes, one group, are 8230 turns, against the sizes-only batch
    compression per candidate: device against device on purpose, 8-bit pictures cannot be kept off the ties."""
    from test_gpu_probe_pictures_n import _pixels, _yardstick
    rows, cols = PICTURE
    pixels = _pixels(1, rows, cols, 3)
    want, refused = _yardstick(gpu, pixels, 1, PICTURE_N, "divide", PICTURE_DIVISORS, 0, 3)
    assert not refused.any()
    got, bad = gpu.batch_probe_pictures_n(pixels, 1, PICTURE_N, "divide", PICTURE_DIVISORS, group_planes=3)
    assert not bad.any() and np.array_equal(got, want), (got.tolist(), want.tolist())
    again, _ = gpu.batch_probe_pictures_n(pixels, 1, PICTURE_N, "divide", PICTURE_DIVISORS, group_planes=3)
    assert np.array_equal(again, got)
