"""The dct_size-8 probes past their grid cap, against tests/probe_oracle_8.py.  Every comparison is exact.

A workgroup of k_probe_8 is one wave that takes 64 blocks a turn and owns run = ceil(turns / PROBE8_MAX_WORKGROUPS) consecutive
turns, keeping the sums of its current plane in LDS from turn to turn.  Below the cap run is 1, every turn is the last of its
run, and three things never happen: the plane comparison of `leave` decides, the sums are cleared for a turn that follows, row
0 is carried into the next turn.  The stack here is the smallest of its planes that gives a workgroup a second turn: 1748
planes of 10 x 15 blocks (80 x 120 samples behind bands of 78 x 119 pixels at block_size 1, so the crop is live), 262 200
blocks, 4097 turns, 134 MB of planes and as much of moments, uploaded once.  Seven distinct bands are cycled, so the oracle
runs on seven.

test_the_premises needs no device: it reads the cap from the source and holds the shape against the model of
tests/probe_schedule.py (a block per thread of a 64-thread workgroup), so that a moved constant fails there instead of sending
the GPU tests quietly back to run 1."""
import numpy as np
import pytest

import probe_oracle_8 as po
import probe_schedule as ps

gpu_test = pytest.mark.gpu

DISTINCT = 7
ROWS, COLS, BS = 78, 119, 1                          # bands of 78 x 119 pixels: planes of 80 x 120 samples, 10 x 15 blocks
HB, WB, NPLANES = 10, 15, 1748
DIVISORS = [1.0, 3.0, 64.0]                          # a multiply (1, 64) and a true division
BAD = np.uint64(1 << 63)


def cap():
    return ps.constant_of("jpegx_probe_8.hip", "PROBE8_MAX_WORKGROUPS")


def test_the_premises():
    max_wg = cap()
    s = ps.Schedule(1, NPLANES, HB * WB, 64, max_wg)   # n = 1: a "block" of the model is a block of a 64-lane turn
    assert s.bpw == 64 and s.nturns > max_wg and s.run == 2 and s.grid <= max_wg
    assert ps.Schedule(1, NPLANES - 1, HB * WB, 64, max_wg).run == 1, "not the smallest stack of these planes"
    assert (HB * WB) % 64 != 0 and NPLANES > DISTINCT
    assert po.band_plane(np.zeros((ROWS, COLS)), BS).shape == (HB * 8, WB * 8)
    found = ps.events(s)
    for name in ("carry", "flush_then_on", "short_last", "straddle_first", "straddle_later"):
        assert found[name], "no workgroup's run has the event %r" % name
    rng = np.random.default_rng(5)
    weight = np.tile(rng.integers(1, 40, (DISTINCT, HB * WB)), (-(-NPLANES // DISTINCT), 1))[:NPLANES].ravel()
    want = weight.reshape(NPLANES, HB * WB).sum(axis=1).tolist()
    assert ps.simulate(s, weight) == want
    assert ps.simulate(s, weight, clear=False) != want, "the shape would not notice sums that are never cleared"
    assert ps.simulate(s, weight, leave_against=1) != want, "the shape would not notice a wrong plane comparison"


def distinct_bands():
    rng = np.random.default_rng(88)
    yy, xx = np.mgrid[0:ROWS, 0:COLS]
    out = []
    for p in range(DISTINCT):
        smooth = 127.5 + (20 + 15 * p) * np.sin(0.03 * (p + 1) * xx) * np.cos(0.05 * yy)
        noise = rng.integers(-(4 ** (p % 4)), 4 ** (p % 4) + 1, (ROWS, COLS))
        out.append(np.clip(np.rint(smooth + noise), 0, 255).astype(np.uint8))
    return out


@pytest.fixture(scope="module")
def stack(gpu):
    bands = distinct_bands()
    cycle = np.arange(NPLANES) % DISTINCT
    planes = np.stack([po.band_plane(b, BS) for b in bands])[cycle]
    moments = np.stack([po.band_moments(b, BS) for b in bands])[cycle]
    din, dmo, dtot = gpu.DeviceBuffer(planes.nbytes), gpu.DeviceBuffer(moments.nbytes), gpu.DeviceBuffer(NPLANES * len(DIVISORS) * 8)
    din.upload(planes)
    dmo.upload(moments)
    yield bands, cycle, din, dmo, dtot
    for b in (din, dmo, dtot):
        b.free()


def _totals(gpu, dtot, k):
    gpu.check(gpu.lib().jpegx_stream_synchronize(None))
    raw = dtot.download((NPLANES, k), np.uint64)
    return (raw & ~BAD).astype(np.int64), (raw & BAD) != 0


@gpu_test
def test_sizes_over_runs_of_two_turns(gpu, stack):
    bands, cycle, din, dmo, dtot = stack
    want, want_bad = po.band_sizes(bands, BS, "divide", DIVISORS)
    assert not want_bad.any()
    for _ in range(2):                                                  # twice: identical totals
        gpu.probe_sizes_8_device(din.ptr, NPLANES, HB * 8, WB * 8, "divide", DIVISORS, dtot.ptr)
        got, bad = _totals(gpu, dtot, len(DIVISORS))
        assert not bad.any()
        wrong = np.argwhere(got != want[cycle])
        assert wrong.size == 0, (len(wrong), wrong[:8].tolist())


@gpu_test
def test_distortion_over_runs_of_two_turns(gpu, stack):
    bands, cycle, din, dmo, dtot = stack
    want, want_bad = po.band_sse(bands, BS, "divide", DIVISORS)
    assert not want_bad.any() and (want[:, 1] > 0).all()
    gpu.probe_distortion_8_device(din.ptr, dmo.ptr, NPLANES, HB * 8, WB * 8, BS, ROWS, COLS, "divide", DIVISORS, dtot.ptr)
    got, bad = _totals(gpu, dtot, len(DIVISORS))
    assert not bad.any()
    wrong = np.argwhere(got != want[cycle])
    assert wrong.size == 0, (len(wrong), wrong[:8].tolist())
