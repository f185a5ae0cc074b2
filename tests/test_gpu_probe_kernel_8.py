"""jpegx_probe_sizes_8 and jpegx_probe_distortion_8 against tests/probe_oracle_8.py, which is built from the checker alone and
pinned to the reference by tests/golden/probe8.npz.  Every comparison is exact: the 8 x 8 roads are bit-exact with the
reference, rounding ties included, and so are the probes.

Shapes: seven bands unlike each other (noise at three amplitudes, smooth, smooth with noise, all zero, all white) of 70 x 118
pooled 3 x 3 into planes of 3 x 5 blocks -- 105 blocks, so a wave's 64 lanes span five planes, the second wave has dead lanes
and a sum that leaked into a neighbour shows; and one band of 70 x 61 in a plane of 9 x 8 blocks, two waves inside one plane.
The planes sit at a pitch whose gap holds 1e300, the totals between canaries on garbage."""
import numpy as np
import pytest

import probe_oracle_8 as po

pytestmark = pytest.mark.gpu

BAD = np.uint64(1 << 63)
CANARY = np.uint64(0xC0FFEE0DDBA11AD5)
MANY = [float(v) for v in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128, 160, 200, 256, 300, 400, 512, 640,
                           800, 1000, 2000, 4096, 100000)]
CASES = [("none", [0.0]), ("qtable", [0.0]), ("discard", [0.0, 2.0, 8.0]), ("discard", [2.0]), ("divide", [40.0]),
         ("divide", [3.0, 64.0]), ("divide", MANY)]


def seven_bands(rows=70, cols=118):
    rng = np.random.default_rng(808)
    yy, xx = np.mgrid[0:rows, 0:cols]
    smooth = np.rint(127.5 + 100 * np.sin(0.11 * xx) * np.cos(0.07 * yy) + 0.3 * yy)
    bands = [rng.integers(0, 256, (rows, cols)), rng.integers(120, 137, (rows, cols)), rng.integers(0, 2, (rows, cols)) * 255, smooth,
             smooth + rng.integers(-9, 10, (rows, cols)), np.zeros((rows, cols)), np.full((rows, cols), 255)]
    return [np.clip(b, 0, 255).astype(np.uint8) for b in bands]


def one_band(rows=70, cols=61):
    rng = np.random.default_rng(809)
    yy, xx = np.mgrid[0:rows, 0:cols]
    return [np.clip(np.rint(128 + 90 * np.sin(0.05 * xx * yy / 9.0)) + rng.integers(-30, 31, (rows, cols)), 0, 255).astype(np.uint8)]


class Device:
    """Bands as planes and moments on the device, at pitches of their own, and the probes between canaries."""

    def __init__(self, gpu, bands, bs, pad=3, scale=None):
        self.gpu, self.L, self.bands, self.bs = gpu, gpu.lib(), bands, bs
        self.rows, self.cols = bands[0].shape
        planes = np.stack([po.band_plane(b, bs) for b in bands])
        if scale is not None:                                          # the size probe takes any float64 plane
            planes = planes * np.asarray(scale, np.float64)[:, None, None]
        self.planes = planes
        self.nplanes, self.h, self.w = planes.shape
        self.pitch, self.mpitch = self.w + pad, self.w + pad + 2
        tall = np.full((self.nplanes * self.h, self.pitch), 1e300)      # the gap would flag everything if it were read
        tall[:, :self.w] = planes.reshape(-1, self.w)
        mom = np.full((self.nplanes * self.h, self.mpitch), np.uint64(0xFFFFFFFFFFFFFFFF))
        mom[:, :self.w] = np.stack([po.band_moments(b, bs) for b in bands]).reshape(-1, self.w)
        self.din, self.dmo = gpu.DeviceBuffer(tall.nbytes), gpu.DeviceBuffer(mom.nbytes)
        self.din.upload(tall)
        self.dmo.upload(mom)

    def _run(self, k, enqueue):
        count = self.nplanes * k
        dtot = self.gpu.DeviceBuffer((count + 4) * 8)
        fill = np.full(count + 4, np.uint64(0xDEADBEEFDEADBEEF))        # garbage where the totals go
        fill[:2] = fill[-2:] = CANARY
        dtot.upload(fill)
        enqueue(dtot.ptr + 16)
        self.gpu.check(self.L.jpegx_stream_synchronize(None))
        raw = dtot.download((count + 4,), np.uint64)
        dtot.free()
        assert (raw[:2] == CANARY).all() and (raw[-2:] == CANARY).all()
        raw = raw[2:-2].reshape(self.nplanes, k)
        return (raw & ~BAD).astype(np.int64), (raw & BAD) != 0

    def sizes(self, mode, params, device=None):
        return self._run(len(params), lambda t: self.gpu.probe_sizes_8_device(self.din.ptr, self.nplanes, self.h, self.w, mode, params, t,
                                                                              pitch=self.pitch, device=device))

    def sse(self, mode, params):
        return self._run(len(params), lambda t: self.gpu.probe_distortion_8_device(self.din.ptr, self.dmo.ptr, self.nplanes, self.h, self.w, self.bs,
                                                                                   self.rows, self.cols, mode, params, t, pitch=self.pitch,
                                                                                   mpitch=self.mpitch))

    def check_sizes(self, mode, params):
        got, bad = self.sizes(mode, params)
        want, want_bad = po.plane_sizes(self.planes, mode, params)
        assert np.array_equal(bad, want_bad), (mode, params)
        assert np.array_equal(got[~want_bad], want[~want_bad]), (mode, params, got, want)
        again, again_bad = self.sizes(mode, params)                       # two calls in a row: identical totals
        assert np.array_equal(again[~bad], got[~bad]) and np.array_equal(again_bad, bad)
        return got, bad

    def check_sse(self, mode, params):
        got, bad = self.sse(mode, params)
        want, want_bad = po.band_sse(self.bands, self.bs, mode, params)
        assert np.array_equal(bad, want_bad), (mode, params)
        assert np.array_equal(got[~want_bad], want[~want_bad]), (mode, params, got, want)
        return got, bad

    def free(self):
        self.din.free()
        self.dmo.free()


@pytest.fixture(scope="module")
def stacks(gpu):
    devs = [Device(gpu, seven_bands(), 3), Device(gpu, one_band(), 1, pad=0)]
    yield devs
    for d in devs:
        d.free()


@pytest.mark.parametrize("mode, params", CASES, ids=["%s-K%d" % (m, len(p)) for m, p in CASES])
def test_sizes_equal_the_oracle(stacks, mode, params):
    for d in stacks:
        got, bad = d.check_sizes(mode, params)
        assert not bad.any() and (got >= (d.h // 8) * (d.w // 8)).all()      # a block is one byte at least
    if mode == "divide":
        got, _ = stacks[0].check_sizes(mode, params)
        assert (got[5] == 15).all()                                          # the all-zero plane: one byte per block


@pytest.mark.parametrize("mode, params", CASES, ids=["%s-K%d" % (m, len(p)) for m, p in CASES])
def test_distortion_equals_the_oracle(stacks, mode, params):
    for d in stacks:
        got, bad = d.check_sse(mode, params)
        assert not bad.any()
    if mode == "divide" and len(params) == 32:
        got, _ = stacks[0].check_sse(mode, params)
        assert (np.diff(got[0]) >= 0).any() and got[0, -1] > got[0, 0]       # noise loses more under coarser divisors
        assert (got[5] == 0).all()                                           # all zero comes back as it was


def test_scaled_planes_and_bit_63_for_exactly_the_bad_entries(gpu):
    """Any float64 plane is taken; amplitudes beyond 15 bits raise bit 63 for their plane and candidate alone."""
    d = Device(gpu, seven_bands(), 3, pad=1, scale=[1.0, 0.37, 60.0, 1.0, -2.5, 1.0, 1.5])
    try:
        got, bad = d.check_sizes("divide", [1.0, 40.0, 0.25])
        assert bad[2, 0] and bad[6, 0] and not bad[5].any() and not bad[:, 1].any() and bad[:, 2].sum() >= 5
        d.check_sizes("none", [0.0])
    finally:
        d.free()


def test_one_block_a_plane_with_thirty_two_candidates(gpu):
    """70 bands of 7 x 6 pixels in planes of ONE block: a wave spans 64 planes, so every lane adds into a row of its own (the
    lane-by-lane path on 64 rows of sums), and with 32 candidates the distortion kernel's dynamic LDS is at its largest, 64 * 32 * 8
    + 49152 = 65536 bytes.  The second wave has six lanes."""
    rng = np.random.default_rng(810)
    bands = [np.clip(rng.integers(0, 256, (7, 6)) // (1 + p % 5) + 3 * (p % 11), 0, 255).astype(np.uint8) for p in range(70)]
    d = Device(gpu, bands, 1, pad=1)
    try:
        assert (d.nplanes, d.h, d.w) == (70, 8, 8)
        for params in (MANY, [3.0, 40.0]):
            got, bad = d.check_sizes("divide", params)
            sse, bad2 = d.check_sse("divide", params)
            assert not bad.any() and not bad2.any() and len(set(got[:, 0].tolist())) > 8 and len(set(sse[:, -1].tolist())) > 8
        d.check_sse("qtable", [0.0])
    finally:
        d.free()


def test_explicit_device_form(stacks):
    d = stacks[1]
    got, bad = d.sizes("divide", [3.0, 40.0], device=0)
    want, _ = po.plane_sizes(d.planes, "divide", [3.0, 40.0])
    assert np.array_equal(got, want) and not bad.any()
