"""What the size probe (jpegx_probe_sizes_n) must give, from tests/codec_oracle_n.py alone: the length of the oracle's byte
stream per plane and candidate, or the bad-amplitude flag.  A helper module of the suite; it imports nothing of the product
(the `gpu` module reaches Stack as an argument).

Content.  The planes are built OFF the rounding ties, so that a plane and a candidate have exactly one admissible stream:
noise is round(uniform(-a, a), 2) + uniform(-1e-3, 1e-3) -- two decimals alone land on ties under whole divisors -- with
a <= amp = min(128, 12000 / N^2), which keeps every coefficient of the un-normalised transform inside the 15 bits of a code
under divisor 1.  Seven planes unlike each other (five of noise at different amplitudes, a smooth one, an all-zero one), so
that a sum that leaks into a neighbouring plane shows.

What is asserted of the oracle before anything is compared (a failure means: change the seed, nothing is masked):
  * a cell (plane, candidate) whose largest |v| is within tau of 16383.5 has no certain flag: none may exist;
  * a cell that is not flagged has Forward.distance > Forward.tau: no coefficient of it within tau of a half-integer.
A flagged cell's size is unspecified, so its other ties do not matter (under divisors like 1e-30 tau exceeds 1/2 and the
distance could not pass it)."""
import numpy as np

import codec_oracle_n as on
from codec_oracle import BadRleCodeError, MAX_AMPLITUDE

BAD = np.uint64(1 << 63)
CANARY = np.uint64(0xC0FFEE0DDBA11AD5)
MODES = {"none": 0, "discard": 1, "divide": 2}


def amp_of(n):
    return min(128.0, 12000.0 / (n * n))


def noise(rng, a, shape):
    return np.round(rng.uniform(-a, a, shape), 2) + rng.uniform(-1e-3, 1e-3, shape)


def distinct_planes(n, hb, wb, count=7, seed=0):
    """count (at most 7) float64 planes of hb x wb blocks: noise, all zero, smooth, then noise at four lower amplitudes."""
    rng = np.random.default_rng([n, hb, wb, seed])
    h, w = hb * n, wb * n
    amp = amp_of(n)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = (yy * 1.75 + xx * 0.5 + 1.0) / (h * 1.75 + w * 0.5 + 1.0) * 2.0 - 1.0
    smooth = amp * (0.55 * ramp + 0.4 * np.sin(0.37 * yy + 0.11) * np.cos(0.23 * xx + 0.05))
    out = [noise(rng, amp, (h, w)), np.zeros((h, w)), smooth + rng.uniform(-1e-3, 1e-3, (h, w))]
    out += [noise(rng, amp * f, (h, w)) for f in (0.5, 0.2, 0.05, 0.33)]
    planes = np.stack(out[:count])
    assert np.abs(planes).max() <= amp + 0.01                # rounding to two decimals and the jitter may pass amp, by less than this
    return planes


class Cell:
    """One plane under one candidate: size (None where flagged), bad, distance, tau, margin (| max|v| - 16383.5 |)."""

    def __init__(self, plane, n, mode, param, peak):
        with np.errstate(invalid="ignore"):                 # Forward.k is an int64 cast, undefined beyond 2^63 (divisor 1e-30)
            f = on.Forward(plane, 1, n, mode, param, peak=peak)
        self.tau, self.distance = f.tau, f.distance
        top = float(np.abs(f.v).max())
        self.margin = abs(top - (MAX_AMPLITUDE + 0.5))
        if top > 2.0 ** 62:                                 # blob() would look at the wrapped cast
            self.size, self.bad = None, True
        else:
            try:
                self.size, self.bad = len(f.blob()), False
            except BadRleCodeError:
                self.size, self.bad = None, True

    def certain(self):
        return self.margin > self.tau and (self.bad or self.distance > self.tau)


def expected(planes, n, mode, params, peak=None):
    """(sizes uint64 [planes][K], bad bool [planes][K]) of the oracle; peak None: every plane's own largest |sample|.  Every
    cell is certain, or the assertion names it."""
    sizes = np.zeros((len(planes), len(params)), np.uint64)
    bad = np.zeros((len(planes), len(params)), bool)
    for p, plane in enumerate(planes):
        pk = float(np.abs(plane).max()) if peak is None else peak
        for q, param in enumerate(params):
            c = Cell(plane, n, mode, param, pk)
            assert c.certain(), "N %d %s %r plane %d: distance %.3g, margin %.3g, tau %.3g" % (n, mode, param, p, c.distance, c.margin, c.tau)
            bad[p, q] = c.bad
            sizes[p, q] = 0 if c.bad else c.size
    return sizes, bad


class Stack:
    """Planes [nplanes][h][w] on the device at a pitch of w + pad doubles; the probe between canaries."""

    def __init__(self, gpu, planes, n, pad=0):
        self.gpu, self.n = gpu, n
        self.nplanes, self.h, self.w = planes.shape
        self.pitch = self.w + pad
        if pad:
            tall = np.full((self.nplanes * self.h, self.pitch), 1e300)      # the pitch gap would flag everything if it were read
            tall[:, :self.w] = planes.reshape(-1, self.w)
        else:
            tall = np.ascontiguousarray(planes).reshape(-1, self.w)
        self.din = gpu.DeviceBuffer(tall.nbytes)
        self.din.upload(tall)

    def probe(self, mode, params):
        k = len(params)
        count = self.nplanes * k
        dtot = self.gpu.DeviceBuffer((count + 4) * 8)
        try:
            fill = np.full(count + 4, np.uint64(0xDEADBEEFDEADBEEF))        # garbage where the totals go
            fill[:2] = fill[-2:] = CANARY
            dtot.upload(fill)
            self.gpu.probe_sizes_n_device(self.din.ptr, self.nplanes, self.h, self.w, self.n, MODES[mode], [float(v) for v in params],
                                          dtot.ptr + 16, pitch=self.pitch)
            self.gpu.check(self.gpu.lib().jpegx_stream_synchronize(None))
            raw = dtot.download((count + 4,), np.uint64)
        finally:
            dtot.free()
        assert (raw[:2] == CANARY).all() and (raw[-2:] == CANARY).all(), "the probe wrote outside its totals"
        raw = raw[2:-2].reshape(self.nplanes, k)
        return raw & ~BAD, (raw & BAD) != 0

    def check(self, mode, params, want, want_bad, what=""):
        """Twice in a row: flags equal the oracle's everywhere, sizes wherever no flag stands, and the same raw answer again."""
        got, bad = self.probe(mode, params)
        where = np.argwhere(bad != want_bad)
        assert where.size == 0, "%s N %d %s %r: flags differ at (plane, candidate) %s" % (what, self.n, mode, list(params), where[:8].tolist())
        ok = ~want_bad
        where = np.argwhere((got != want) & ok)
        assert where.size == 0, "%s N %d %s %r: %d sizes differ, first (plane, candidate) %s: got %s for %s" % (
            what, self.n, mode, list(params), len(where), where[:4].tolist(), [int(got[tuple(i)]) for i in where[:4]],
            [int(want[tuple(i)]) for i in where[:4]])
        again, again_bad = self.probe(mode, params)
        assert np.array_equal(again_bad, bad) and np.array_equal(again[ok], got[ok]), "%s N %d: two calls in a row differ" % (what, self.n)
        return got, bad

    def free(self):
        self.din.free()
