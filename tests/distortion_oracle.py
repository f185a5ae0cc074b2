"""The bands on which the distortion probe is held against tests/codec_oracle_n.py, and what the oracle says about them.

One band per 'free' cell of codec_oracle_n.matrix_cases() (every N, block size, shape and quantiser of that matrix: 'none',
'discard' and 'divide'), probed with K = 1 under the quantiser the band was built for.  The comparison can only be exact where
the oracle's extended-precision values leave one admissible integer on both ways: no coefficient within Forward.tau of a
half-integer, no decoded sample within tau_inv of one.  make_band keeps the rational coefficients off the ties and carries the
seeds of the bands whose seed-0 version lands on one after all; every cell as it comes from there is clear on both ways, which
tests/test_distortion_oracle_inputs.py asserts on the oracle's values alone.

The way back is codec_oracle_n.Inverse for every quantiser but 'divide' with a divisor that is no whole number (0.75): the
reference stores the restored coefficients into an integer array and so truncates them, which jpegx_inverse_fused_n -- the road
jpegx_probe_distortion_n is defined by -- does not (pipeline._whole_divisor keeps such divisors off every device road).  For that
divisor the oracle's own pieces are put together without the truncation: idct_plane(k * d), tau_inv_plane, the clamp, rint, grow."""
import functools

import numpy as np

import codec_oracle_n as co


def cells():
    return [c[:5] for c in co.matrix_cases() if c[5] == "free"]


class Cell:
    """band int64 (h, w); distance, tau: the forward margin; ties: how many decoded samples lie on a tie; sse: the oracle's
    sum of squared differences between the band and its decoded self."""

    def __init__(self, n, bs, mode, param, shape):
        self.key = (n, bs, mode, param, shape)
        self.band, peak = co.make_band(n, bs, mode, param, shape, "free")
        h, w = self.band.shape
        f = co.Forward(self.band, bs, n, mode, param, peak=peak)
        self.distance, self.tau = f.distance, f.tau
        if mode != "divide" or param == np.trunc(param):
            inv = co.Inverse(f.blob(), h, w, bs, n, mode, param)
            assert np.array_equal(inv.zz, f.k_stream)
            ties, back = inv.ties, inv.band
        else:
            f.blob()                                           # the stream exists: no amplitude beyond 15 bits
            restored = f.k.astype(np.float64) * float(param)
            clipped = np.clip(co.idct_plane(restored, n), co.LD(0), co.LD(255))
            ties = np.abs(clipped - np.floor(clipped) - co.LD(0.5)) <= co.tau_inv_plane(restored, n)
            back = co.grow(np.rint(clipped).astype(np.int64), h, w, bs)
        self.ties = int(np.count_nonzero(ties))
        self.sse = int(((back - self.band) ** 2).sum())
        self.band.setflags(write=False)


@functools.lru_cache(maxsize=None)
def cell(n, bs, mode, param, shape):
    return Cell(n, bs, mode, param, shape)
