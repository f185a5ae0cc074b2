"""The identity the distortion probe rests on, on tests/distortion_model.py alone: for every band shape and block size the
squared error of the grown plane against the band equals the sum of S2 - 2 s S1 + cnt s^2 over the plane's samples, exactly, for
random decoded planes -- the samples of both paddings (no live pixel) included, whose term must be 0 whatever they hold.  CPU
only."""
import numpy as np
import pytest

import distortion_model as dm

BLOCK_SIZES = [1, 2, 3, 7, 255]
SHAPES = ["ragged", "exact", "row", "col", "one"]


def _band_shape(shape, bs, n):
    if shape == "one":
        return 1, 1
    if shape == "row":
        return 1, (2 * n + 1) * bs - (1 if bs > 1 else 0)
    if shape == "col":
        return (2 * n + 1) * bs - (bs - 1), 1
    if shape == "exact":
        return (2 * n * bs, 3 * n * bs) if bs < 255 else (n * bs, n * bs)
    # ragged: the last tile is partial (Padding) and the pooled band is no multiple of N (DCTPadding), on both axes
    return (n + 1) * bs - (bs - 1), (2 * n - 1) * bs - (1 if bs > 1 else 0)


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_squared_error_from_moments(bs, shape, n):
    rows, cols = _band_shape(shape, bs, n)
    rng = np.random.default_rng([bs, SHAPES.index(shape), n])
    band = rng.integers(0, 256, (rows, cols))
    s1, s2, cnt = dm.moments(band, bs, n)
    h, w = dm.blocked_shape(rows, cols, bs, n)
    assert s1.shape == (h, w) and h % n == 0 and w % n == 0
    assert int(cnt.sum()) == rows * cols and int(s1.sum()) == int(band.sum()) and int(s2.sum()) == int((band * band).sum())
    assert int(cnt.max()) <= bs * bs and int(s1.max()) < 2 ** 24 and int(s2.max()) < 2 ** 32
    if shape in ("ragged", "row", "col", "one"):
        assert (cnt == 0).any(), "no sample of a padding"
    if shape == "ragged" and bs > 1:
        assert ((cnt > 0) & (cnt < bs * bs)).any(), "no partial tile"
    dead = cnt == 0
    assert not s1[dead].any() and not s2[dead].any()
    for trial in range(3):
        plane = rng.integers(0, 256, (h, w))
        assert dm.sse_direct(band, plane, bs) == dm.sse_moments(s1, s2, cnt, plane)
    for level in (0, 255):
        plane = np.full((h, w), level)
        assert dm.sse_direct(band, plane, bs) == dm.sse_moments(s1, s2, cnt, plane)
    # the packed word holds both moments
    word = dm.pack(s1, s2)
    assert np.array_equal(word & np.uint64(0xFFFFFFFF), s1.astype(np.uint64)) and np.array_equal(word >> np.uint64(32), s2.astype(np.uint64))


def test_the_extremes_fit_their_fields():
    band = np.full((255 * 2, 255 * 2), 255)
    s1, s2, cnt = dm.moments(band, 255, 2)
    assert int(s1.max()) == 255 * 65025 < 2 ** 24 and int(s2.max()) == 65025 * 65025 < 2 ** 32 and int(cnt.max()) == 65025
    assert dm.sse_moments(s1, s2, cnt, np.zeros((2, 2), np.int64)) == 4 * 65025 * 65025
