"""jpegx_picture_set_moments_n against its NumPy twin (tests/distortion_set_model.py), word for word, on the smallest shapes
where the tile clamp, a partial tile, the three store widths (N a multiple of 4, even, odd) and the two prefix searches (LDS up
to 1023 pictures, global memory beyond) can each go wrong.  The strip is pre-filled with 0xFF.. between margins: a word that is
not written, or one written outside the k pictures' blocks, shows."""
import numpy as np
import pytest

import distortion_set_device as dsd
import distortion_set_model as dsm
import picture_set_model as model

pytestmark = pytest.mark.gpu

RAGGED = [(1, 1), (1, 9), (9, 1), (5, 7), (13, 22), (31, 3), (8, 8), (17, 40)]


def _check(gpu, pictures, bs, n, colour=0, layout=None, ranges=((0, None),)):
    d = dsd.PictureSet(gpu, pictures, bs, n, colour, layout)
    try:
        want = dsm.moments_twin(pictures, bs, n, colour).reshape(-1)
        strip_want = model.strip_twin(pictures, bs, n, colour).reshape(-1)
        assert want.size == d.words
        for p0, k in ranges:
            k = d.npictures - p0 if k is None else k
            strip, mom, at = d.gather(p0, k)
            lo = at
            hi = lo + int(d.first[(p0 + k) * d.nbands] - d.first[p0 * d.nbands]) * n * n
            src = slice(int(d.first[p0 * d.nbands]) * n * n, int(d.first[(p0 + k) * d.nbands]) * n * n)
            where = np.flatnonzero(mom[lo:hi] != want[src])
            assert where.size == 0, "N %d bs %d colour %d pictures %d..%d: %d words differ, first at %s: got %s for %s" % (
                n, bs, colour, p0, p0 + k - 1, where.size, where[:4].tolist(), [hex(int(v)) for v in mom[lo:hi][where[:4]]],
                [hex(int(v)) for v in want[src][where[:4]]])
            assert (mom[:lo] == dsd.ONES).all() and (mom[hi:] == dsd.ONES).all(), "a word was written outside the k pictures' blocks"
            # the blocks gather beside it: the same block and element order
            assert np.array_equal(strip[lo:hi], strip_want[src]) and (strip[:lo] == 1e300).all() and (strip[hi:] == 1e300).all()
    finally:
        d.free()


@pytest.mark.parametrize("n", [2, 3, 4, 7, 16, 32])
@pytest.mark.parametrize("bs", [1, 2, 3])
def test_ragged_pictures_of_three_bands(gpu, n, bs):
    pictures = model.noise_pictures(n * 10 + bs, RAGGED, 3)
    _check(gpu, pictures, bs, n, ranges=((0, None), (2, 3), (len(RAGGED) - 1, 1)))


@pytest.mark.parametrize("nbands", [1, 2, 4])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_other_band_counts_and_a_layout_with_slack(gpu, nbands, n):
    pictures = model.noise_pictures(nbands, RAGGED, nbands)
    _check(gpu, pictures, 2, n, layout=model.Layout(RAGGED, nbands, seed=n), ranges=((0, None), (3, 4)))


@pytest.mark.parametrize("n", [2, 3, 4, 16])
def test_colour_and_a_layout_with_slack(gpu, n):
    pictures = model.noise_pictures(77, RAGGED, 3)
    pictures[2] = np.random.default_rng(n).integers(0, 256, pictures[2].shape, dtype=np.uint8)
    _check(gpu, pictures, 3, n, colour=1, layout=model.Layout(RAGGED, 3, seed=1), ranges=((0, None), (1, 5)))


@pytest.mark.parametrize("n", [2, 5, 8])
def test_block_size_255(gpu, n):
    """One tile is 255 x 255 pixels: S1 and S2 reach their largest values, and most tiles are partial or empty."""
    sizes = [(255, 255), (256, 300), (1, 600), (511, 2)]
    pictures = [np.full((r, c, 1), 255, np.uint8) for r, c in sizes]
    pictures[1] = np.random.default_rng(n).integers(0, 256, pictures[1].shape, dtype=np.uint8)
    want = dsm.moments_twin(pictures[:1], 255, n).reshape(-1)
    assert int(want[0]) == ((255 * 255 * 65025) << 32) | (255 * 65025)
    _check(gpu, pictures, 255, n, ranges=((0, None), (1, 2)))


@pytest.mark.parametrize("n", [2, 3])
def test_1025_one_block_pictures_take_the_global_search(gpu, n):
    rng = np.random.default_rng(n)
    sizes = [(int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))) for _ in range(1025)]
    pictures = [rng.integers(0, 256, (r, c, 2), dtype=np.uint8) for r, c in sizes]
    _check(gpu, pictures, 1, n, ranges=((0, None), (1, 1024), (2, 1023)))       # 1024 pictures: global; 1023: the LDS prefix
