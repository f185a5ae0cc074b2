"""The identity the distortion probe over a set rests on, on the NumPy twin alone: for an arbitrary decoded strip s the sum over
a plane's strip elements of S2 - 2 s S1 + cnt s^2 is the squared error of the scatter's pixels (picture_set_model.pixels_twin)
against the picture's own.  CPU only, nothing of the product runs."""
import numpy as np
import pytest

import distortion_model
import distortion_set_model
import picture_set_model


def _sizes(n, bs):
    return [(1, 1), (1, 9), (9, 1), (n * bs, n * bs), (n * bs + 1, n * bs + 1), (2 * n * bs - 1, n * bs + bs + 1), (7, 3 * n * bs + 2)]


@pytest.mark.parametrize("bs", [1, 2, 3, 7])
@pytest.mark.parametrize("n, nbands", [(2, 3), (3, 1), (4, 3), (5, 2)])
def test_the_identity_per_plane(bs, n, nbands):
    sizes = _sizes(n, bs)
    rng = np.random.default_rng([bs, n, nbands])
    pictures = [rng.integers(0, 256, (r, c, nbands), dtype=np.uint8) for r, c in sizes]
    s1, s2, cnt = distortion_set_model.moment_strips(pictures, bs, n)
    decoded = rng.integers(0, 256, s1.shape, dtype=np.uint8)         # arbitrary: padding samples included
    back = picture_set_model.pixels_twin(decoded, sizes, nbands, bs, n)
    want = np.array([((b.astype(np.int64) - p.astype(np.int64)) ** 2).sum(axis=(0, 1)) for b, p in zip(back, pictures)]).reshape(-1)
    got = distortion_set_model.plane_sse(pictures, decoded, bs, n)
    assert got.shape == (len(sizes) * nbands,) and np.array_equal(got, want)
    # live pixels are counted once each, and padding samples carry nothing
    assert int(cnt.sum()) == nbands * sum(r * c for r, c in sizes)
    assert not s1[cnt == 0].any() and not s2[cnt == 0].any()
    assert (cnt <= bs * bs).all()


def test_the_words_and_the_strip_order():
    n, bs = 4, 2
    sizes = [(9, 17), (8, 8), (3, 30)]
    rng = np.random.default_rng(5)
    pictures = [rng.integers(0, 256, (r, c, 2), dtype=np.uint8) for r, c in sizes]
    words = distortion_set_model.moments_twin(pictures, bs, n)
    shapes, nb, first, planes = picture_set_model.table_twin(sizes, 2, bs, n)
    assert words.dtype == np.uint64 and words.shape == (int(first[-1]) * n, n)
    # plane (1, 1): the second band of the 8 x 8 picture is one block of whole tiles
    blk = words.reshape(-1, n, n)[int(planes[3])]
    band = pictures[1][:, :, 1].astype(np.int64)
    tiles = band.reshape(4, 2, 4, 2)
    assert np.array_equal(blk & np.uint64(0xFFFFFFFF), tiles.sum(axis=(1, 3)).astype(np.uint64))
    assert np.array_equal(blk >> np.uint64(32), (tiles ** 2).sum(axis=(1, 3)).astype(np.uint64))
    # the same pictures one at a time give the same words, picture after picture
    alone = np.concatenate([distortion_set_model.moments_twin([p], bs, n) for p in pictures])
    assert np.array_equal(alone, words)
    # equal to distortion_model's plane, block by block
    s1, s2, _ = distortion_model.moments(pictures[0][:, :, 0], bs, n)
    assert np.array_equal(picture_set_model.blocks_of(distortion_model.pack(s1, s2), n).reshape(-1, n), words[:nb[0] * n])


def test_colour_moments_are_of_the_ycbcr_values():
    import colour_model
    rng = np.random.default_rng(9)
    pictures = [rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)]
    got = distortion_set_model.moments_twin(pictures, 1, 4, colour=1)
    want = distortion_set_model.moments_twin([colour_model.rgb_to_ycbcr(p) for p in pictures], 1, 4)
    assert np.array_equal(got, want) and not np.array_equal(got, distortion_set_model.moments_twin(pictures, 1, 4))
