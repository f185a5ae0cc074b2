"""jpegx.batch_probe_distortion_picture_set_n from uint8 pixels: against the round trip of the set codec
(batch_compress_picture_set_n, batch_decompress_picture_set_n) compared with the pictures in NumPy, per candidate; with
group_samples forcing several groups and a lone picture above the limit; with colour; the flag for exactly the bands that cause
it; and a set of one size against batch_probe_distortion_pictures_n.  Every comparison is exact."""
import numpy as np
import pytest

import distortion_model as dm

pytestmark = pytest.mark.gpu

SIZES = [(67, 93), (64, 64), (20, 24), (128, 96), (40, 200), (1, 1), (33, 70)]
DIVISORS = [5.0, 40.0, 1000.0]                       # 255 * 16^2 / 5 codes in 15 bits
CONFIGS = [(1, 4), (1, 16), (2, 12), (3, 5)]


def _pictures(sizes=SIZES, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for p, (r, c) in enumerate(sizes):
        yy, xx = np.mgrid[0:r, 0:c]
        smooth = ((yy * (2 + p) + xx * 3) % 256)[..., None] + np.arange(3) * 30
        out.append((np.where((xx < c // 2)[..., None], smooth, rng.integers(0, 256, (r, c, 3))) % 256).astype(np.uint8))
    return out


def _round_trip(gpu, pictures, bs, n, divisors, colour):
    """int64 [npictures][3][K]: compress set -> decompress set (the coded bands, no conversion back) -> compare."""
    coded = [dm.ycbcr(p) if colour else p for p in pictures]
    sizes = [p.shape[:2] for p in pictures]
    want = np.empty((len(pictures), 3, len(divisors)), np.int64)
    for q, d in enumerate(divisors):
        blobs = gpu.batch_compress_picture_set_n(pictures, bs, n, "divide", d, **({"colour": colour} if colour else {}))
        back = gpu.batch_decompress_picture_set_n(blobs, sizes, bs, n, "divide", d)
        for p, (b, c) in enumerate(zip(back, coded)):
            want[p, :, q] = ((b.astype(np.int64) - c.astype(np.int64)) ** 2).sum(axis=(0, 1))
    return want


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, n", CONFIGS)
def test_the_sums_are_those_of_the_set_codec_round_trip_whatever_the_groups(gpu, bs, n, colour):
    pictures = _pictures()
    want = _round_trip(gpu, pictures, bs, n, DIVISORS, colour)
    table = gpu.picture_set_table(SIZES, 3, bs, n)
    first = table.entries["first"].astype(np.int64)
    samples = ((first[1:] - first[:-1]) * n * n).tolist()
    lone = max(samples)
    # one group; a limit below the largest picture (a lone picture above it, several groups); a limit that holds a few
    for gs in (0, lone - 1, lone + min(samples) + 1, 1):
        sse, bad = gpu.batch_probe_distortion_picture_set_n(pictures, bs, n, "divide", DIVISORS, colour=colour, group_samples=gs)
        assert sse.shape == (len(SIZES), 3, 3) and not bad.any()
        where = np.argwhere(sse.astype(np.int64) != want)
        assert where.size == 0, (bs, n, colour, gs, where[:6].tolist(), sse[tuple(where[0])], want[tuple(where[0])])
    assert (want[:, :, -1] > want[:, :, 0]).any()


def test_the_flag_for_exactly_the_bands_that_cause_it(gpu):
    pictures = [p // 2 for p in _pictures()]              # no pixel above 127: a coefficient reaches 127 * 256 = 2 * 16256
    pictures[1][:16, :16, 1] = 255                         # one block of band 1 of picture 1: DC 65280 under divisors 2 and 3
    pictures[3][16:32, 32:48, 2] = 255                     # and one of band 2 of picture 3
    sse, bad = gpu.batch_probe_distortion_picture_set_n(pictures, 1, 16, "divide", [2.0, 3.0, 64.0], group_samples=40000)
    flagged = np.zeros(bad.shape, bool)
    flagged[1, 1, :2] = flagged[3, 2, :2] = True
    assert np.array_equal(bad, flagged), np.argwhere(bad != flagged).tolist()
    want = _round_trip(gpu, pictures, 1, 16, [64.0], None)
    assert np.array_equal(sse[:, :, 2].astype(np.int64), want[:, :, 0])


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, n", [(1, 4), (2, 12), (5, 24)])
def test_a_set_of_one_size_equals_the_probe_of_a_stack(gpu, bs, n, colour):
    pictures = _pictures([(67, 93)] * 5, seed=4)
    stack, stack_bad = gpu.batch_probe_distortion_pictures_n(np.stack(pictures), bs, n, "divide", DIVISORS, colour=colour)
    for gs in (0, 1):
        sse, bad = gpu.batch_probe_distortion_picture_set_n(pictures, bs, n, "divide", DIVISORS, colour=colour, group_samples=gs)
        assert np.array_equal(sse, stack) and np.array_equal(bad, stack_bad) and not bad.any()
