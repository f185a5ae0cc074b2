"""jpegx_probe_distortion_set_n against the road it stands for, run once per candidate on the same strip
(tests/distortion_set_device.py: jpegx_forward_fused_n on the strip, jpegx_inverse_fused_n with the uint8 clamp,
jpegx_picture_set_pixels_u8, NumPy against the pixels).  Every comparison is exact, and no cell may be flagged unless the case
says which: the pictures are as bright as dct_size allows without an amplitude beyond 16383 under a divisor of magnitude 1
or more; under fractions the flags are the yardstick's, cell for cell.

The sets are built for what the ragged kernel adds -- the plane of a block and the block's place and band size from the table:
single-band pictures whose planes hold 1, 1, 1, 6, 35, 1, 2, 64, 65 and 3 blocks of unlike widths in blocks (one block across,
the whole band across), with crops that differ per picture, and pictures of three bands.  At dct_size 2 one turn of 64 blocks
holds the first five planes and a part of the sixth; from dct_size 16 on a turn is one block."""
import numpy as np
import pytest

import distortion_device
import distortion_set_device as dsd

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 4, 7, 9, 16, 17, 24, 32]
SHAPES = [(1, 1), (1, 1), (1, 1), (2, 3), (5, 7), (1, 1), (2, 1), (8, 8), (65, 1), (1, 3)]      # blocks down x across
COUNTS = [1, 1, 1, 6, 35, 1, 2, 64, 65, 3]
SHAPES3 = [(1, 2), (1, 1), (7, 1), (5, 8), (1, 1)]       # per band; three bands a picture
COUNTS3 = [2, 1, 7, 40, 1]
MANY = [float(v) for v in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128, 160, 200, 256, 300, 400, 512, 640, 800,
                           1000, 2000, 4096, 100000)]


def _crops(shapes, n, bs, seed):
    rng = np.random.default_rng([seed, n, bs])
    return [(int(rng.integers(0, n * bs)), int(rng.integers(0, n * bs))) for _ in shapes]


def _peak(n):
    """The brightest pixel with which no coefficient of an n x n block passes 16383 under a divisor of magnitude 1 or more (a
    coefficient reaches peak * n * n)."""
    return min(255, 16383 // (n * n))


def _pictures(sizes, nbands, seed, peak=255):
    """Smooth ramps with noise on one half, pixels 0 .. peak: coefficients of every size, and pictures unlike each other."""
    rng = np.random.default_rng(seed)
    out = []
    for p, (r, c) in enumerate(sizes):
        yy, xx = np.mgrid[0:r, 0:c]
        smooth = yy * (3 + p) + xx * 2 + 31 * p
        noise = rng.integers(0, peak + 1, (r, c, nbands))
        out.append((np.where((xx < max(c // 2, 1))[..., None], smooth[..., None] + np.arange(nbands) * 20, noise) % (peak + 1)).astype(np.uint8))
    return out


def _single(gpu, n, bs=1, seed=0):
    sizes = dsd.sizes_for(SHAPES, n, bs, _crops(SHAPES, n, bs, seed))
    return dsd.PictureSet(gpu, _pictures(sizes, 1, seed, _peak(n)), bs, n)


def _triple(gpu, n, bs=1, seed=1):
    sizes = dsd.sizes_for(SHAPES3, n, bs, _crops(SHAPES3, n, bs, seed))
    return dsd.PictureSet(gpu, _pictures(sizes, 3, seed, _peak(n)), bs, n)


@pytest.fixture(scope="module", params=SIZES)
def sets(request, gpu):
    n = request.param
    bs = 1 + SIZES.index(n) % 3                          # block sizes 1, 2, 3 in turn
    devs = [_single(gpu, n, bs), _triple(gpu, n, 1 + (bs % 3))]
    assert devs[0].counts().tolist() == COUNTS and devs[1].counts().tolist() == np.repeat(COUNTS3, 3).tolist()
    wbs = devs[0].table.entries["wb"][:-1].tolist()
    assert wbs == [wb for _, wb in SHAPES] and 1 in wbs
    yield n, devs
    for d in devs:
        d.free()


def test_divide_candidates(sets):
    n, devs = sets
    for d in devs:
        d.check("divide", [40.0], label="K 1")
        got = d.check("divide", [1.0, 2.0, 3.0, 40.0, 1000.0], label="K 5")       # power-of-two and true-division paths side by side
        assert (got[:, -1] > got[:, 0]).any()


def test_thirty_two_candidates_and_the_same_value_twice(sets):
    n, devs = sets
    assert len(MANY) == 32
    devs[0].check("divide", MANY, label="K 32")
    got = devs[1].check("divide", [40.0, 3.0, 40.0])
    assert np.array_equal(got[:, 0], got[:, 2])


def test_signed_powers_of_two_and_fractions(sets):
    n, devs = sets
    for d in devs:
        d.check("divide", [-2.0, 4.0, -64.0, 0.5], expect_bad=dsd.ANY, label="2^e")
        d.check("divide", [2.5, 1.0 / 3.0, -7.25, 0.3], expect_bad=dsd.ANY, label="fractions")


def test_discard_edges_and_none(sets):
    n, devs = sets
    for d in devs:
        got = d.check("discard", [0.0, 1.0, float(n), float(n + 1)])
        assert np.array_equal(got[:, 2], got[:, 3])
        none = d.check("none", [0.0])
        assert np.array_equal(none[:, 0], got[:, 2])      # keeping everything is 'none'


def test_sub_ranges_write_their_own_rows_only(sets):
    """p0 > 0 and k < npictures: row 0 is band 0 of picture p0, k * nbands rows are written (over garbage), the canaries in front
    of and behind them stay (PictureSet.probe)."""
    n, devs = sets
    for d in devs:
        for p0, k in ((1, 1), (2, 3), (3, d.npictures - 3), (0, 2), (d.npictures - 1, 1)):
            d.check("divide", [3.0, 40.0], p0, k)
    devs[0].check("divide", MANY[:7], 4, 5)                              # the 35-block plane first, the 64 and 65 behind it


@pytest.mark.parametrize("n", [2, 4, 16])
def test_bit_63_for_exactly_one_plane_of_one_block(gpu, n):
    """One flat block of DC 20000.3 as the second of the three one-block planes: at dct_size 2 it shares a turn with clean
    blocks of five planes.  Bit 63 for exactly (plane 1, divisor 1); every other total exact, plane 1 under divisor 1000 among
    them."""
    d = _single(gpu, n)
    try:
        strip, _, at = d.gather()
        strip = strip[dsd.MARGIN:-dsd.MARGIN].reshape(-1, n).copy()
        strip[n:2 * n] = 20000.3 / (n * n)
        d.free()
        d = dsd.PictureSet(gpu, d.pictures, 1, n, strip=strip)
        want, want_bad = d.road("divide", [1.0, 1000.0])
        assert np.argwhere(want_bad).tolist() == [[1, 0]]
        d.check("divide", [1.0, 1000.0], expect_bad=[(1, 0)])
        d.check("divide", [1.0, 1000.0], 1, 2, expect_bad=[(1, 0)])
        d.check("divide", [1.0, 1000.0], 2, 4)
    finally:
        d.free()


def test_explicit_device_form(gpu):
    d = _triple(gpu, 4)
    try:
        d.gather(device=0)
        got, bad = d.probe("divide", [3.0, 40.0], 1, 3, device=0)
        want, want_bad = d.road("divide", [3.0, 40.0])
        assert not bad.any() and not want_bad.any() and np.array_equal(got, want[3:12])
    finally:
        d.free()


@pytest.mark.parametrize("n, bs", [(2, 1), (7, 2), (17, 3)])
def test_a_set_of_equal_pictures_gives_the_totals_of_the_equal_size_probe(gpu, n, bs):
    rows, cols = 2 * n * bs - 1, 3 * n * bs - bs - 1         # planes of 2 x 3 blocks, ragged crops
    pictures = _pictures([(rows, cols)] * 4, 3, seed=2, peak=_peak(n))
    d = dsd.PictureSet(gpu, pictures, bs, n)
    bands = np.ascontiguousarray(np.stack([p[:, :, k] for p in pictures for k in range(3)]))
    s = distortion_device.Stack(gpu, bands, bs, n)
    try:
        equal, equal_bad = s.probe("divide", [1.0, 3.0, 40.0])
        got = d.check("divide", [1.0, 3.0, 40.0])
        assert not equal_bad.any() and np.array_equal(got, equal)
    finally:
        s.free()
        d.free()
