"""jpegx_probe_sizes_set_n against tests/codec_oracle_n.py.  Every comparison is exact.

tests/test_gpu_probe_set_kernel_n.py measures the ragged probe with the device road it stands for; here the yardstick is the
extended-precision oracle on planes of UNLIKE block shapes, built off the rounding ties (probe_oracle.distinct_planes: what is
asserted of every cell before it is compared -- a failing premise means another seed, never a mask) and arranged by hand into
the block strip: plane after plane, each plane's blocks row-major, block g in rows g * N .. g * N + N - 1.  The oracle sees
each plane as the picture's band it is; the probe sees only the strip and the table's array of first blocks."""
import numpy as np
import pytest

import probe_oracle as po
import probe_set_device as psd

pytestmark = pytest.mark.gpu

SIZES = [2, 5, 8, 11, 16, 31]
# blocks (rows, columns) of the single-band pictures: one-block planes between larger ones, a tall one, a wide one
SHAPES = [(1, 1), (2, 3), (1, 1), (5, 7), (3, 1), (1, 4), (1, 1), (2, 2)]
SHAPES3 = [(1, 2), (3, 3), (1, 1)]                     # pictures of three bands
DIVISORS = [1, 3, 40, 64, -3, 0.75, 1000, 2.0 ** -20]
SATURATING = DIVISORS.index(2.0 ** -20)


def _planes(n, shapes, per_picture=1):
    """One plane per band of every picture: plane i is the (i mod 7)-th of probe_oracle.distinct_planes at its own shape, so the
    kinds (noise at five amplitudes, all zero, smooth) cycle over unlike shapes."""
    out = []
    for p, (hb, wb) in enumerate(shapes):
        for b in range(per_picture):
            i = p * per_picture + b
            out.append(po.distinct_planes(n, hb, wb, 7, seed=i)[i % 7])
    return out


def _set(gpu, n, shapes, nbands):
    planes = _planes(n, shapes, nbands)
    strip = np.concatenate([psd.strip_of(p, n) for p in planes])
    d = psd.SetStrip(gpu, strip, [(hb * n, wb * n) for hb, wb in shapes], nbands, n)
    assert d.counts().tolist() == [hb * wb for hb, wb in shapes for _ in range(nbands)]
    return planes, d


@pytest.mark.parametrize("n", SIZES)
def test_unlike_planes_against_the_oracle(gpu, n):
    for shapes, nbands in ((SHAPES, 1), (SHAPES3, 3)):
        planes, d = _set(gpu, n, shapes, nbands)
        blocks = d.counts().astype(np.uint64)
        zero = [i for i in range(len(planes)) if i % 7 == 1]
        try:
            want, want_bad = po.expected(planes, n, "divide", DIVISORS)
            # the tiny divisor flags every plane but the all-zero ones, and nothing else is flagged
            assert want_bad[:, SATURATING].sum() == len(planes) - len(zero) and not np.delete(want_bad, SATURATING, axis=1).any()
            assert (want[zero] == blocks[zero, None]).all()
            d.check("divide", DIVISORS, want=(want, want_bad), expect_bad=[tuple(c) for c in np.argwhere(want_bad)])
            d.check("divide", DIVISORS[:4], 1, len(shapes) - 2, want=(want[:, :4], want_bad[:, :4]))
            keeps = [0, 1, n, n + 3]
            want, want_bad = po.expected(planes, n, "discard", keeps)
            assert not want_bad.any() and (want[:, 0] == blocks).all() and np.array_equal(want[:, 2], want[:, 3])
            d.check("discard", keeps, want=(want, want_bad))
            want, want_bad = po.expected(planes, n, "none", [0.0])
            assert not want_bad.any()
            d.check("none", [0.0], want=(want, want_bad))
        finally:
            d.free()


@pytest.mark.parametrize("n", [2, 5])
def test_the_flag_lands_on_the_plane_of_its_block(gpu, n):
    """A checkerboard of +-150000 / N^2 on the lone block of plane 2, between the last block of plane 1 and the first of plane 3
    in one wave step: its highest coefficient passes 15 bits under 1 and -3 and stays inside them under 40 and 1000.  The oracle
    names the cells; the probe flags exactly those and every other total is exact."""
    planes = _planes(n, SHAPES)
    yy, xx = np.mgrid[0:n, 0:n]
    planes[2] = planes[2] + 150000.0 / (n * n) * (-1.0) ** (yy + xx)
    divisors = [1.0, 40.0, -3.0, 1000.0]
    want, want_bad = po.expected(planes, n, "divide", divisors)
    assert np.argwhere(want_bad).tolist() == [[2, 0], [2, 2]]
    strip = np.concatenate([psd.strip_of(p, n) for p in planes])
    d = psd.SetStrip(gpu, strip, [(hb * n, wb * n) for hb, wb in SHAPES], 1, n)
    try:
        d.check("divide", divisors, want=(want, want_bad), expect_bad=[(2, 0), (2, 2)])
    finally:
        d.free()
