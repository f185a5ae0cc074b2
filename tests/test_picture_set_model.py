"""The NumPy twin of the picture set's gather and scatter (tests/picture_set_model.py) held against the product-free oracle
without a device: every plane of the strip is codec_oracle_n.pre_transform of the model's band cut into blocks in strip order,
and the scatter twin of a strip is np.repeat + crop + np.dstack of its planes.  The GPU tests compare the kernels against this
twin.  Every comparison is exact.  CPU only."""
import numpy as np
import pytest

import codec_oracle_n as on
import colour_model
from picture_set_model import Layout, blocks_of, model_of, noise_pictures, pixels_twin, plane_from_blocks, strip_twin, table_twin

SIZES = [(1, 1), (7, 19), (13, 5), (1, 40), (33, 2), (20, 20)]


@pytest.mark.parametrize("colour", [0, 1])
@pytest.mark.parametrize("bs", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [2, 3, 5, 12])
def test_the_strip_is_the_oracles_planes_in_strip_order(n, bs, colour):
    pictures = noise_pictures([n, bs], SIZES, 3)
    strip = strip_twin(pictures, bs, n, colour)
    shapes, nb, first, planes = table_twin(SIZES, 3, bs, n)
    assert strip.shape == (first[-1] * n, n) and strip.dtype == np.float64
    blocks = strip.reshape(-1, n, n)
    for p, px in enumerate(pictures):
        model = model_of(px, colour)
        for k in range(3):
            want = on.pre_transform(model[:, :, k], bs, n)
            assert want.shape == shapes[p]
            at = planes[3 * p + k]
            assert at == first[p] + k * nb[p]
            assert np.array_equal(plane_from_blocks(blocks[at:at + nb[p]], *shapes[p], n), want), (p, k)
            # block b of the band is rows by * n .., columns bx * n .. of the plane
            wb = shapes[p][1] // n
            b = nb[p] - 1
            assert np.array_equal(blocks[at + b], want[(b // wb) * n:(b // wb + 1) * n, (b % wb) * n:(b % wb + 1) * n])


@pytest.mark.parametrize("colour", [0, 1])
@pytest.mark.parametrize("bs", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [2, 5, 12])
def test_the_scatter_twin_replicates_crops_and_stacks(n, bs, colour):
    shapes, nb, first, _ = table_twin(SIZES, 3, bs, n)
    strip = np.random.default_rng([n, bs, colour]).integers(0, 256, (first[-1] * n, n), dtype=np.uint8)
    got = pixels_twin(strip, SIZES, 3, bs, n, colour)
    blocks = strip.reshape(-1, n, n)
    for p, (rows, cols) in enumerate(SIZES):
        planes = [plane_from_blocks(blocks[first[p] + k * nb[p]:first[p] + (k + 1) * nb[p]], *shapes[p], n) for k in range(3)]
        want = np.dstack([np.repeat(np.repeat(q, bs, 0), bs, 1)[:rows, :cols] for q in planes])
        if colour:
            want = colour_model.ycbcr_to_rgb(want)
        assert got[p].dtype == np.uint8 and got[p].shape == (rows, cols, 3)
        assert np.array_equal(got[p], want), p


def test_blocks_and_back_and_the_layout_helper():
    plane = np.arange(6 * 9, dtype=np.float64).reshape(6, 9)
    blocks = blocks_of(plane, 3)
    assert blocks.shape == (6, 3, 3) and np.array_equal(blocks[4], plane[3:6, 3:6])
    assert np.array_equal(plane_from_blocks(blocks, 6, 9, 3), plane)
    pictures = noise_pictures(1, SIZES, 3)
    lay = Layout(SIZES, 3, seed=4)
    buf = lay.pack(pictures, 0xEE)
    back, mask = lay.unpack(buf)
    assert all(np.array_equal(a, b) for a, b in zip(back, pictures))
    assert mask.sum() == sum(r * c * 3 for r, c in SIZES) and np.all(buf[~mask] == 0xEE)
    assert any(o % 4 for o in lay.offsets) and any(q % 2 for q in lay.pitches)
