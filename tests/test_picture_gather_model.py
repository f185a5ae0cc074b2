"""The contract of jpegx_picture_planes_stacked_u8 held against the reference without a device: the NumPy twin of the gather
(tests/picture_gather_model.py, built from jpegx.edge_source_indices and tests/colour_model.py), mean-pooled over
block_size x block_size tiles, is the plane that enters the DCT -- codec_oracle.pre_transform of the model's band, i.e.
Padding, SubSampling, DCTPadding and Normalization of the reference.  Every comparison is exact.  CPU only."""
import numpy as np
import pytest

import codec_oracle
import jpegx
from picture_gather_model import distinct_pictures, mean_pooled, model_of, planes_twin

SHAPES = [(1, 17), (29, 1), (23, 41), (9, 130)]
BLOCK_SIZES = [1, 2, 3, 4, 5, 7]


@pytest.mark.parametrize("colour", [0, 1])
@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("rows,cols", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_pooled_twin_is_the_plane_that_enters_the_dct(rows, cols, bs, colour):
    k, nb = 2, 3
    px = np.random.default_rng([rows, cols, bs]).integers(0, 256, (k, rows, cols, nb), dtype=np.uint8)
    twin = planes_twin(px, bs, colour)
    h, w = jpegx.padded_shape(rows, cols, bs)
    assert twin.shape == (k, nb, h * bs, w * bs) and twin.dtype == np.uint8
    pooled = mean_pooled(twin, bs)
    model = model_of(px, colour)
    for p in range(k):
        for b in range(nb):
            want = codec_oracle.pre_transform(model[p][:, :, b], bs)
            assert want.shape == (h, w)
            assert np.array_equal(pooled[p, b], want), (rows, cols, bs, colour, p, b)


def test_the_twin_keeps_every_picture_to_itself():
    """Pictures of distinct levels: every sample of plane (p, k) lies in picture p's own range, the top left corner is the
    picture, and the order is picture-major."""
    px = distinct_pictures(3, 4, 9, 17, 3)
    twin = planes_twin(px, 4)
    for p in range(4):
        lo = 10 + (37 * p) % 200
        assert twin[p].min() >= lo and twin[p].max() <= lo + 5
        for b in range(3):
            assert np.array_equal(twin[p, b, :9, :17], px[p, :, :, b])
