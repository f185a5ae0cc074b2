"""The NumPy twin of jpegx_picture_planes_stacked_u8 (csrc/jpegx_picture_u8.hip), the front of the dct_size-8 picture
batch: pictures [k][rows][cols][nb] -> padded raw uint8 planes [k][nb][H * bs][W * bs],

    plane (p, k)[y][x] = model_p[src_y[y]][src_x[x]][k],    src = jpegx.edge_source_indices per axis,

model_p picture p itself or, with colour, tests/colour_model.py's YCbCr of it.  A plain helper module of the suite, like
fenced.py; tests/test_picture_gather_model.py pins it to the reference's steps 0-3 without a device."""
import numpy as np

import colour_model
import jpegx


def model_of(pixels, colour):
    return colour_model.rgb_to_ycbcr(pixels) if colour else np.asarray(pixels)


def planes_twin(pixels, bs, colour=0):
    px = np.asarray(pixels)
    assert px.ndim == 4 and px.dtype == np.uint8
    model = model_of(px, colour)
    sy, sx = jpegx.edge_source_indices(px.shape[1], bs), jpegx.edge_source_indices(px.shape[2], bs)
    return np.ascontiguousarray(model[:, sy][:, :, sx].transpose(0, 3, 1, 2))


def mean_pooled(planes, bs):
    """[..., H * bs, W * bs] uint8 -> float64 [..., H, W]: the exact integer sum of every bs x bs tile, divided once."""
    a = np.asarray(planes)
    hh, ww = a.shape[-2:]
    tiles = a.reshape(a.shape[:-2] + (hh // bs, bs, ww // bs, bs)).astype(np.int64)
    return tiles.sum(axis=(-3, -1)).astype(np.float64) / float(bs * bs)


def distinct_pictures(seed, k, rows, cols, nb):
    """uint8 [k][rows][cols][nb]: picture p is noise of a narrow range around its own level, so that a clamp that reaches
    into the neighbouring picture -- or the pitch gap, which the tests fill with another value still -- shows."""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 6, (k, rows, cols, nb), dtype=np.uint8)
    for p in range(k):
        px[p] += np.uint8(10 + (37 * p) % 200)
    return px
