"""The NumPy twin of the gather and the scatter of a SET of pictures of unequal sizes (csrc/jpegx_band_set_n.hip), built from
the package's own steps: per picture and band Padding -> SubSampling -> DCTPadding (pipeline/geometry.py), the plane cut into
n x n blocks and the blocks laid behind each other in STRIP order -- picture-major, then band, then block-row-major inside the
band -- and the way back: the strip's blocks put together again, DCTPadding.invert, SubSampling.invert, Padding.invert, np.dstack.
With colour the model pixels are tests/colour_model.py's YCbCr of the input, and its RGB of the output.  A plain helper module
of the suite, like picture_gather_model.py; tests/test_picture_set_model.py holds it against the product-free oracle."""
import numpy as np

import colour_model
import pipeline
from pipeline.geometry import DCTPadding, Padding, SubSampling


def config_of(rows, cols, bs, n):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n)


def model_of(pixels, colour):
    return colour_model.rgb_to_ycbcr(pixels) if colour else np.asarray(pixels)


def plane_of(band, bs, n):
    """float64 [H][W]: steps 0-2 of the package on one band (step 3 is the identity)."""
    cfg = config_of(band.shape[0], band.shape[1], bs, n)
    return np.asarray(DCTPadding(cfg).execute(SubSampling(cfg).execute(Padding(cfg).execute(band))), np.float64)


def blocks_of(plane, n):
    """[H][W] -> [nb][n][n], block-row-major."""
    h, w = plane.shape
    return plane.reshape(h // n, n, w // n, n).transpose(0, 2, 1, 3).reshape(-1, n, n)


def plane_from_blocks(blocks, h, w, n):
    return blocks.reshape(h // n, w // n, n, n).transpose(0, 2, 1, 3).reshape(h, w)


def strip_twin(pictures, bs, n, colour=0):
    """A list of uint8 [rows_p][cols_p][nb] -> float64 [nblk * n][n], the block strip of the gather."""
    out = []
    for px in pictures:
        model = model_of(px, colour)
        for k in range(model.shape[2]):
            out.append(blocks_of(plane_of(np.ascontiguousarray(model[:, :, k]), bs, n), n))
    return np.concatenate(out).reshape(-1, n)


def shapes_of(sizes, bs, n):
    return [pipeline._blocked_shape(r, c, bs, n) for r, c in sizes]


def pixels_twin(strip, sizes, nbands, bs, n, colour=0):
    """uint8 [nblk * n][n] and the pictures' (rows, cols) -> a list of uint8 [rows_p][cols_p][nbands], the scatter."""
    blocks = np.asarray(strip).reshape(-1, n, n)
    out, at = [], 0
    for (rows, cols), (h, w) in zip(sizes, shapes_of(sizes, bs, n)):
        cfg = config_of(rows, cols, bs, n)
        nb = (h // n) * (w // n)
        bands = []
        for _ in range(nbands):
            plane = plane_from_blocks(blocks[at:at + nb], h, w, n)
            at += nb
            bands.append(Padding(cfg).invert(SubSampling(cfg).invert(DCTPadding(cfg).invert(plane))))
        px = np.ascontiguousarray(np.dstack(bands))
        out.append(colour_model.ycbcr_to_rgb(px) if colour else px)
    assert at == blocks.shape[0]
    return out


def table_twin(sizes, nbands, bs, n):
    """(shapes, blocks per band, first block of every picture and the total behind them, first block of every plane and the
    total) restated from pipeline._blocked_shape."""
    shapes = shapes_of(sizes, bs, n)
    nb = [(h // n) * (w // n) for h, w in shapes]
    first = np.concatenate([[0], np.cumsum([nbands * b for b in nb])]).astype(np.int64)
    planes = np.array([first[p] + k * nb[p] for p in range(len(sizes)) for k in range(nbands)] + [first[-1]], np.int64)
    return shapes, nb, first, planes


def noise_pictures(seed, sizes, nbands):
    """Picture p is noise of a narrow range around its own level (a clamp that reaches a neighbour shows), every third one
    full-range noise."""
    rng = np.random.default_rng(seed)
    out = []
    for p, (r, c) in enumerate(sizes):
        if p % 3 == 2:
            out.append(rng.integers(0, 256, (r, c, nbands), dtype=np.uint8))
        else:
            out.append((rng.integers(0, 6, (r, c, nbands), dtype=np.uint8) + np.uint8(10 + (37 * p) % 200)))
    return out


class Layout:
    """Pictures at unaligned offsets with odd pitches in one buffer: ``offsets``, ``pitches``, ``nbytes``; ``pack`` writes the
    pictures into a buffer filled with ``fill`` and ``unpack`` reads them back with a mask of the bytes that are pixels."""

    def __init__(self, sizes, nbands, seed=0, lead=3):
        rng = np.random.default_rng([seed, len(sizes)])
        self.sizes, self.nbands = list(sizes), nbands
        self.pitches, self.offsets, at = [], [], lead
        for r, c in self.sizes:
            pitch = c * nbands + int(rng.integers(0, 8))
            self.pitches.append(pitch)
            self.offsets.append(at)
            at += r * pitch + int(rng.integers(0, 23))       # a gap between pictures
        self.nbytes = at

    def pack(self, pictures, fill):
        buf = np.full(self.nbytes, fill, np.uint8)
        for px, o, q in zip(pictures, self.offsets, self.pitches):
            r, c, nb = px.shape
            rows = np.lib.stride_tricks.as_strided(buf[o:], (r, c * nb), (q, 1))
            rows[:] = px.reshape(r, c * nb)
        return buf

    def unpack(self, buf):
        mask = np.zeros(self.nbytes, bool)
        out = []
        for (r, c), o, q in zip(self.sizes, self.offsets, self.pitches):
            w = c * self.nbands
            out.append(np.lib.stride_tricks.as_strided(buf[o:], (r, w), (q, 1)).reshape(r, c, self.nbands).copy())
            np.lib.stride_tricks.as_strided(mask[o:], (r, w), (q, 1))[:] = True
        return out, mask
