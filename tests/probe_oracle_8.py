"""What the dct_size-8 probes must answer, composed from the checker's functions (oracle/jpegx_oracle.c) and NumPy alone.

A plain helper module of the suite, not a conftest.  It imports only ``numpy`` and ``oracle``: nothing of the product, so a
mistake the product's roads share cannot hide in it.  It is pinned to the reference itself by tests/golden/probe8.npz
(tests/test_probe_oracle_8.py): len(Jpeg.compress) and the per-band squared error of Jpeg.decompress on 37 x 53 pictures.

Sizes:       the host steps' plane (edge padding, oracle.mean_pool, edge padding to 8) -> oracle.dct_plane -> quant_plane ->
             zigzag_plane -> len(oracle.rle_bytestream); an amplitude beyond 15 bits (|value| > 16383) is the reference's
             BadRleCodeError and comes back as ``bad``.
Distortion:  those integers -> oracle.restore_plane -> idct_plane(rounded=True) -> the clamp to 0..255 -> every sample
             block_size x block_size times, cropped to the band -> the sum of squared differences with the band.

The 8 x 8 roads are exact, rounding ties included, so nothing here avoids ties.
"""
import numpy as np

import oracle

MAX_AMPLITUDE = 16383


def _edge_pad(a, factor):
    """util.pad_array: replicate the last column and the last row up to a multiple of factor."""
    h, w = a.shape
    return np.pad(a, ((0, -h % factor), (0, -w % factor)), mode="edge")


def band_plane(band, bs):
    """Steps 0-3 forward: the float64 plane of whole 8 x 8 blocks that enters the DCT."""
    a = np.asarray(band).astype(np.float64)
    if bs > 1:
        a = oracle.mean_pool(_edge_pad(a, bs), bs)
    return _edge_pad(a, 8)


def band_moments(band, bs):
    """uint64 [H][W] beside band_plane: S2 << 32 | S1 over the band's pixels behind every sample, 0 where there are none."""
    v = np.asarray(band).astype(np.int64)
    rows, cols = v.shape
    h, w = band_plane(band, bs).shape
    s1 = np.zeros((h * bs, w * bs), np.int64)
    s1[:rows, :cols] = v
    s2 = s1 * s1
    s1 = s1.reshape(h, bs, w, bs).sum(axis=(1, 3))
    s2 = s2.reshape(h, bs, w, bs).sum(axis=(1, 3))
    return (s2.astype(np.uint64) << np.uint64(32)) | s1.astype(np.uint64)


def _quantised(plane, mode, param):
    """(int64 (H/8, W/8, 64) zigzag stream, bad) of one float64 plane."""
    zz = oracle.zigzag_plane(oracle.quant_plane(oracle.dct_plane(plane), mode, param))
    return zz, bool(np.abs(zz).max() > MAX_AMPLITUDE)


def plane_sizes(planes, mode, params):
    """(sizes int64 [nplanes][K], bad bool [nplanes][K]) of float64 planes [nplanes][H][W]; a bad entry's size is 0."""
    sizes = np.zeros((len(planes), len(params)), np.int64)
    bad = np.zeros(sizes.shape, bool)
    for p, plane in enumerate(planes):
        for q, param in enumerate(params):
            zz, bad[p, q] = _quantised(plane, mode, param)
            if not bad[p, q]:
                sizes[p, q] = len(oracle.rle_bytestream(zz.astype(np.int16)))
    return sizes, bad


def band_sizes(bands, bs, mode, params):
    """plane_sizes of the bands' planes: bands is a sequence of 2-D integer arrays of one shape."""
    return plane_sizes([band_plane(b, bs) for b in bands], mode, params)


def band_sse(bands, bs, mode, params):
    """(sse int64 [nbands][K], bad bool [nbands][K]): the squared error of the decoded band; a bad entry's sum is 0."""
    sse = np.zeros((len(bands), len(params)), np.int64)
    bad = np.zeros(sse.shape, bool)
    for p, band in enumerate(bands):
        v = np.asarray(band).astype(np.int64)
        rows, cols = v.shape
        plane = band_plane(v, bs)
        for q, param in enumerate(params):
            zz, bad[p, q] = _quantised(plane, mode, param)
            if bad[p, q]:
                continue
            rec = oracle.idct_plane(oracle.restore_plane(oracle.unzigzag_plane(zz), mode, param), rounded=True)
            back = np.repeat(np.repeat(np.clip(rec, 0, 255), bs, 0), bs, 1)[:rows, :cols]
            sse[p, q] = ((back - v) ** 2).sum()
    return sse, bad


def picture_bands(pixels):
    """uint8 [rows][cols][nb] -> its nb bands."""
    return [np.ascontiguousarray(pixels[:, :, b]) for b in range(pixels.shape[2])]
