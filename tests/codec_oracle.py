"""End-to-end codec oracle: what the reference's compress_band / decompress_band compute for one band with
transform 'DCT' and dct_size 8, composed from the checker's functions (oracle/jpegx_oracle.c) and NumPy.

This is a plain helper module of the suite, not a conftest.  It imports only ``numpy`` and ``oracle``: never
``pipeline``, ``jpegx``, ``util``, ``file_format`` or anything else of the product, so a routing, padding, crop or
dtype mistake the product's roads share cannot hide in it (tests/test_abi.py checks this).  It is pinned to the
reference by every ``tests/golden/case_*.npz`` (tests/test_codec_oracle.py).

Forward (steps 0-8):
  0 Padding        edge replication to a multiple of block_size (only when block_size > 1)
  1 SubSampling    mean over block_size x block_size tiles (oracle.mean_pool)
  2 DCTPadding     edge replication of the POOLED samples to a multiple of 8
  3 Normalization  the identity on the way in
  4-6              float64 DCT, quantiser, zigzag (oracle.dct_plane / quant_plane / zigzag_plane)
  7-8              run-length codes and their byte stream (oracle.rle_bytestream); an amplitude beyond 15 bits
                   (|value| > 16383) is the reference's BadRleCodeError
Inverse: oracle.rle_decode, un-zigzag, restore, IDCT (rounded), clamp to 0..255, replication, crop.
"""
import math

import numpy as np

import oracle

# fixtures written by tests/golden/make_golden.py for the shapes conftest.CASES does not cover
# (conftest.py stays as it is, so the new names live here)
ROAD_CASES = ["ragged44x70b3", "ragged37x53b2", "ragged23x41b5", "ragged9x130b4", "ragged1x17b2", "ragged29x1b3",
              "ragged50x50b16", "ragged7x300b7", "extremes32x96b4", "halfties47x41b2"]

MAX_AMPLITUDE = 16383        # util.py RunLengthCode: a size above 15 bits (sign bit included) is refused


class BadRleCodeError(Exception):
    """The reference's util.BadRleCodeError condition: a zigzag value needs more than 15 bits."""


def padded_size(n, factor):
    return int(math.ceil(float(n) / factor) * factor)


def edge_pad(a, factor):
    """util.pad_array: replicate the last column, then the last row, up to a multiple of factor."""
    return np.pad(a, ((0, padded_size(a.shape[0], factor) - a.shape[0]), (0, padded_size(a.shape[1], factor) - a.shape[1])),
                  mode="edge")


def blocks_of(h, w, bs):
    """(block rows, block columns) of the zigzag stream for an h x w band."""
    ph, pw = padded_size(h, bs) // bs, padded_size(w, bs) // bs
    return padded_size(ph, 8) // 8, padded_size(pw, 8) // 8


def pre_transform(band, bs):
    """Steps 0-3 forward: the float64 plane that enters the DCT."""
    a = np.asarray(band).astype(np.float64)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("a non-empty 2-D band is expected")
    if bs > 1:
        a = oracle.mean_pool(edge_pad(a, bs), bs)
    return edge_pad(a, 8)


def forward_zigzag(band, bs, mode, param=0.0):
    """Steps 0-6 forward: float64 (H/8, W/8, 64) in the reference's order, before any narrowing."""
    return oracle.zigzag_plane(oracle.quant_plane(oracle.dct_plane(pre_transform(band, bs)), mode, param))


def compress_reference(band, bs, mode, param=0.0):
    """compress_band of the reference: the byte stream, or BadRleCodeError where the reference raises it."""
    zz = forward_zigzag(band, bs, mode, param)
    if np.abs(zz).max() > MAX_AMPLITUDE:
        raise BadRleCodeError("a zigzag value needs more than 15 bits (max |value| %d)" % int(np.abs(zz).max()))
    return oracle.rle_bytestream(zz.astype(np.int16))


def inverse_samples(zz, h, w, bs, mode, param=0.0):
    """Steps 6-0 inverted on an integer (hb, wb, 64) stream: the int64 (h, w) band."""
    rec = oracle.idct_plane(oracle.restore_plane(oracle.unzigzag_plane(zz), mode, param))
    out = np.repeat(np.repeat(np.clip(rec, 0, 255), bs, 0), bs, 1)[:h, :w]
    return np.ascontiguousarray(out, dtype=np.int64)


def decompress_reference(blob, h, w, bs, mode, param=0.0):
    """decompress_band of the reference on a byte stream: the int64 (h, w) band; oracle.RleStreamError (a ValueError)
    for a stream that does not decode into the band's blocks."""
    hb, wb = blocks_of(h, w, bs)
    zz = oracle.rle_decode(blob, hb * wb).reshape(hb, wb, 64)
    return inverse_samples(zz, h, w, bs, mode, param)
