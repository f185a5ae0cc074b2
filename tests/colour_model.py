"""Pillow's RGB <-> YCbCr conversion as integer table look-ups, in NumPy, from tests/golden/colour_tables.npz -- the
model the device kernels of csrc/jpegx_colour.hip are written after (scale 2^6, `>>` an arithmetic shift):

    Y  =  (y_r[r]  + y_g[g]  + y_b[b])  >> 6
    Cb = ((cb_r[r] + cb_g[g] + 32 * b)  >> 6) + 128
    Cr = ((32 * r  + cr_g[g] + cr_b[b]) >> 6) + 128

    R = clamp(Y + d_r[Cr])      G = clamp(Y + ((g_cb[Cb] + g_cr[Cr]) >> 6))      B = clamp(Y + d_b[Cb])

The tables are recovered from the installed Pillow by tests/golden/make_colour_tables.py; tests/test_colour_tables.py
holds the model against Pillow on every colour.  Uses NumPy only.
"""
import os

import numpy as np

TABLES_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colour_tables.npz")
FORWARD_TABLES = ("y_r", "y_g", "y_b", "cb_r", "cb_g", "cr_g", "cr_b")      # the order of the kernels' LDS image
INVERSE_TABLES = ("d_r", "g_cb", "g_cr", "d_b")

_tables = None


def load_tables():
    """name -> int32 array of 256 entries (int16 in the file)."""
    global _tables
    if _tables is None:
        with np.load(TABLES_PATH) as t:
            _tables = {k: t[k].astype(np.int32) for k in FORWARD_TABLES + INVERSE_TABLES}
    return _tables


def _bands(pixels):
    a = np.asarray(pixels)
    if a.dtype != np.uint8 or a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError("expected uint8 pixels (..., 3), got %r of %s" % (a.shape, a.dtype))
    return a[..., 0], a[..., 1], a[..., 2]


def rgb_to_ycbcr(pixels, tables=None):
    """uint8 (..., 3) RGB -> uint8 (..., 3) YCbCr, as Image.convert('YCbCr') gives it."""
    t = tables or load_tables()
    r, g, b = _bands(pixels)
    out = np.empty(r.shape + (3,), np.uint8)
    out[..., 0] = (t["y_r"][r] + t["y_g"][g] + t["y_b"][b]) >> 6
    out[..., 1] = ((t["cb_r"][r] + t["cb_g"][g] + 32 * b.astype(np.int32)) >> 6) + 128
    out[..., 2] = ((32 * r.astype(np.int32) + t["cr_g"][g] + t["cr_b"][b]) >> 6) + 128
    return out


def ycbcr_to_rgb(pixels, tables=None):
    """uint8 (..., 3) YCbCr -> uint8 (..., 3) RGB, as Image.convert('RGB') gives it."""
    t = tables or load_tables()
    y, cb, cr = _bands(pixels)
    y = y.astype(np.int32)
    out = np.empty(y.shape + (3,), np.uint8)
    out[..., 0] = np.clip(y + t["d_r"][cr], 0, 255)
    out[..., 1] = np.clip(y + ((t["g_cb"][cb] + t["g_cr"][cr]) >> 6), 0, 255)
    out[..., 2] = np.clip(y + t["d_b"][cb], 0, 255)
    return out


def all_colours():
    """The 4096 x 4096 x 3 uint8 picture that holds every triple once: pixel number i (row-major) is
    (i >> 16, (i >> 8) & 255, i & 255)."""
    i = np.arange(1 << 24, dtype=np.uint32)
    out = np.empty((1 << 24, 3), np.uint8)
    out[:, 0] = i >> 16
    out[:, 1] = (i >> 8) & 255
    out[:, 2] = i & 255
    return out.reshape(4096, 4096, 3)
