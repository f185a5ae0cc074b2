"""A NumPy twin of jpegx_band_moments_packed_stacked_n and of the identity the distortion probe rests on, with nothing of the
product imported.

A band of rows x cols pixels pooled bs x bs and padded to whole N x N blocks is a plane of H x W samples.  After
DCTPadding.invert, SubSampling.invert and Padding.invert a decoded sample s at (y, x) stands for the pixels of its bs x bs tile
that lie inside the band -- its LIVE pixels, none for a sample of either padding -- and over them

    sum (p - s)^2 = S2 - 2 s S1 + cnt s^2,    S1 = sum p,  S2 = sum p^2,  cnt = their number,

so that the squared error of the whole band is the sum of that expression over the plane.  Everything here is int64 (uint64
for the packed words): S1 < 2^24, S2 < 2^32 and cnt <= 65025 for bs <= 255."""
import numpy as np


def blocked_shape(rows, cols, bs, n):
    """(H, W) of the plane of whole blocks: ceil(ceil(v / bs) / n) * n."""
    return tuple(-(-(-(-v // bs)) // n) * n for v in (rows, cols))


def moments(band, bs, n):
    """(S1, S2, cnt), each int64 [H][W], of a 2-D band of integers."""
    band = np.asarray(band).astype(np.int64)
    rows, cols = band.shape
    h, w = blocked_shape(rows, cols, bs, n)
    big = np.zeros((h * bs, w * bs), np.int64)
    live = np.zeros((h * bs, w * bs), np.int64)
    big[:rows, :cols] = band
    live[:rows, :cols] = 1

    def tiles(a):
        return a.reshape(h, bs, w, bs).sum(axis=(1, 3))
    return tiles(big), tiles(big * big), tiles(live)


def pack(s1, s2):
    """The words of the device gather: S2 << 32 | S1."""
    return (np.asarray(s2).astype(np.uint64) << np.uint64(32)) | np.asarray(s1).astype(np.uint64)


def grow(plane, rows, cols, bs):
    """Steps 2-0 inverted: crop the DCT padding, every sample bs x bs times, crop to the band."""
    return np.repeat(np.repeat(np.asarray(plane), bs, axis=0), bs, axis=1)[:rows, :cols]


def sse_direct(band, plane, bs):
    band = np.asarray(band).astype(np.int64)
    return int(((band - grow(plane, band.shape[0], band.shape[1], bs).astype(np.int64)) ** 2).sum())


def sse_moments(s1, s2, cnt, plane):
    s = np.asarray(plane).astype(np.int64)
    return int((s2 - 2 * s * s1 + cnt * s * s).sum())


def ycbcr(rgb):
    """Pillow's YCbCr of uint8 RGB pixels [...][3]."""
    from PIL import Image
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    flat = rgb.reshape(-1, 1, 3)
    return np.asarray(Image.fromarray(flat, mode="RGB").convert("YCbCr")).reshape(rgb.shape)
