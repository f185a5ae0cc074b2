"""jpegx.batch_probe_distortion_pictures_n against jpegx_probe_distortion_n per group: the batch entry with group_planes forcing 1, 2
and 3 groups equals the two gathers and the kernel entry run group by group by hand, and -- through the host convenience -- the
round trip of the batch codec (batch_compress_pictures_n, batch_decompress_pictures_n) compared with the pictures in NumPy.
Pictures of 67 x 93 with three bands, colour off and on."""
import numpy as np
import pytest

import distortion_model as dm

pytestmark = pytest.mark.gpu

ROWS, COLS, COUNT = 67, 93, 5
DIVISORS = [5.0, 40.0, 1000.0]                       # 255 * 16^2 / 5 codes in 15 bits
BAD = np.uint64(1 << 63)


def _pixels(seed=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ROWS, 0:COLS]
    out = np.empty((COUNT, ROWS, COLS, 3), np.uint8)
    for p in range(COUNT):
        smooth = ((yy * (2 + p) + xx * 3) % 256)[..., None] + np.arange(3) * 30
        out[p] = np.where((xx < COLS // 2)[..., None], smooth, rng.integers(0, 256, (ROWS, COLS, 3))) % 256
    return out


def _by_hand(gpu, pixels, bs, n, colour, pictures_per_group):
    """The gathers and the kernel entry, one group of pictures after another, each into fresh buffers."""
    h, w = gpu.band_shape_n(ROWS, COLS, bs, n)
    out = np.empty((COUNT, 3, len(DIVISORS)), np.uint64)
    for q0 in range(0, COUNT, pictures_per_group):
        part = np.ascontiguousarray(pixels[q0:q0 + pictures_per_group])
        k = part.shape[0]
        din, dpl, dmo, dtot = (gpu.DeviceBuffer(v) for v in (part.nbytes, k * 3 * h * w * 8, k * 3 * h * w * 8, k * 3 * len(DIVISORS) * 8))
        try:
            din.upload(part)
            gpu.band_planes_packed_stacked_n_device(din.ptr, k, 3, ROWS, COLS, bs, n, dpl.ptr, colour=colour)
            gpu.band_moments_packed_stacked_n_device(din.ptr, k, 3, ROWS, COLS, bs, n, dmo.ptr, colour=colour)
            gpu.probe_distortion_n_device(dpl.ptr, dmo.ptr, k * 3, h, w, n, bs, ROWS, COLS, "divide", DIVISORS, dtot.ptr)
            gpu.check(gpu.lib().jpegx_stream_synchronize(None))
            out[q0:q0 + k] = dtot.download((k, 3, len(DIVISORS)), np.uint64)
        finally:
            for b in (din, dpl, dmo, dtot):
                b.free()
    return out


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, n", [(1, 4), (1, 16), (2, 12)])
def test_groups_of_pictures_equal_the_kernel_entry_per_group(gpu, bs, n, colour):
    pixels = _pixels()
    first = None
    for pictures_per_group, groups in ((5, 1), (3, 2), (2, 3)):
        want = _by_hand(gpu, pixels, bs, n, 1 if colour else 0, pictures_per_group)
        sse, bad = gpu.batch_probe_distortion_pictures_n(pixels, bs, n, "divide", DIVISORS, colour=colour, group_planes=3 * pictures_per_group)
        assert -(-COUNT // pictures_per_group) == groups
        assert np.array_equal(sse, want & ~BAD) and np.array_equal(bad, (want & BAD) != 0), (bs, n, colour, groups)
        first = sse if first is None else first
        assert np.array_equal(sse, first)                                  # the cut changes nothing
    assert not bad.any() and (np.diff(first.astype(np.int64), axis=2) > 0).all()


@pytest.mark.parametrize("colour", [None, "rgb"])
def test_the_sums_are_those_of_the_batch_codec_round_trip(gpu, colour):
    pixels = _pixels(4)
    bs, n = 2, 12
    sse, bad = gpu.batch_probe_distortion_pictures_n(pixels, bs, n, "divide", DIVISORS, colour=colour)
    assert not bad.any()
    coded = dm.ycbcr(pixels) if colour else pixels
    for q, d in enumerate(DIVISORS):
        blobs = gpu.batch_compress_pictures_n(pixels, bs, n, "divide", d, **({"colour": colour} if colour else {}))
        back = gpu.batch_decompress_pictures_n(blobs, ROWS, COLS, bs, n, "divide", d)          # the coded bands, no conversion back
        want = ((np.asarray(back).astype(np.int64) - coded.astype(np.int64)) ** 2).sum(axis=(1, 2))
        assert np.array_equal(sse[:, :, q].astype(np.int64), want), (colour, d)
