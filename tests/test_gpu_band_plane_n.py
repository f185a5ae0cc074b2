"""The geometry prologue of the dct_size-N band job alone (csrc/jpegx_band_n.hip: Padding, SubSampling, DCTPadding and
Normalization.execute as one kernel) against the host step classes, float64 bit for bit: shapes that need no padding,
one padding, both, bands lower than one tile, one sample filling the plane, several workgroups, more than 65 535 output
rows; and through the device-pointer entry pitches off the width on both sides, with guard values that must survive."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (rows, cols, block_size, dct_size)
SHAPES = [(12, 20, 1, 4),               # nothing padded
          (13, 21, 1, 4),               # DCT padding only
          (31, 43, 3, 5),               # both paddings: 33 x 45 -> 11 x 15 -> 15 x 15
          (2, 7, 3, 2),                 # band lower than one tile
          (1, 1, 1, 2), (1, 1, 255, 32),        # one sample fills the plane
          (50, 341, 7, 24),             # several workgroups, k / 49 means
          (70000, 2, 1, 2), (2, 70000, 1, 2)]   # beyond 65 535 output rows / a long row


def host_plane(band, bs, n):
    """What leaves step 3 on the host: the reference's four step classes one after another."""
    import pipeline
    from pipeline import dct_padding, normalization, padding, subsampling
    cfg = pipeline.Configuration(width=band.shape[1], height=band.shape[0], block_size=bs, dct_size=n)
    a = band
    for cls in (padding.Padding, subsampling.SubSampling, dct_padding.DCTPadding, normalization.Normalization):
        a = cls(cfg).execute(a)
    return np.ascontiguousarray(a, dtype=np.float64)


def bands_of(rows, cols):
    noise = np.random.default_rng(rows * 100003 + cols).integers(0, 256, (rows, cols)).astype(np.uint8)
    edge = np.zeros((rows, cols), np.uint8)             # an off-by-one in either clamp changes what this one gives
    edge[-1, :] = 255
    edge[:, -1] = 255
    return (("noise", noise), ("edge", edge))


@pytest.mark.parametrize("rows,cols,bs,n", SHAPES)
def test_plane_is_the_host_steps_bit_for_bit(gpu, rows, cols, bs, n):
    for name, band in bands_of(rows, cols):
        want = host_plane(band, bs, n)
        assert want.shape == gpu.band_shape_n(rows, cols, bs, n)
        got = gpu.band_plane_n(band, bs, n)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert got.tobytes() == want.tobytes(), "%s band: %d samples differ" % (name, np.count_nonzero(got != want))


def test_wide_integer_bands_give_the_same_plane(gpu):
    band = bands_of(31, 43)[0][1]
    want = host_plane(band, 3, 5)
    for dtype in (np.int32, np.int64, np.uint16):
        assert gpu.band_plane_n(band.astype(dtype), 3, 5).tobytes() == want.tobytes()


def _device_plane(gpu, band, bs, n, in_gap, in_fill, out_gap, base_offset=0):
    """jpegx_band_plane_n on device pointers: the band stored with `in_gap` bytes of `in_fill` behind every row (and
    `base_offset` bytes in front), the output `out_gap` doubles wider than W and pre-filled with a guard value.
    Returns the whole output buffer [H][W + out_gap]."""
    rows, cols = band.shape
    h, w = gpu.band_shape_n(rows, cols, bs, n)
    pitch, opitch = cols + in_gap, w + out_gap
    stored = np.full(base_offset + rows * pitch, in_fill, np.uint8)
    stored[base_offset:].reshape(rows, pitch)[:, :cols] = band
    guard = np.full((h, opitch), -12345.5)
    din, dout = gpu.DeviceBuffer(stored.nbytes), gpu.DeviceBuffer(guard.nbytes)
    try:
        din.upload(stored)
        dout.upload(guard)
        gpu.check(gpu.lib().jpegx_band_plane_n(din.ptr + base_offset, rows, cols, pitch, bs, n, dout.ptr, opitch, None), "jpegx_band_plane_n")
        return dout.download((h, opitch), np.float64)
    finally:
        din.free()
        dout.free()


@pytest.mark.parametrize("rows,cols,bs,n", [(13, 21, 1, 4), (31, 43, 3, 5), (50, 341, 7, 24), (9, 300, 1, 16)])
def test_pitches_off_the_width(gpu, rows, cols, bs, n):
    """The margin replicates column cols - 1, never the bytes between the rows; nothing is written behind W."""
    for name, band in bands_of(rows, cols):
        want = host_plane(band, bs, n)
        w = want.shape[1]
        for fill in (0, 255):                           # both extremes: one of them is the opposite of the band's last column
            for base_offset in (0, 1, 2):               # rows that start on and off a dword boundary
                got = _device_plane(gpu, band, bs, n, 13, fill, 3, base_offset)
                assert got[:, :w].tobytes() == want.tobytes(), (name, fill, base_offset)
                assert np.all(got[:, w:] == -12345.5), "guard values behind the row were written"


def test_the_explicit_device_twin(gpu):
    band = bands_of(31, 43)[0][1]
    want = host_plane(band, 3, 5)
    din, dout = gpu.DeviceBuffer(band.nbytes), gpu.DeviceBuffer(want.nbytes)
    try:
        din.upload(band)
        gpu.check(gpu.lib().jpegx_band_plane_n_on(0, din.ptr, 31, 43, 43, 3, 5, dout.ptr, want.shape[1], None), "jpegx_band_plane_n_on")
        assert dout.download(want.shape, np.float64).tobytes() == want.tobytes()
    finally:
        din.free()
        dout.free()


def test_a_full_band_at_the_largest_block_size_is_exactly_255(gpu):
    band = np.full((300, 520), 255, np.uint8)           # 2 x 3 pooled samples, the last tile of each axis partly replicated
    got = gpu.band_plane_n(band, 255, 2)
    assert got.shape == (2, 4) and np.all(got == 255.0)
    assert got.tobytes() == host_plane(band, 255, 2).tobytes()
