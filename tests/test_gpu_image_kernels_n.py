"""The two kernels of the dct_size-N picture job alone (csrc/jpegx_band_n.hip).

jpegx_band_planes_packed_n -- Padding, SubSampling, DCTPadding and Normalization.execute for every band of a pixel-interleaved
picture in one launch -- against the host step classes on pixels[:, :, k], float64 bit for bit, for 1..4 bands over the
shapes of tests/test_gpu_band_plane_n.py: bands of different noise (a band mix-up shows), an "edge" picture whose last row
and last column are 255 in band 0 only (an off-by-one in a clamp or in the band stride shows), and through the
device-pointer entry a packed pitch off the row, a base pointer off a dword and planes wider than W between NaN guards.

jpegx_inflate_crop_pack_u8 -- DCTPadding.invert, SubSampling.invert, Padding.invert and the np.dstack of Jpeg.decompress as
one scatter -- against np.repeat, a crop and np.dstack for 1..4 bands and block sizes 1, 3, 7, 255: output bases 0..3 bytes
off 16, an output pitch off the row between 0xA5 guards, plane pitches off the width, and a sentinel in every plane sample
the kernel must not read."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_band_plane_n import SHAPES, host_plane

pytestmark = pytest.mark.gpu

MAX_BANDS = 4


@functools.lru_cache(maxsize=None)
def pictures_of(rows, cols):
    """(name, pixels (rows, cols, 4)) -- every test takes the first nb bands; built once, read-only."""
    noise = np.random.default_rng(rows * 100003 + cols).integers(0, 256, (rows, cols, MAX_BANDS)).astype(np.uint8)
    edge = np.zeros((rows, cols, MAX_BANDS), np.uint8)
    edge[-1, :, 0] = 255
    edge[:, -1, 0] = 255
    for a in (noise, edge):
        a.setflags(write=False)
    return (("noise", noise), ("edge", edge))


@functools.lru_cache(maxsize=None)
def host_planes(rows, cols, bs, n, which):
    """The four step classes on every band of picture `which` of pictures_of(rows, cols): a tuple of float64 planes."""
    pixels = pictures_of(rows, cols)[which][1]
    planes = tuple(host_plane(np.ascontiguousarray(pixels[:, :, k]), bs, n) for k in range(MAX_BANDS))
    for p in planes:
        p.setflags(write=False)
    return planes


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
@pytest.mark.parametrize("rows,cols,bs,n", SHAPES)
def test_every_plane_is_the_host_steps_bit_for_bit(gpu, rows, cols, bs, n, nb):
    for which, (name, pixels) in enumerate(pictures_of(rows, cols)):
        want = host_planes(rows, cols, bs, n, which)
        got = gpu.band_planes_packed_n(np.ascontiguousarray(pixels[:, :, :nb]), bs, n)
        assert len(got) == nb
        for k in range(nb):
            assert got[k].dtype == np.float64 and got[k].shape == want[k].shape == gpu.band_shape_n(rows, cols, bs, n)
            assert got[k].tobytes() == want[k].tobytes(), "%s picture, band %d of %d: %d samples differ" % (
                name, k, nb, np.count_nonzero(got[k] != want[k]))


def test_one_band_is_the_band_kernel(gpu):
    """nbands 1 is jpegx_band_plane_n's job: the same plane from both entries."""
    pixels = pictures_of(31, 43)[0][1]
    for bs, n in ((1, 4), (3, 5)):
        assert gpu.band_planes_packed_n(np.ascontiguousarray(pixels[:, :, :1]), bs, n)[0].tobytes() == \
            gpu.band_plane_n(np.ascontiguousarray(pixels[:, :, 0]), bs, n).tobytes()


def _device_planes(gpu, pixels, bs, n, in_gap, in_fill, out_gap, base_offset, on=False):
    """jpegx_band_planes_packed_n on device pointers: the picture stored with `in_gap` bytes of `in_fill` behind every row
    and `base_offset` bytes in front; every plane `out_gap` doubles wider than W with 8 doubles behind its last row, all NaN
    beforehand.  Returns the whole plane buffers, flat."""
    rows, cols, nb = pixels.shape
    h, w = gpu.band_shape_n(rows, cols, bs, n)
    pitch, opitch = cols * nb + in_gap, w + out_gap
    stored = np.full(base_offset + rows * pitch, in_fill, np.uint8)
    stored[base_offset:].reshape(rows, pitch)[:, :cols * nb] = pixels.reshape(rows, cols * nb)
    guard = np.full(h * opitch + 8, np.nan)
    din, douts = gpu.DeviceBuffer(stored.nbytes), [gpu.DeviceBuffer(guard.nbytes) for _ in range(nb)]
    try:
        din.upload(stored)
        for d in douts:
            d.upload(guard)
        ptrs = (ctypes.c_void_p * nb)(*[d.ptr for d in douts])
        args = (din.ptr + base_offset, nb, rows, cols, pitch, bs, n, ptrs, opitch, None)
        if on:
            gpu.check(gpu.lib().jpegx_band_planes_packed_n_on(0, *args), "jpegx_band_planes_packed_n_on")
        else:
            gpu.check(gpu.lib().jpegx_band_planes_packed_n(*args), "jpegx_band_planes_packed_n")
        return [d.download((h * opitch + 8,), np.float64) for d in douts], h, w, opitch
    finally:
        din.free()
        for d in douts:
            d.free()


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
@pytest.mark.parametrize("rows,cols,bs,n", [(13, 21, 1, 4), (31, 43, 3, 5), (50, 341, 7, 24), (9, 300, 1, 16)])
def test_pitches_and_bases_off_their_alignment(gpu, rows, cols, bs, n, nb):
    """The margin replicates pixel cols - 1, never the bytes between the rows; nothing is written beside or behind a plane."""
    for which, (name, pixels) in enumerate(pictures_of(rows, cols)):
        want = host_planes(rows, cols, bs, n, which)
        for fill, base_offset in ((0, 1), (255, 2), (255, 3), (0, 0)):     # both extremes: one is the opposite of the last column
            got, h, w, opitch = _device_planes(gpu, np.ascontiguousarray(pixels[:, :, :nb]), bs, n, 5, fill, 3, base_offset)
            for k in range(nb):
                body = got[k][:h * opitch].reshape(h, opitch)
                assert body[:, :w].tobytes() == want[k].tobytes(), (name, k, fill, base_offset)
                assert np.all(np.isnan(body[:, w:])), "guard values beside plane %d were written" % k
                assert np.all(np.isnan(got[k][h * opitch:])), "guard values behind plane %d were written" % k


def test_the_gather_twin_gives_the_same_planes(gpu):
    pixels = np.ascontiguousarray(pictures_of(31, 43)[0][1][:, :, :3])
    want = host_planes(31, 43, 3, 5, 0)
    got, h, w, opitch = _device_planes(gpu, pixels, 3, 5, 0, 0, 0, 0, on=True)
    for k in range(3):
        assert got[k][:h * opitch].reshape(h, opitch).tobytes() == want[k].tobytes()


def test_full_pixels_at_the_largest_block_size_are_exactly_255(gpu):
    pixels = np.full((300, 520, 3), 255, np.uint8)      # 2 x 3 pooled samples, the last tile of each axis partly replicated
    pixels[:, :, 1] = 0
    got = gpu.band_planes_packed_n(pixels, 255, 2)
    assert all(p.shape == (2, 4) for p in got)
    assert np.all(got[0] == 255.0) and np.all(got[1] == 0.0) and np.all(got[2] == 255.0)


# ---- the way back -------------------------------------------------------------------------------------------------------
SENTINEL = 255
# (rows, cols): every column count at which the lane's span ends differently (1, 5: inside the first; 16, 17: at and one
# past a 16-byte unit; 341: several workgroups' worth at four bands), beyond 65 535 rows, and a long row
BACK_SHAPES = [(9, 1), (9, 5), (9, 16), (9, 17), (9, 341), (70000, 2), (2, 70000)]


@functools.lru_cache(maxsize=None)
def back_case(rows, cols, bs):
    """Four planes one row and two columns larger than the pooled band, the sentinel in everything beyond it, values below it
    inside; and what np.repeat, the crop and np.dstack make of them."""
    pr, pc = -(-rows // bs), -(-cols // bs)
    rng = np.random.default_rng(rows * 7919 + cols * 31 + bs)
    planes = np.full((MAX_BANDS, pr + 1, pc + 2), SENTINEL, np.uint8)
    planes[:, :pr, :pc] = rng.integers(0, SENTINEL, (MAX_BANDS, pr, pc))
    grown = [np.repeat(np.repeat(planes[k, :pr, :pc], bs, axis=0)[:rows], bs, axis=1)[:, :cols] for k in range(MAX_BANDS)]
    want = np.dstack(grown)
    planes.setflags(write=False)
    want.setflags(write=False)
    return planes, want


def _device_pack(gpu, planes, nb, rows, cols, bs, plane_gap, out_gap, base_offset, on=False):
    """jpegx_inflate_crop_pack_u8 on device pointers: planes stored `plane_gap` bytes (of the sentinel) wider than they are,
    the output `base_offset` bytes off a 16-byte boundary with `out_gap` bytes behind every row, 0xA5 everywhere beforehand.
    Returns the whole output buffer."""
    ph, pw = planes.shape[1:]
    pitch, opitch = pw + plane_gap, cols * nb + out_gap
    guard = np.full(base_offset + rows * opitch + 16, 0xA5, np.uint8)
    dins, dout = [gpu.DeviceBuffer(ph * pitch) for _ in range(nb)], gpu.DeviceBuffer(guard.nbytes)
    try:
        for k, d in enumerate(dins):
            stored = np.full((ph, pitch), SENTINEL, np.uint8)
            stored[:, :pw] = planes[k]
            d.upload(stored)
        dout.upload(guard)
        assert dout.ptr % 16 == 0
        ptrs = (ctypes.c_void_p * nb)(*[d.ptr for d in dins])
        args = (ptrs, nb, pitch, rows, cols, bs, dout.ptr + base_offset, opitch, None)
        if on:
            gpu.check(gpu.lib().jpegx_inflate_crop_pack_u8_on(0, *args), "jpegx_inflate_crop_pack_u8_on")
        else:
            gpu.check(gpu.lib().jpegx_inflate_crop_pack_u8(*args), "jpegx_inflate_crop_pack_u8")
        return dout.download(guard.shape, np.uint8), opitch
    finally:
        dout.free()
        for d in dins:
            d.free()


def check_pack(gpu, nb, rows, cols, bs, plane_gap, out_gap, base_offset, on=False):
    planes, want = back_case(rows, cols, bs)
    got, opitch = _device_pack(gpu, planes, nb, rows, cols, bs, plane_gap, out_gap, base_offset, on)
    what = (nb, rows, cols, bs, base_offset)
    assert np.all(got[:base_offset] == 0xA5), what
    body = got[base_offset:base_offset + rows * opitch].reshape(rows, opitch)
    assert not np.any(body[:, :cols * nb] == SENTINEL), "a sample the kernel must not read reached the output: %r" % (what,)
    assert np.array_equal(body[:, :cols * nb].reshape(rows, cols, nb), want[:, :, :nb]), what
    assert np.all(body[:, cols * nb:] == 0xA5), "guard bytes behind a row were written: %r" % (what,)
    assert np.all(got[base_offset + rows * opitch:] == 0xA5), "guard bytes behind the picture were written: %r" % (what,)


@pytest.mark.parametrize("bs", [1, 3, 7, 255])
@pytest.mark.parametrize("nb", [1, 2, 3, 4])
def test_the_scatter_is_repeat_crop_and_dstack(gpu, nb, bs):
    for rows, cols in BACK_SHAPES:
        for base_offset in range(4):
            check_pack(gpu, nb, rows, cols, bs, 3, 7, base_offset)


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
def test_rows_back_to_back_take_the_wide_stores(gpu, nb):
    """No gap anywhere and an aligned base: with 48 columns every row of every band count starts on a 16-byte boundary."""
    for bs in (1, 3):
        check_pack(gpu, nb, 9, 48, bs, 0, 0, 0)
        planes, want = back_case(9, 48, bs)
        got = gpu.inflate_crop_pack_u8([planes[k] for k in range(nb)], 9, 48, bs)
        assert got.shape == (9, 48, nb) and got.dtype == np.uint8 and np.array_equal(got, want[:, :, :nb])
        got = gpu.inflate_crop_pack_u8([planes[k] for k in range(nb)], 9, 48, bs, pitch=planes.shape[2] + 5, out_pitch=48 * nb + 9)
        assert np.array_equal(got, want[:, :, :nb])


def test_one_band_is_the_band_scatter(gpu):
    planes, want = back_case(9, 341, 3)
    assert np.array_equal(gpu.inflate_crop_pack_u8([planes[0]], 9, 341, 3)[:, :, 0], gpu.inflate_crop_u8(planes[0], 3, 9, 341))


def test_the_scatter_twin_gives_the_same_picture(gpu):
    check_pack(gpu, 3, 9, 341, 3, 3, 7, 1, on=True)
