"""GPU: jpegx_picture_planes_stacked_u8, the fused gather in front of the dct_size-8 picture batch, against its NumPy twin
(tests/picture_gather_model.py) on fenced buffers.  Every comparison is exact; every byte the kernel has no business
writing -- the pitch slack, the guards in front of and behind the planes -- must still hold the canary, and the input is
never written.

Shapes: cols 1, 15, 16, 17, 33 (below, at and above a lane's 16 samples, with and without a whole lane inside the picture),
rows 1 and 9, block_size 1, 2, 3, 4, 7 (padded rows of 8, 16 and more bytes: the 8-byte last piece and the 16-byte one), the
source 0, 1 and 3 bytes past a 16-byte boundary with an odd pitch (so the dword body and the byte path both run), 1, 3 and 22
pictures of distinct levels (a clamp that reaches into the neighbouring picture, or the 0xEE in the pitch gap, shows), both
values of colour."""
import numpy as np
import pytest

from fenced import Fenced, pitched, rows_mask, rows_of
from picture_gather_model import distinct_pictures, planes_twin

pytestmark = pytest.mark.gpu

COLS = [1, 15, 16, 17, 33]
ROWS = [1, 9]
SKEWS = [0, 1, 3]
PICTURES = [1, 3, 22]


def run(gpu, px, bs, colour, skew, extra=16):
    """The kernel on fenced buffers: the planes [k][nb][H * bs][W * bs], after the canaries and the input have been checked."""
    k, rows, cols, nb = px.shape
    h, w = gpu.padded_shape(rows, cols, bs)
    hh, ww = h * bs, w * bs
    pitch = (cols * nb + 4) | 1                           # odd, a gap of at least 4 bytes behind every row
    opitch = (ww + 15) // 16 * 16 + extra
    stacked = pitched(px.reshape(k * rows, cols * nb), pitch, 0xEE)
    din, dout = Fenced(gpu, stacked.size, offset=skew), Fenced(gpu, k * nb * hh * opitch)
    try:
        din.upload(stacked)
        gpu.picture_planes_stacked_u8_device(din.ptr, k, nb, rows, cols, bs, dout.ptr, opitch, colour, pitch=pitch)
        what = "gather %r bs %d colour %d skew %d" % (px.shape, bs, colour, skew)
        span = dout.download(rows_mask(dout.nbytes, k * nb * hh, opitch, ww), what)
        got = rows_of(span, k * nb * hh, opitch, ww).reshape(k, nb, hh, ww)
        assert np.array_equal(din.download(np.ones(din.nbytes, bool), what + ", input"), stacked), what + ": the input was written"
        return got
    finally:
        din.free()
        dout.free()


@pytest.mark.parametrize("colour", [0, 1])
@pytest.mark.parametrize("bs", [1, 2, 3, 4, 7])
def test_gather_equals_the_twin(gpu, bs, colour):
    for cols in COLS:
        for rows in ROWS:
            for k in PICTURES:
                for skew in SKEWS:
                    px = distinct_pictures([cols, rows, bs, k], k, rows, cols, 3)
                    got = run(gpu, px, bs, colour, skew)
                    want = planes_twin(px, bs, colour)
                    assert got.shape == want.shape
                    assert np.array_equal(got, want), "cols %d rows %d bs %d pictures %d skew %d colour %d: %d samples differ, first at %r" % (
                        cols, rows, bs, k, skew, colour, np.count_nonzero(got != want), tuple(np.argwhere(got != want)[0]))


@pytest.mark.parametrize("nb", [1, 2, 4])
def test_other_band_counts(gpu, nb):
    for cols, rows, bs, k, skew in [(33, 9, 1, 3, 1), (17, 9, 2, 22, 0), (16, 1, 4, 3, 3), (40, 9, 3, 3, 0), (15, 9, 7, 1, 1)]:
        px = distinct_pictures([nb, cols], k, rows, cols, nb)
        assert np.array_equal(run(gpu, px, bs, 0, skew), planes_twin(px, bs, 0)), (nb, cols, rows, bs, k, skew)


def test_full_range_colours_and_no_slack(gpu):
    """Noise over all 256 levels (the colour tables' whole range) on wider pictures, several lanes a row, and an output pitch
    of exactly the padded row rounded up to 16 bytes (at 23 x 41 and 44 x 70 the row is 8 mod 16: 8 bytes of slack)."""
    for rows, cols, bs in [(23, 41, 1), (37, 53, 2), (9, 130, 4), (44, 70, 3)]:
        px = np.random.default_rng([rows, cols]).integers(0, 256, (3, rows, cols, 3), dtype=np.uint8)
        for colour in (0, 1):
            assert np.array_equal(run(gpu, px, bs, colour, 3, extra=0), planes_twin(px, bs, colour)), (rows, cols, bs, colour)


@pytest.mark.parametrize("colour", [1, 0])
def test_the_colour_grid_on_its_second_trip(gpu, colour):
    """With colour the grid is capped at 1024 workgroups of 256 lanes and strides; 43 pictures of 100 x 1000 are
    43 * 104 * 63 = 281 736 lanes, 19 592 of them on their second trip through the tables filled once.  colour 0, whose grid
    covers the lanes, is the one-trip control."""
    px = np.random.default_rng(43).integers(0, 256, (43, 100, 1000, 3), dtype=np.uint8)
    assert 43 * gpu.padded_shape(100, 1000, 1)[0] * ((gpu.padded_shape(100, 1000, 1)[1] + 15) // 16) > 1024 * 256
    assert np.array_equal(run(gpu, px, 1, colour, 1), planes_twin(px, 1, colour))


def test_the_twin_is_the_three_kernel_composition(gpu):
    """Plane (p, k) is byte for byte what jpegx_rgb_to_ycbcr_u8 -> jpegx_deinterleave_u8 -> jpegx_pad_edges make today: the
    host conveniences of those three on one picture, against the fused gather and its convenience."""
    rows, cols, bs = 23, 41, 2
    px = np.random.default_rng(7).integers(0, 256, (2, rows, cols, 3), dtype=np.uint8)
    h, w = gpu.padded_shape(rows, cols, bs)
    fused = gpu.picture_planes_stacked_u8(px, bs, colour="rgb")
    assert fused.shape == (2, 3, h * bs, w * bs)
    for p in range(2):
        ycc = gpu.rgb_to_ycbcr(px[p])
        stack = np.zeros((3 * h * bs, w * bs), np.uint8)
        for b in range(3):
            stack[b * h * bs:b * h * bs + rows, :cols] = ycc[:, :, b]
        padded = gpu.pad_edges(stack, rows, cols, bs)
        assert np.array_equal(fused[p].reshape(3 * h * bs, w * bs), padded)
    assert np.array_equal(gpu.picture_planes_stacked_u8(px, bs), planes_twin(px, bs, 0))
