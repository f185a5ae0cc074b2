"""GPU: the gather and the scatter of the picture batch for dct_size != 8 alone, against NumPy.

jpegx_band_planes_packed_stacked_n: plane p * nbands + k must be what tests/codec_oracle_n.py's pre_transform makes of band k
of picture p (exact: integer tile sums, one division) -- with colour 1 of the picture's YCbCr as tests/colour_model.py gives
it -- whatever stands in the neighbouring pictures of the stack and in the gap behind every input row.
jpegx_inflate_crop_pack_stacked_u8: out[p][y][x * nbands + k] = plane (p, k)[y // bs][x // bs] -- with colour 1 the RGB of
that triple -- exactly cols * nbands bytes per row.  Every output lies between canaries and has canaries in its pitch slack.
One test puts the rows a far pitch apart, so that the whole last picture lies past 2^32 bytes (tests/far.py)."""
import numpy as np
import pytest

import codec_oracle_n as on
import colour_model
import far
from batch_n_dev import CANARY, Fenced, pitched

pytestmark = pytest.mark.gpu

N = 5
SHAPES = [(1, 1), (1, 37), (37, 1), (29, 43)]
# (nbands, colour): both colours at three bands on every shape; 1, 2 and 4 bands as they are on the largest shape
GRID = [(shape, nb, colour) for shape in SHAPES for nb, colour in ((3, 0), (3, 1))] + [((29, 43), nb, 0) for nb in (1, 2, 4)]
GRID_IDS = ["%dx%d-nb%d-colour%d" % (s + (nb, c)) for s, nb, c in GRID]


def far_last_plane(nrows, per_picture, row_bytes, align):
    """`nrows` rows whose last picture (or plane) of `per_picture` rows starts past 2^32 bytes: the smallest such pitch that is
    a multiple of `align`."""
    pitch = -(-far.WRAP // (nrows - per_picture))
    pitch = (pitch + align - 1) // align * align + align
    lay = far.Rows(nrows, row_bytes, pitch)
    assert lay.far_rows().size >= per_picture and lay.far_rows()[0] <= nrows - per_picture
    return lay


def pictures_of(seed, npictures, rows, cols, nbands):
    return np.random.default_rng(seed).integers(0, 256, (npictures, rows, cols, nbands), dtype=np.uint8)


def planes_of(pixels, colour, bs, n):
    """The float64 planes, picture-major, of the model pixels: the input, or colour_model's YCbCr of it."""
    model = colour_model.rgb_to_ycbcr(pixels) if colour else pixels
    return np.concatenate([on.pre_transform(model[p][:, :, k], bs, n) for p in range(model.shape[0]) for k in range(model.shape[3])])


def pixels_of(planes, npictures, nbands, rows, cols, bs, colour):
    """[npictures][rows][cols][nbands] from uint8 planes [npictures * nbands][H][W]: np.repeat + crop + np.dstack per picture,
    then colour_model's RGB."""
    out = np.stack([np.dstack([np.repeat(np.repeat(planes[p * nbands + k], bs, 0), bs, 1)[:rows, :cols] for k in range(nbands)])
                    for p in range(npictures)])
    return colour_model.ycbcr_to_rgb(out) if colour else out


@pytest.mark.parametrize("case", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("npictures", [1, 2, 5])
@pytest.mark.parametrize("bs", [1, 2, 3, 7])
def test_packed_stacked_gather(gpu, bs, npictures, case):
    (rows, cols), nb, colour = case
    pixels = pictures_of([bs, npictures, rows, cols, nb, colour], npictures, rows, cols, nb)
    H, W = gpu.band_shape_n(rows, cols, bs, N)
    pitch, opitch = cols * nb + 3, W + 3                  # doubles: a slack of 24 bytes behind every output row
    din = Fenced(gpu, npictures * rows * pitch, skew=1)   # the pixels need no alignment
    dout = Fenced(gpu, npictures * nb * H * opitch * 8)
    try:
        din.upload(pitched(pixels.reshape(npictures * rows, cols * nb), pitch, 0xEE))      # a poisoned gap
        gpu.band_planes_packed_stacked_n_device(din.ptr, npictures, nb, rows, cols, bs, N, dout.ptr, colour=colour, pitch=pitch,
                                                out_pitch=opitch)
        got = dout.payload(dout.nbytes, "packed stacked gather").view(np.float64).reshape(npictures * nb * H, opitch)
        want = planes_of(pixels, colour, bs, N)
        assert np.array_equal(got[:, :W], want)
        assert np.all(got[:, W:].view(np.uint8) == CANARY), "the pitch slack was written"
        # a group of the batch on its own: the caller offsets the pointer
        if npictures > 3:
            dout.fill()
            gpu.band_planes_packed_stacked_n_device(din.ptr + 2 * rows * pitch, 2, nb, rows, cols, bs, N, dout.ptr, colour=colour,
                                                    pitch=pitch, out_pitch=opitch)
            part = dout.payload(2 * nb * H * opitch * 8, "gather of pictures 2..3").view(np.float64).reshape(2 * nb * H, opitch)
            assert np.array_equal(part[:, :W], want[2 * nb * H:4 * nb * H])
    finally:
        din.free()
        dout.free()


@pytest.mark.parametrize("case", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("npictures", [1, 2, 5])
@pytest.mark.parametrize("bs", [1, 2, 3, 7])
def test_packed_stacked_scatter(gpu, bs, npictures, case):
    (rows, cols), nb, colour = case
    H, W = gpu.band_shape_n(rows, cols, bs, N)
    planes = np.random.default_rng([7, bs, npictures, rows, cols, nb, colour]).integers(0, 256, (npictures * nb, H, W), dtype=np.uint8)
    pitch, opitch = W + 5, cols * nb + 19
    din = Fenced(gpu, npictures * nb * H * pitch, skew=3)
    dout = Fenced(gpu, npictures * rows * opitch, skew=1)
    try:
        din.upload(pitched(planes.reshape(npictures * nb * H, W), pitch, 0xEE))
        gpu.inflate_crop_pack_stacked_u8_device(din.ptr, npictures, nb, H, pitch, rows, cols, bs, dout.ptr, colour=colour,
                                                out_pitch=opitch)
        got = dout.payload(dout.nbytes, "packed stacked scatter").reshape(npictures * rows, opitch)
        want = pixels_of(planes, npictures, nb, rows, cols, bs, colour).reshape(npictures * rows, cols * nb)
        assert np.array_equal(got[:, :cols * nb], want)
        assert np.all(got[:, cols * nb:] == CANARY), "the pitch slack was written"
    finally:
        din.free()
        dout.free()


def test_packed_stacked_kernels_refuse_bad_arguments(gpu):
    L = gpu.lib()
    buf = gpu.DeviceBuffer(4096)
    try:
        p = buf.ptr
        G, S = L.jpegx_band_planes_packed_stacked_n, L.jpegx_inflate_crop_pack_stacked_u8
        assert G(None, 1, 3, 4, 4, 12, 0, 1, 4, p, 4, None) == -1
        assert G(p, 1, 3, 4, 4, 12, 0, 1, 4, None, 4, None) == -1
        assert G(p, 0, 3, 4, 4, 12, 0, 1, 4, p, 4, None) == -1
        assert G(p, 1, 0, 4, 4, 12, 0, 1, 4, p, 4, None) == -1
        assert G(p, 1, 5, 4, 4, 20, 0, 1, 4, p, 4, None) == -1
        assert G(p, 1, 2, 4, 4, 12, 1, 1, 4, p, 4, None) == -1          # colour 1 needs three bands
        assert G(p, 1, 3, 4, 4, 12, 2, 1, 4, p, 4, None) == -1
        assert G(p, 1, 3, 4, 4, 11, 0, 1, 4, p, 4, None) == -1          # pitch below cols * nbands
        assert G(p, 1, 3, 4, 4, 12, 0, 1, 4, p, 3, None) == -1          # output pitch below W
        assert G(p, 1, 3, 4, 4, 12, 0, 1, 4, p + 4, 4, None) == -1      # misaligned doubles
        assert G(p, 1, 3, 4, 4, 12, 0, 0, 4, p, 4, None) == -4
        assert G(p, 1, 3, 4, 4, 12, 0, 256, 4, p, 4, None) == -4
        assert G(p, 1, 3, 4, 4, 12, 0, 1, 33, p, 4, None) == -1
        assert G(p, 1 << 28, 3, 4, 4, 12, 0, 1, 4, p, 4, None) == -1    # 2^31 samples and more
        assert S(None, 1, 3, 4, 4, 4, 4, 1, 0, p, 12, None) == -1
        assert S(p, 0, 3, 4, 4, 4, 4, 1, 0, p, 12, None) == -1
        assert S(p, 1, 5, 4, 4, 4, 4, 1, 0, p, 20, None) == -1
        assert S(p, 1, 2, 4, 4, 4, 4, 1, 1, p, 12, None) == -1
        assert S(p, 1, 3, 4, 4, 4, 4, 1, 2, p, 12, None) == -1
        assert S(p, 1, 3, 1, 4, 4, 4, 2, 0, p, 12, None) == -1          # planes lower than the pooled band
        assert S(p, 1, 3, 4, 1, 4, 4, 2, 0, p, 12, None) == -1          # pitch below ceil(cols / bs)
        assert S(p, 1, 3, 4, 4, 4, 4, 1, 0, p, 11, None) == -1
        assert S(p, 1, 3, 4, 4, 4, 4, 256, 0, p, 12, None) == -4
        assert S(p, 1 << 30, 3, 4, 4, 4, 4, 1, 0, p, 12, None) == -1
    finally:
        buf.free()


def test_packed_stacked_kernels_with_a_far_pitch(gpu):
    """Three RGB pictures of 24 pooled rows each at bs 3, colour 1, the rows so far apart that the whole last picture lies
    past 2^32 bytes: the gather with far input, the scatter with far output, the other side with tight rows."""
    n, bs, npictures, nb = 8, 3, 3, 3
    rows, cols = 24 * bs - (bs - 1), 37 * bs
    H, W = gpu.band_shape_n(rows, cols, bs, n)
    assert (H, W) == (24, 40)
    pixels = pictures_of([99, bs], npictures, rows, cols, nb)
    lin = far_last_plane(npictures * rows, rows, cols * nb, 1)
    lout = far.Rows(npictures * nb * H, W * 8, W * 8 + 8)
    a, b = far.FarBuffer(gpu, lin.nbytes), far.FarBuffer(gpu, lout.nbytes)
    try:
        a.upload_rows(lin, pixels.reshape(npictures * rows, cols * nb))
        gpu.band_planes_packed_stacked_n_device(a.ptr, npictures, nb, rows, cols, bs, n, b.ptr, colour=1, pitch=lin.pitch,
                                                out_pitch=lout.pitch // 8)
        assert np.array_equal(b.download_rows(lout, np.float64), planes_of(pixels, 1, bs, n))
        b.check_output(lout.extents(), "packed stacked gather, far input")
    finally:
        a.free()
        b.free()
    planes = np.random.default_rng([98, bs]).integers(0, 256, (npictures * nb, H, W), dtype=np.uint8)
    lin = far.Rows(npictures * nb * H, W, W + 3)
    lout = far_last_plane(npictures * rows, rows, cols * nb, 1)
    a, b = far.FarBuffer(gpu, lin.nbytes), far.FarBuffer(gpu, lout.nbytes)
    try:
        a.upload_rows(lin, planes.reshape(npictures * nb * H, W))
        gpu.inflate_crop_pack_stacked_u8_device(a.ptr, npictures, nb, H, lin.pitch, rows, cols, bs, b.ptr, colour=1, out_pitch=lout.pitch)
        assert np.array_equal(b.download_rows(lout), pixels_of(planes, npictures, nb, rows, cols, bs, 1).reshape(npictures * rows, cols * nb))
        b.check_output(lout.extents(), "packed stacked scatter, far output")
    finally:
        a.free()
        b.free()
