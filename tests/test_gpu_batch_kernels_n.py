"""GPU: the two stacked kernels of the batch codec for dct_size != 8 alone, against NumPy.

jpegx_band_planes_stacked_n: plane p must be what tests/codec_oracle_n.py's pre_transform makes of band p (exact: integer
tile sums, one division), whatever stands in the neighbouring bands of the stack and in the gap behind every input row.
jpegx_inflate_crop_stacked_u8: out[p][y][x] = plane p[y // bs][x // bs], exactly cols bytes per row.  Every output lies
between canaries and has canaries in its pitch slack.  One test puts the rows of both a far pitch apart, so that the
later planes lie past 2^32 bytes (tests/far.py)."""
import numpy as np
import pytest

import codec_oracle_n as on
import far
from batch_n_dev import CANARY, Fenced, pitched

pytestmark = pytest.mark.gpu

N = 5
SHAPES = [(1, 1), (1, 37), (37, 1), (29, 43)]


def far_last_plane(nrows, per_plane, row_bytes, align):
    """`nrows` rows whose last plane of `per_plane` rows starts past 2^32 bytes: the smallest such pitch that is a multiple
    of `align` (about 6.4 GiB for three planes)."""
    pitch = -(-far.WRAP // (nrows - per_plane))
    pitch = (pitch + align - 1) // align * align + align
    lay = far.Rows(nrows, row_bytes, pitch)
    assert lay.far_rows().size >= per_plane and lay.far_rows()[0] <= nrows - per_plane
    return lay


def stack_of(seed, nplanes, rows, cols):
    return np.random.default_rng(seed).integers(0, 256, (nplanes, rows, cols), dtype=np.uint8)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("nplanes", [1, 2, 5])
@pytest.mark.parametrize("bs", [1, 2, 3, 7])
def test_stacked_gather(gpu, bs, nplanes, shape):
    rows, cols = shape
    bands = stack_of([bs, nplanes, rows, cols], nplanes, rows, cols)
    H, W = gpu.band_shape_n(rows, cols, bs, N)
    pitch, opitch = cols + 3, W + 3                       # doubles: a slack of 24 bytes behind every output row
    din = Fenced(gpu, nplanes * rows * pitch, skew=1)     # the bands need no alignment
    dout = Fenced(gpu, nplanes * H * opitch * 8)
    try:
        din.upload(pitched(bands.reshape(nplanes * rows, cols), pitch, 0xEE))      # a poisoned gap
        gpu.band_planes_stacked_n_device(din.ptr, nplanes, rows, cols, bs, N, dout.ptr, pitch=pitch, out_pitch=opitch)
        got = dout.payload(dout.nbytes, "stacked gather").view(np.float64).reshape(nplanes * H, opitch)
        want = np.concatenate([on.pre_transform(b, bs, N) for b in bands])
        assert np.array_equal(got[:, :W], want)
        assert np.all(got[:, W:].view(np.uint8) == CANARY), "the pitch slack was written"
        # a group of the batch on its own: the caller offsets the pointer
        if nplanes > 2:
            dout.fill()
            gpu.band_planes_stacked_n_device(din.ptr + 2 * rows * pitch, 2, rows, cols, bs, N, dout.ptr, pitch=pitch, out_pitch=opitch)
            part = dout.payload(2 * H * opitch * 8, "stacked gather of planes 2..3").view(np.float64).reshape(2 * H, opitch)
            assert np.array_equal(part[:, :W], want[2 * H:4 * H])
    finally:
        din.free()
        dout.free()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("nplanes", [1, 2, 5])
@pytest.mark.parametrize("bs", [1, 2, 3, 7])
def test_stacked_scatter(gpu, bs, nplanes, shape):
    rows, cols = shape
    H, W = gpu.band_shape_n(rows, cols, bs, N)
    planes = stack_of([7, bs, nplanes, rows, cols], nplanes, H, W)
    pitch, opitch = W + 5, cols + 19
    din = Fenced(gpu, nplanes * H * pitch, skew=3)
    dout = Fenced(gpu, nplanes * rows * opitch, skew=1)
    try:
        din.upload(pitched(planes.reshape(nplanes * H, W), pitch, 0xEE))
        gpu.inflate_crop_stacked_u8_device(din.ptr, nplanes, H, pitch, rows, cols, bs, dout.ptr, out_pitch=opitch)
        got = dout.payload(dout.nbytes, "stacked scatter").reshape(nplanes * rows, opitch)
        want = np.concatenate([np.repeat(np.repeat(p, bs, 0), bs, 1)[:rows, :cols] for p in planes])
        assert np.array_equal(got[:, :cols], want)
        assert np.all(got[:, cols:] == CANARY), "the pitch slack was written"
    finally:
        din.free()
        dout.free()


def test_stacked_kernels_refuse_bad_arguments(gpu):
    L = gpu.lib()
    buf = gpu.DeviceBuffer(4096)
    try:
        p = buf.ptr
        assert L.jpegx_band_planes_stacked_n(p, 0, 4, 4, 4, 1, 4, p, 4, None) == -1
        assert L.jpegx_band_planes_stacked_n(p, 1, 4, 4, 3, 1, 4, p, 4, None) == -1          # pitch below cols
        assert L.jpegx_band_planes_stacked_n(p, 1, 4, 4, 4, 1, 4, p + 4, 4, None) == -1      # misaligned doubles
        assert L.jpegx_band_planes_stacked_n(p, 1, 4, 4, 4, 0, 4, p, 4, None) == -4
        assert L.jpegx_band_planes_stacked_n(p, 1 << 30, 4, 4, 4, 1, 4, p, 4, None) == -1    # 2^31 samples and more
        assert L.jpegx_inflate_crop_stacked_u8(p, 0, 4, 4, 4, 4, 1, p, 4, None) == -1
        assert L.jpegx_inflate_crop_stacked_u8(p, 1, 1, 4, 4, 4, 2, p, 4, None) == -1        # planes lower than the pooled band
        assert L.jpegx_inflate_crop_stacked_u8(p, 1, 4, 1, 4, 4, 2, p, 4, None) == -1        # pitch below ceil(cols / bs)
        assert L.jpegx_inflate_crop_stacked_u8(p, 1, 4, 4, 4, 4, 1, p, 3, None) == -1
        assert L.jpegx_inflate_crop_stacked_u8(p, 1, 4, 4, 4, 4, 256, p, 4, None) == -4
    finally:
        buf.free()


@pytest.mark.parametrize("bs", [1, 3])
def test_stacked_kernels_with_a_far_pitch(gpu, bs):
    """Three bands of 24 pooled rows each, the rows of the stack so far apart that the whole last plane lies past 2^32 bytes:
    on the input side and on the output side of the gather and of the scatter, the other side with tight rows."""
    n, nplanes = 8, 3
    rows, cols = 24 * bs - (bs - 1), 37 * bs
    H, W = gpu.band_shape_n(rows, cols, bs, n)
    assert (H, W) == (24, 40)
    bands = stack_of([99, bs], nplanes, rows, cols)
    want_planes = np.concatenate([on.pre_transform(b, bs, n) for b in bands])
    # gather, far input: the bands' rows a far pitch apart
    lin = far_last_plane(nplanes * rows, rows, cols, 1)
    lout = far.Rows(nplanes * H, W * 8, W * 8 + 8)
    a, b = far.FarBuffer(gpu, lin.nbytes), far.FarBuffer(gpu, lout.nbytes)
    try:
        a.upload_rows(lin, bands.reshape(nplanes * rows, cols))
        gpu.band_planes_stacked_n_device(a.ptr, nplanes, rows, cols, bs, n, b.ptr, pitch=lin.pitch, out_pitch=lout.pitch // 8)
        assert np.array_equal(b.download_rows(lout, np.float64), want_planes)
        b.check_output(lout.extents(), "stacked gather, far input")
    finally:
        a.free()
        b.free()
    # gather, far output: the planes' rows a far pitch apart
    lin = far.Rows(nplanes * rows, cols, cols + 1)
    lout = far_last_plane(nplanes * H, H, W * 8, 8)
    a, b = far.FarBuffer(gpu, lin.nbytes), far.FarBuffer(gpu, lout.nbytes)
    try:
        a.upload_rows(lin, bands.reshape(nplanes * rows, cols))
        gpu.band_planes_stacked_n_device(a.ptr, nplanes, rows, cols, bs, n, b.ptr, pitch=lin.pitch, out_pitch=lout.pitch // 8)
        assert np.array_equal(b.download_rows(lout, np.float64), want_planes)
        b.check_output(lout.extents(), "stacked gather, far output")
    finally:
        a.free()
        b.free()
    planes = stack_of([98, bs], nplanes, H, W)
    want_bands = np.concatenate([np.repeat(np.repeat(p, bs, 0), bs, 1)[:rows, :cols] for p in planes])
    for side in ("in", "out"):
        lin = far_last_plane(nplanes * H, H, W, 1) if side == "in" else far.Rows(nplanes * H, W, W + 3)
        lout = far_last_plane(nplanes * rows, rows, cols, 1) if side == "out" else far.Rows(nplanes * rows, cols, cols + 5)
        a, b = far.FarBuffer(gpu, lin.nbytes), far.FarBuffer(gpu, lout.nbytes)
        try:
            a.upload_rows(lin, planes.reshape(nplanes * H, W))
            gpu.inflate_crop_stacked_u8_device(a.ptr, nplanes, H, lin.pitch, rows, cols, bs, b.ptr, out_pitch=lout.pitch)
            assert np.array_equal(b.download_rows(lout), want_bands)
            b.check_output(lout.extents(), "stacked scatter, far " + side)
        finally:
            a.free()
            b.free()
