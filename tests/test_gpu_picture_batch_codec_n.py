"""GPU: the batch codec for whole pictures on device buffers for dct_size != 8 (jpegx_batch_compress_pictures_n /
_decompress_pictures_n with the band batch's _status_n / _emit_n at nbands * npictures planes) and its Python surface.
Every comparison is exact.

The reference is the per-band device road on the MODEL's bands: jpegx.compress_band_n / decompress_band_n of
model[p][:, :, k], where the model pixels are the input or, with colour 1, tests/colour_model.py's YCbCr of it; on the way
back the per-band samples through np.dstack and colour_model's RGB.  One case runs against the product-free oracle of
tests/codec_oracle_n.py on its tie-free bands.

The shapes are the smallest that reach each mechanism: 22 and 43 pictures of one block per plane (66 and 129 planes, so
waves and groups of 64 blocks straddle pictures), group_planes 3, 6 and the recommended value with a short last group,
destinations 0, 1, 7 and 15 bytes behind a 16-byte boundary, both colours, and ONE workspace for all of them that is filled
once and never cleared."""
import numpy as np
import pytest

import codec_oracle_n as on
import colour_model
from batch_n_dev import CANARY, Fenced, band_shape, pitched
from test_codec_oracle_n import case_id, known

pytestmark = pytest.mark.gpu

WORKSPACE_BYTES = 64 << 20
NB = 3

# (N, bs, block rows, block columns, ragged, pictures, group_planes (None: recommended), destination skew, mode, param, colour)
CASES = [
    (2, 1, 1, 1, False, 22, None, 0, "none", 0.0, 0),
    (5, 1, 1, 1, False, 43, 6, 1, "none", 0.0, 1),
    (3, 1, 5, 13, False, 5, 3, 7, "discard", 2.0, 0),
    (3, 2, 5, 13, True, 5, 6, 15, "divide", 3.0, 1),
    (12, 1, 5, 7, True, 5, 6, 15, "divide", 40.0, 1),
    (12, 3, 5, 7, True, 4, 3, 1, "divide", 40.0, 0),
    (24, 5, 1, 1, True, 7, None, 7, "divide", 1000.0, 1),
    (24, 5, 2, 3, True, 5, 6, 0, "divide", 1000.0, 0),
    (32, 1, 8, 8, False, 1, 3, 0, "divide", 40.0, 0),
    (32, 1, 8, 8, False, 1, None, 1, "divide", 40.0, 1),
]


def cid(c):
    return "N%d-bs%d-%dx%d%s-p%d-g%s-s%d-%s%g-colour%d" % (c[0], c[1], c[2], c[3], "r" if c[4] else "", c[5], c[6], c[7], c[8], c[9], c[10])


@pytest.fixture(scope="module")
def workspace(gpu):
    """One workspace for every case of this module: filled with a pattern once, never cleared between calls."""
    buf = gpu.DeviceBuffer(WORKSPACE_BYTES)
    gpu.check(gpu.lib().jpegx_memset(buf.ptr, 0xC3, WORKSPACE_BYTES, None), "jpegx_memset")
    gpu.check(gpu.lib().jpegx_device_synchronize())
    yield buf
    buf.free()


def pictures_of(seed, npictures, rows, cols):
    """uint8 [npictures][rows][cols][3] of 8-bit noise; every third picture a smooth ramp instead."""
    px = np.random.default_rng(seed).integers(0, 256, (npictures, rows, cols, NB), dtype=np.uint8)
    y, x = np.mgrid[0:rows, 0:cols]
    for p in range(0, npictures, 3):
        for k in range(NB):
            px[p, :, :, k] = ((3 * y + 2 * x + 11 * p + 50 * k) // 4 % 256).astype(np.uint8)
    return px


def model_of(pixels, colour):
    return colour_model.rgb_to_ycbcr(pixels) if colour else pixels


@pytest.fixture(scope="module")
def reference():
    """(pixels, blobs of the model's bands by the per-band device road, picture-major) per case, made once and shared by the
    tests both ways."""
    cache = {}

    def get(gpu, case):
        if case not in cache:
            n, bs, hb, wb, ragged, npictures, _, _, mode, param, colour = case
            rows, cols = band_shape(hb, wb, n, bs, ragged)
            pixels = pictures_of([n, bs, hb, wb, npictures], npictures, rows, cols)
            model = model_of(pixels, colour)
            blobs = [gpu.compress_band_n(np.ascontiguousarray(model[p][:, :, k]), bs, n, mode, param) for p in range(npictures) for k in range(NB)]
            assert all(isinstance(b, bytes) and b for b in blobs)
            pixels.setflags(write=False)
            cache[case] = (pixels, blobs)
        return cache[case]
    return get


def offsets_of(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    return off


def group_planes_of(gpu, gp, rows, cols, bs, n):
    rec = gpu.batch_group_planes_pictures_n(NB, rows, cols, bs, n)
    assert rec >= NB and rec % NB == 0
    return rec if gp is None else gp


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_compress_equals_the_per_band_road(gpu, workspace, reference, case):
    n, bs, hb, wb, ragged, npictures, gp, skew, mode, param, colour = case
    pixels, want = reference(gpu, case)
    _, rows, cols, _ = pixels.shape
    gp = group_planes_of(gpu, gp, rows, cols, bs, n)
    nplanes = NB * npictures
    pics, planes = (npictures, NB, rows, cols, bs, n), (nplanes, rows, cols, bs, n)
    assert gpu.band_shape_n(rows, cols, bs, n) == (hb * n, wb * n)
    assert 0 < gpu.batch_workspace_bytes_n(*planes, gp) <= WORKSPACE_BYTES
    off, total = offsets_of(want), sum(len(b) for b in want)
    assert total <= gpu.batch_max_bytes_n(*planes)
    pitch = cols * NB + 5
    din = Fenced(gpu, npictures * rows * pitch, skew=3)
    dout = Fenced(gpu, total + 64, skew=skew)
    try:
        stacked = pitched(pixels.reshape(npictures * rows, cols * NB), pitch, 0xEE)
        din.upload(stacked)
        # sizes only
        gpu.batch_compress_pictures_n_device(din.ptr, *pics, workspace.ptr, None, 0, gp, mode, param, colour, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status_n(workspace.ptr, *planes, gp)
        assert (rc, got_total) == (0, total)
        assert np.array_equal(got_off, off)               # the cumulated per-band lengths
        # one byte short: nothing is written, the verdict is 1, and the emit step completes the job
        gpu.batch_compress_pictures_n_device(din.ptr, *pics, workspace.ptr, dout.ptr, total - 1, gp, mode, param, colour, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status_n(workspace.ptr, *planes, gp)
        assert (rc, got_total) == (1, total) and np.array_equal(got_off, off)
        dout.untouched("a compress one byte short")
        gpu.batch_emit_n_device(workspace.ptr, *planes, dout.ptr, total, gp)
        rc, got_total, _ = gpu.batch_compress_status_n(workspace.ptr, *planes, gp)
        assert (rc, got_total) == (0, total)
        got = dout.payload(total, "emit").tobytes()
        for q in range(nplanes):
            assert got[int(off[q]):int(off[q + 1])] == want[q], "band %d of picture %d of %s" % (q % NB, q // NB, cid(case))
        # the input is never written
        front, body, back = din.everything()
        assert np.all(front == CANARY) and np.all(back == CANARY)
        assert np.array_equal(body[:stacked.size].reshape(stacked.shape), stacked), "compress wrote to its input"
    finally:
        din.free()
        dout.free()


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_decompress_equals_the_per_band_road(gpu, workspace, reference, case):
    n, bs, hb, wb, ragged, npictures, gp, skew, mode, param, colour = case
    pixels, blobs = reference(gpu, case)
    _, rows, cols, _ = pixels.shape
    gp = group_planes_of(gpu, gp, rows, cols, bs, n)
    pics = (npictures, NB, rows, cols, bs, n)
    bands = [gpu.decompress_band_n(b, rows, cols, bs, n, mode, param) for b in blobs]
    want = np.stack([np.dstack(bands[NB * p:NB * p + NB]) for p in range(npictures)])
    if colour:
        want = colour_model.ycbcr_to_rgb(want)
    off, total = offsets_of(blobs), sum(len(b) for b in blobs)
    first = gpu.batch_groups_pictures_n(off, *pics, gp)
    assert np.array_equal(first, list(range(0, npictures, gp // NB)) + [npictures])
    assert 0 < gpu.batch_decompress_pictures_workspace_bytes_n(total, *pics, gp) <= WORKSPACE_BYTES
    opitch = cols * NB + 7
    din = Fenced(gpu, total, skew=skew)                   # no slack behind the stream, any alignment
    dout = Fenced(gpu, npictures * rows * opitch, skew=1)
    try:
        din.upload(np.frombuffer(b"".join(blobs), np.uint8))
        gpu.batch_decompress_pictures_n_device(din.ptr, off, *pics, workspace.ptr, dout.ptr, gp, opitch, mode, param, colour)
        got = dout.payload(dout.nbytes, "decompress").reshape(npictures, rows, opitch)
        assert np.array_equal(got[:, :, :cols * NB].reshape(npictures, rows, cols, NB), want)
        assert np.all(got[:, :, cols * NB:] == CANARY), "the pitch slack was written"
    finally:
        din.free()
        dout.free()


FREE_CASE = [c for c in on.matrix_cases() if c[5] == "free"][0]


def test_both_ways_against_the_oracle(gpu):
    """Three pictures whose three bands are all one tie-free band, as one batch in groups of two pictures, colour 0: the
    oracle's bytes nine times, and the oracle's band back in every band of every picture."""
    k = known(FREE_CASE)
    band = np.ascontiguousarray(k.band, np.uint8)
    pixels = np.stack([np.dstack([band] * NB)] * 3)
    blobs = gpu.batch_compress_pictures_n(pixels, k.bs, k.n, k.mode, k.param, group_planes=2 * NB)
    assert blobs == [[k.blob] * NB] * 3, k.what
    back = gpu.batch_decompress_pictures_n(blobs, k.h, k.w, k.bs, k.n, k.mode, k.param, group_planes=2 * NB)
    assert back.dtype == np.uint8 and back.shape == (3, k.h, k.w, NB)
    whole = k.mode != "divide" or k.param == np.trunc(k.param)
    want = k.inv.band if whole else gpu.decompress_band_n(k.blob, k.h, k.w, k.bs, k.n, k.mode, k.param)
    for p in range(3):
        for b in range(NB):
            assert np.array_equal(back[p, :, :, b], want), (case_id(FREE_CASE), p, b)


def test_an_amplitude_beyond_15_bits_in_the_middle_of_the_batch(gpu, workspace):
    """Peak 255 at N 16 without a divisor: a DC of 255 * 256 = 65280.  One such band in the third of five quiet pictures."""
    n, bs, rows, cols, npictures, gp = 16, 1, 32, 48, 5, 6
    pixels = np.full((npictures, rows, cols, NB), 8, np.uint8)
    pixels[2, :, :, 1] = 255
    pics, planes = (npictures, NB, rows, cols, bs, n), (npictures * NB, rows, cols, bs, n)
    din, dout = Fenced(gpu, pixels.nbytes), Fenced(gpu, 8192, skew=1)
    try:
        din.upload(pixels)
        gpu.batch_compress_pictures_n_device(din.ptr, *pics, workspace.ptr, dout.ptr, 8192, gp, "none", 0.0, 0)
        rc, _, _ = gpu.batch_compress_status_n(workspace.ptr, *planes, gp)
        assert rc == -1 and b"BadRleCodeError" in gpu.lib().jpegx_last_error()
        dout.untouched("a refused compress")
        with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
            gpu.batch_compress_pictures_n(pixels, bs, n, "none", 0.0)
        # the same workspace takes the next batch as it is
        pixels[2, :, :, 1] = 8
        din.upload(pixels)
        gpu.batch_compress_pictures_n_device(din.ptr, *pics, workspace.ptr, dout.ptr, 8192, gp, "none", 0.0, 0)
        rc, total, off = gpu.batch_compress_status_n(workspace.ptr, *planes, gp)
        assert rc == 0
        want = gpu.compress_band_n(np.full((rows, cols), 8, np.uint8), bs, n, "none", 0.0)
        assert dout.payload(total, "compress").tobytes() == want * (npictures * NB)
    finally:
        din.free()
        dout.free()


def test_a_damaged_picture_in_the_second_group(gpu, workspace):
    """Five RGB pictures in groups of two; band 1 of picture 3 is damaged by bytes the host parser refuses (a chain code that
    runs past the block).  The error names pictures 2..3, the first group's pictures are written, nothing of the second or the
    third group is."""
    n, bs, npictures, gp = 4, 2, 5, 6
    rows, cols = band_shape(3, 4, n, bs, True)
    pixels = pictures_of(5, npictures, rows, cols)
    model = model_of(pixels, 1)
    pics = (npictures, NB, rows, cols, bs, n)
    blobs = [gpu.compress_band_n(np.ascontiguousarray(model[p][:, :, k]), bs, n, "divide", 3.0) for p in range(npictures) for k in range(NB)]
    off = offsets_of(blobs)
    bands = [gpu.decompress_band_n(b, rows, cols, bs, n, "divide", 3.0) for b in blobs]
    want = colour_model.ycbcr_to_rgb(np.stack([np.dstack(bands[NB * p:NB * p + NB]) for p in range(npictures)]))
    stream = np.frombuffer(b"".join(blobs), np.uint8).copy()
    din, dout = Fenced(gpu, stream.size), Fenced(gpu, npictures * rows * cols * NB)
    try:
        din.upload(stream)
        gpu.batch_decompress_pictures_n_device(din.ptr, off, *pics, workspace.ptr, dout.ptr, gp, None, "divide", 3.0, 1)
        assert np.array_equal(dout.payload(dout.nbytes, "decompress").reshape(want.shape), want)
        q = 3 * NB + 1                                    # band 1 of picture 3
        stream[int(off[q]):int(off[q]) + 2] = 0xF0       # 0xF0 chain codes: more than 16 zeros in a block of 16 coefficients
        bad = stream[int(off[q]):int(off[q + 1])].tobytes()
        with pytest.raises(gpu.JpegxError):
            gpu.entropy_decode_n(bad, 12, n * n)           # the host parser refuses it
        din.upload(stream)
        dout.fill()
        with pytest.raises(gpu.JpegxError, match=r"pictures 2\.\.3"):
            gpu.batch_decompress_pictures_n_device(din.ptr, off, *pics, workspace.ptr, dout.ptr, gp, None, "divide", 3.0, 1)
        got = dout.payload(2 * rows * cols * NB, "a refused second group").reshape(2, rows, cols, NB)
        assert np.array_equal(got, want[:2])
        nested = [blobs[NB * p:NB * p + NB] for p in range(npictures)]
        nested[3][1] = bad
        with pytest.raises(gpu.JpegxError, match=r"pictures 2\.\.3"):
            gpu.batch_decompress_pictures_n(nested, rows, cols, bs, n, "divide", 3.0, colour="rgb", group_planes=gp)
    finally:
        din.free()
        dout.free()


def test_python_surface_equals_the_per_band_functions(gpu, reference):
    """jpegx.batch_compress_pictures_n / batch_decompress_pictures_n with the recommended group on the README example."""
    case = CASES[7]
    n, bs, _, _, _, npictures, _, _, mode, param, colour = case
    pixels, want = reference(gpu, case)
    _, rows, cols, _ = pixels.shape
    nested = [want[NB * p:NB * p + NB] for p in range(npictures)]
    assert gpu.batch_compress_pictures_n(pixels, bs, n, mode, param) == nested
    bands = [gpu.decompress_band_n(b, rows, cols, bs, n, mode, param) for b in want]
    back = np.stack([np.dstack(bands[NB * p:NB * p + NB]) for p in range(npictures)])
    assert np.array_equal(gpu.batch_decompress_pictures_n(nested, rows, cols, bs, n, mode, param), back)
    assert np.array_equal(gpu.batch_decompress_pictures_n(nested, rows, cols, bs, n, mode, param, colour="rgb"), colour_model.ycbcr_to_rgb(back))
