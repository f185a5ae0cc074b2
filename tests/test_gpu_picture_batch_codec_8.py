"""GPU: the batch codec for whole pictures at dct_size 8 on device buffers (jpegx_batch_compress_pictures /
jpegx_batch_decompress_pictures with the band batch's jpegx_batch_compress_status / jpegx_batch_emit at nbands * npictures
planes) and its Python surface.  Every comparison is exact.

The reference for compress is the per-band host job on the MODEL's bands: jpegx.compress_plane_native(model[p][:, :, k],
ragged=True), where the model pixels are the input or, with colour 1, tests/colour_model.py's YCbCr of it; two cases are
also held against the product-free oracle, codec_oracle.compress_reference.  The reference for decompress is
codec_oracle.decompress_reference per band, then np.dstack and colour_model's RGB.

Cases: the uint8 road (block_size 1, 2, 4, padded rows of a multiple of 16 bytes) with 22 and 43 pictures of two blocks a
plane (66 and 129 planes: waves of 64 blocks straddle pictures) and the ragged 37 x 53 and 9 x 130; the float64 road with
block_size 1 at W = 8 and W = 24, and block_size 3 and 5 on the ragged 44 x 70 and 23 x 41, in groups of 3 and 6 planes and
of the recommended size, 5 pictures in groups of 2 ending in a short last group; every quantiser (qtable, none, discard 2,
divide 7); destinations 0, 1, 7 and 15 bytes behind a 16-byte boundary; both colours; ONE workspace for all of them that is
filled with a pattern once and never cleared.  8-bit input cannot reach the 15-bit amplitude limit at 8 x 8 (no coefficient
of 64 samples of at most 255 passes 64 * 255 = 16 320 < 16 383), so no case is skipped for a BadRleCodeError."""
import numpy as np
import pytest

import codec_oracle
import colour_model
import oracle
from batch_n_dev import CANARY, Fenced, pitched

pytestmark = pytest.mark.gpu

WORKSPACE_BYTES = 64 << 20
NB = 3

# (road, bs, rows, cols, pictures, group_planes (None: recommended), destination skew, mode, param, colour)
CASES = [
    ("u8", 1, 8, 16, 22, None, 0, "qtable", 0.0, 0),
    ("u8", 1, 8, 16, 43, 3, 1, "none", 0.0, 1),
    ("u8", 2, 37, 53, 3, None, 7, "divide", 7.0, 1),
    ("u8", 2, 37, 53, 2, 6, 15, "qtable", 0.0, 0),
    ("u8", 4, 9, 130, 3, 3, 15, "discard", 2.0, 0),
    ("u8", 4, 9, 130, 2, None, 1, "qtable", 0.0, 1),
    ("f64", 1, 8, 8, 5, 6, 7, "qtable", 0.0, 1),
    ("f64", 1, 13, 20, 4, 3, 0, "none", 0.0, 0),
    ("f64", 3, 44, 70, 5, 6, 1, "divide", 7.0, 1),
    ("f64", 3, 44, 70, 2, None, 15, "qtable", 0.0, 0),
    ("f64", 5, 23, 41, 5, 6, 0, "discard", 2.0, 0),
    ("f64", 5, 23, 41, 3, 3, 7, "qtable", 0.0, 1),
]
ORACLE_CASES = (CASES[3], CASES[8])          # also against codec_oracle.compress_reference


def cid(c):
    return "%s-bs%d-%dx%d-p%d-g%s-s%d-%s%g-colour%d" % c


@pytest.fixture(scope="module")
def workspace(gpu):
    """One workspace for every case of this module: filled with a pattern once, never cleared between calls."""
    buf = gpu.DeviceBuffer(WORKSPACE_BYTES)
    assert buf.ptr % 256 == 0
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
    """(pixels, blobs of the model's bands by the per-band host job, picture-major) per case, made once and shared by the
    tests both ways."""
    cache = {}

    def get(gpu, case):
        if case not in cache:
            _, bs, rows, cols, npictures, _, _, mode, param, colour = case
            pixels = pictures_of([bs, rows, cols, npictures], npictures, rows, cols)
            model = model_of(pixels, colour)
            blobs = [gpu.compress_plane_native(np.ascontiguousarray(model[p][:, :, k]), bs, mode, param, ragged=True)
                     for p in range(npictures) for k in range(NB)]
            assert all(isinstance(b, bytes) and b for b in blobs)
            pixels.setflags(write=False)
            cache[case] = (pixels, blobs)
        return cache[case]
    return get


def offsets_of(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    return off


def group_planes_of(gpu, gp, rows, cols, bs):
    rec = gpu.batch_group_planes_pictures_n(NB, rows, cols, bs, 8)
    assert rec >= NB and rec % NB == 0
    return rec if gp is None else gp


def road_of(gpu, rows, cols, bs):
    return "u8" if bs in (1, 2, 4) and (gpu.padded_shape(rows, cols, bs)[1] * bs) % 16 == 0 else "f64"


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_compress_equals_the_per_band_job(gpu, workspace, reference, case):
    road, bs, rows, cols, npictures, gp, skew, mode, param, colour = case
    pixels, want = reference(gpu, case)
    assert road_of(gpu, rows, cols, bs) == road
    gp = group_planes_of(gpu, gp, rows, cols, bs)
    nplanes = NB * npictures
    h, w = gpu.padded_shape(rows, cols, bs)
    pics, planes = (npictures, NB, rows, cols, bs), (nplanes, h, w)
    assert 0 < gpu.batch_pictures_workspace_bytes(*pics, gp) <= WORKSPACE_BYTES
    off, total = offsets_of(want), sum(len(b) for b in want)
    assert total <= gpu.batch_max_bytes(*planes)
    if case in ORACLE_CASES:
        model = model_of(pixels, colour)
        for q in range(nplanes):
            assert want[q] == codec_oracle.compress_reference(model[q // NB][:, :, q % NB], bs, mode, param), (q, cid(case))
    pitch = cols * NB + 5
    din = Fenced(gpu, npictures * rows * pitch, skew=3)
    dout = Fenced(gpu, total + 64, skew=skew)
    try:
        stacked = pitched(pixels.reshape(npictures * rows, cols * NB), pitch, 0xEE)
        din.upload(stacked)
        # sizes only -> status -> (below) jpegx_batch_emit
        gpu.batch_compress_pictures_device(din.ptr, *pics, workspace.ptr, None, 0, gp, mode, param, colour, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status(workspace.ptr, *planes)
        assert (rc, got_total) == (0, total)
        assert np.array_equal(got_off, off)               # the cumulated per-band lengths
        # one byte short: nothing is written, the verdict is 1, and the emit step completes the job
        gpu.batch_compress_pictures_device(din.ptr, *pics, workspace.ptr, dout.ptr, total - 1, gp, mode, param, colour, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status(workspace.ptr, *planes)
        assert (rc, got_total) == (1, total) and np.array_equal(got_off, off)
        dout.untouched("a compress one byte short")
        gpu.batch_emit_device(workspace.ptr, *planes, dout.ptr, total)
        rc, got_total, _ = gpu.batch_compress_status(workspace.ptr, *planes)
        assert (rc, got_total) == (0, total)
        got = dout.payload(total, "emit").tobytes()
        for q in range(nplanes):
            assert got[int(off[q]):int(off[q + 1])] == want[q], "band %d of picture %d of %s" % (q % NB, q // NB, cid(case))
        # in one call, with room to spare
        dout.fill()
        gpu.batch_compress_pictures_device(din.ptr, *pics, workspace.ptr, dout.ptr, total + 64, gp, mode, param, colour, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status(workspace.ptr, *planes)
        assert (rc, got_total) == (0, total) and np.array_equal(got_off, off)
        assert dout.payload(total, "compress").tobytes() == b"".join(want)
        # the input is never written
        front, body, back = din.everything()
        assert np.all(front == CANARY) and np.all(back == CANARY)
        assert np.array_equal(body[:stacked.size].reshape(stacked.shape), stacked), "compress wrote to its input"
    finally:
        din.free()
        dout.free()


def reference_pictures(blobs, npictures, rows, cols, bs, mode, param, colour):
    bands = [codec_oracle.decompress_reference(b, rows, cols, bs, mode, param) for b in blobs]
    want = np.stack([np.dstack(bands[NB * p:NB * p + NB]) for p in range(npictures)]).astype(np.uint8)
    return colour_model.ycbcr_to_rgb(want) if colour else want


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_decompress_equals_the_oracle(gpu, workspace, reference, case):
    _, bs, rows, cols, npictures, _, skew, mode, param, colour = case
    _, blobs = reference(gpu, case)
    pics = (npictures, NB, rows, cols, bs)
    want = reference_pictures(blobs, npictures, rows, cols, bs, mode, param, colour)
    off, total = offsets_of(blobs), sum(len(b) for b in blobs)
    assert 0 < gpu.batch_decompress_pictures_workspace_bytes(total, *pics) <= WORKSPACE_BYTES
    opitch = cols * NB + 7
    din = Fenced(gpu, total + 16, skew=skew)
    dout = Fenced(gpu, npictures * rows * opitch, skew=1)
    try:
        din.upload(np.frombuffer(b"".join(blobs) + bytes(16), np.uint8))
        gpu.batch_decompress_pictures_device(din.ptr, off, *pics, workspace.ptr, dout.ptr, opitch, mode, param, colour)
        got = dout.payload(dout.nbytes, "decompress").reshape(npictures, rows, opitch)
        assert np.array_equal(got[:, :, :cols * NB].reshape(npictures, rows, cols, NB), want)
        assert np.all(got[:, :, cols * NB:] == CANARY), "the pitch slack was written"
    finally:
        din.free()
        dout.free()


def test_a_stream_with_one_damaged_byte_writes_nothing(gpu, workspace, reference):
    """One byte of band 1 of picture 1 changed so that the sequential parser refuses the stream: decompress refuses it, names
    the planes, and every byte of d_out still holds the canary -- the scatter runs only after the decoder's verdict.  The same
    workspace then takes the undamaged stream."""
    case = CASES[3]
    _, bs, rows, cols, npictures, _, _, mode, param, colour = case
    _, blobs = reference(gpu, case)
    pics = (npictures, NB, rows, cols, bs)
    h, w = gpu.padded_shape(rows, cols, bs)
    nblocks = NB * npictures * (h // 8) * (w // 8)
    off, stream = offsets_of(blobs), b"".join(blobs)

    def refuses(data):
        try:
            oracle.rle_decode(data, nblocks)
        except oracle.RleStreamError:
            return True
        return False

    q, bad = NB + 1, None
    for pos in range(int(off[q]) + 3, int(off[q + 1]) - 3):
        for flip in (0xFF, 0x40, 0x0F):
            cand = bytearray(stream)
            cand[pos] ^= flip
            if refuses(bytes(cand)):
                bad = bytes(cand)
                break
        if bad:
            break
    assert bad is not None and len(bad) == len(stream) and sum(a != b for a, b in zip(bad, stream)) == 1
    din, dout = Fenced(gpu, len(stream) + 16), Fenced(gpu, npictures * rows * cols * NB, skew=7)
    try:
        din.upload(np.frombuffer(bad + bytes(16), np.uint8))
        with pytest.raises(gpu.JpegxError, match=r"planes \d+\.\.\d+"):
            gpu.batch_decompress_pictures_device(din.ptr, off, *pics, workspace.ptr, dout.ptr, None, mode, param, colour)
        dout.untouched("a refused decompress")
        nested = [[bad[int(off[NB * p + k]):int(off[NB * p + k + 1])] for k in range(NB)] for p in range(npictures)]
        with pytest.raises(gpu.JpegxError, match=r"planes \d+\.\.\d+"):
            gpu.batch_decompress_pictures(nested, rows, cols, bs, mode, param)
        din.upload(np.frombuffer(stream + bytes(16), np.uint8))
        gpu.batch_decompress_pictures_device(din.ptr, off, *pics, workspace.ptr, dout.ptr, None, mode, param, colour)
        want = reference_pictures(blobs, npictures, rows, cols, bs, mode, param, colour)
        assert np.array_equal(dout.payload(dout.nbytes, "decompress").reshape(want.shape), want)
    finally:
        din.free()
        dout.free()


def test_the_brightest_pictures_stay_below_the_amplitude_limit(gpu, workspace):
    """All-255 pictures with mode none, the largest DC 8-bit samples can make (255 * 8 = 2040, below 16 383): the verdict is
    OK on both roads and the bytes are the per-band job's."""
    for bs, rows, cols in ((1, 8, 16), (3, 20, 20)):
        px = np.full((2, rows, cols, NB), 255, np.uint8)
        want = gpu.compress_plane_native(np.ascontiguousarray(px[0][:, :, 0]), bs, "none", 0.0, ragged=True)
        assert gpu.batch_compress_pictures(px, bs, "none", 0.0) == [[want] * NB] * 2


@pytest.mark.parametrize("case", [CASES[2], CASES[8]], ids=cid)
def test_python_surface(gpu, reference, case):
    """jpegx.batch_compress_pictures / batch_decompress_pictures with the recommended group, on one case of each road."""
    _, bs, rows, cols, npictures, _, _, mode, param, colour = case
    pixels, want = reference(gpu, case)
    nested = [want[NB * p:NB * p + NB] for p in range(npictures)]
    kw = {"colour": "rgb"} if colour else {}
    assert gpu.batch_compress_pictures(pixels, bs, mode, param, **kw) == nested
    assert gpu.batch_compress_pictures(pixels, bs, mode, param, group_planes=NB, **kw) == nested
    back = gpu.batch_decompress_pictures(nested, rows, cols, bs, mode, param, **kw)
    assert back.dtype == np.uint8 and back.shape == (npictures, rows, cols, NB)
    assert np.array_equal(back, reference_pictures(want, npictures, rows, cols, bs, mode, param, colour))
