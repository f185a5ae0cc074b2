"""GPU: bands and pictures of ANY size compressed on the device -- the margin-fill kernel alone (jpegx_pad_edges), one band
(jpegx_host_compress_begin_ragged), whole pictures (jpegx_host_compress_image_ragged / _packed_ragged behind
Jpeg.compress), the batch codec fed by jpegx_padded_shape + jpegx_pad_edges, and the aligned shapes that must not change.
Everything goes through the C ABI and every comparison is exact (bytes with ==, arrays with np.array_equal): the feature
is integer and bit-exact by construction.  The reference is tests/codec_oracle.py.

The Python wrappers take bands of any size with ``ragged=True``; without it they keep answering None for a plane that is
not whole 8 * block_size tiles, which tests/test_gpu_codec_roads.py asserts for the same calls."""
import ctypes
import glob
import os

import numpy as np
import pytest

import file_format
import pipeline
from codec_oracle import blocks_of, compress_reference, decompress_reference
from conftest import GOLDEN, MODES
from pipeline import CompressedData, Configuration, QuantizationMethod

pytestmark = pytest.mark.gpu

BLOCK_SIZES = [1, 2, 3, 4, 5, 7, 16]
SHAPES = [(1, 17), (29, 1), (37, 53), (23, 41), (9, 130), (7, 300), (50, 50), (33, 64), (1080, 1920)]
BAND_SHAPES = SHAPES[:8] + [(20, 28)]          # (20, 28) with block_size 1: a padded row of 24 samples, 8 mod 16
SENTINEL = 0xA5


def method(mode, param):
    if mode == "divide":
        return QuantizationMethod("divide", divisor=param)
    if mode == "discard":
        return QuantizationMethod("discard", keep=int(param))
    return QuantizationMethod(mode)


def gather(gpu, band, bs):
    sy, sx = gpu.edge_source_indices(band.shape[0], bs), gpu.edge_source_indices(band.shape[1], bs)
    return band[sy][:, sx]


def stacked(gpu, planes, bs, slack):
    """The planes in a sentinel-filled stacked buffer of the padded shape with `slack` elements of pitch behind each row;
    returns (buffer, Hraw, Wraw)."""
    rows, cols = planes[0].shape
    h, w = gpu.padded_shape(rows, cols, bs)
    hraw, wraw = h * bs, w * bs
    buf = np.full((len(planes) * hraw, wraw + slack), SENTINEL, dtype=planes[0].dtype)
    for p, plane in enumerate(planes):
        buf[p * hraw:p * hraw + rows, :cols] = plane
    return buf, hraw, wraw


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("nplanes", [1, 3])
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_pad_edges_writes_the_margins_and_nothing_else(gpu, bs, nplanes, dtype):
    for k, (rows, cols) in enumerate(SHAPES + [(16 * bs, 32 * bs)]):          # the last one has no margin at all
        rng = np.random.default_rng(31 * bs + 7 * k + nplanes)
        planes = [rng.integers(0, 256, (rows, cols)).astype(dtype) for _ in range(nplanes)]
        aligned = 16 // np.dtype(dtype).itemsize
        slack = aligned if k % 2 == 0 else aligned - 3 + 8                     # rows 16-byte aligned, or not
        buf, hraw, wraw = stacked(gpu, planes, bs, slack)
        got = gpu.pad_edges(buf, rows, cols, bs)
        tag = (rows, cols, bs, nplanes, dtype)
        assert got.shape == buf.shape and got.dtype == buf.dtype, tag
        for p, plane in enumerate(planes):
            rect = got[p * hraw:(p + 1) * hraw, :wraw]
            assert np.array_equal(rect[:rows, :cols], plane), tag              # the picture is untouched
            assert np.array_equal(rect, gather(gpu, plane, bs)), tag           # the rectangle is the gather
        assert np.all(got[:, wraw:] == SENTINEL), tag                          # the pitch slack is untouched
        if (hraw, wraw) == (rows, cols):
            assert np.array_equal(got, buf), tag


def golden_bands():
    out = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, "case_ragged*.npz"))):
        case = np.load(f)
        out.append((os.path.basename(f), case["input"], int(case["block_size"])))
    return out


@pytest.mark.parametrize("suffix,mode,param", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_one_band_of_any_shape_is_one_native_call(gpu, bs, suffix, mode, param):
    for k, (rows, cols) in enumerate(BAND_SHAPES):
        rng = np.random.default_rng(97 * bs + k)
        band = rng.integers(0, 256, (rows, cols))
        want = compress_reference(band, bs, mode, param)
        for dtype in (np.uint8, np.int32, np.int64):
            got = gpu.compress_plane_native(np.ascontiguousarray(band.astype(dtype)), bs, mode, param, ragged=True)
            assert isinstance(got, bytes) and got == want, (rows, cols, bs, mode, np.dtype(dtype).name)


@pytest.mark.parametrize("suffix,mode,param", MODES, ids=[m[0] for m in MODES])
def test_golden_ragged_bands(gpu, suffix, mode, param):
    bands = golden_bands()
    assert len(bands) >= 9
    for k, (name, band, bs) in enumerate(bands):
        want = compress_reference(band, bs, mode, param)
        dtype = (np.uint8, np.int32, np.int64)[k % 3]
        assert gpu.compress_plane_native(np.ascontiguousarray(band.astype(dtype)), bs, mode, param, ragged=True) == want, name
        cfg = Configuration(width=band.shape[1], height=band.shape[0], block_size=bs, quantization=method(mode, param))
        assert pipeline.compress_band(band, cfg) == want, name


def test_padded_row_of_8_mod_16_at_block_size_1(gpu):
    """20 x 28 pads to 24 x 32 -- fine; 20 x 20 pads to 24 x 24, a row the uint8 forward kernel does not take: the ragged
    entry goes through the float64 road (same bytes), the entry for whole tiles keeps refusing the shape."""
    L = gpu.lib()
    for rows, cols in [(20, 28), (20, 20), (24, 24), (3, 9)]:
        band = np.random.default_rng(rows * cols).integers(0, 256, (rows, cols)).astype(np.uint8)
        for _suffix, mode, param in MODES:
            assert gpu.compress_plane_native(band, 1, mode, param, ragged=True) == compress_reference(band, 1, mode, param), (rows, cols, mode)
    whole = np.zeros((24, 24), np.uint8)
    n = ctypes.c_size_t(0)
    assert L.jpegx_host_compress_begin(whole.ctypes.data, 1, 24, 24, 24, 1, gpu.Q_QTABLE, 0.0, ctypes.byref(n)) == -4
    assert gpu.compress_plane_native(whole, 1, "qtable", 0.0) is None


def test_a_band_outside_8_bits_is_still_refused(gpu):
    """JPEGX_E_UNSUPPORTED from the C entry (None from the wrapper), wherever the sample stands; the pool is fine after."""
    L = gpu.lib()
    band = np.random.default_rng(256).integers(0, 256, (37, 53)).astype(np.int64)
    want = compress_reference(band, 2, "qtable")
    for y, x, v in [(0, 0, 256), (36, 52, 256), (17, 29, -1), (36, 0, 1 << 40)]:
        for dtype in (np.int32, np.int64):
            bad = band.astype(dtype)
            bad[y, x] = v if dtype == np.int64 or abs(v) < 2 ** 31 else 300
            n = ctypes.c_size_t(0)
            rc = L.jpegx_host_compress_begin_ragged(bad.ctypes.data, bad.dtype.itemsize, 37, 53, 53, 2, gpu.Q_QTABLE, 0.0, ctypes.byref(n))
            assert rc == -4 and b"0..255" in L.jpegx_last_error(), (y, x, v)
            assert gpu.compress_plane_native(bad, 2, "qtable", 0.0, ragged=True) is None
        assert gpu.compress_plane_native(band, 2, "qtable", 0.0, ragged=True) == want
    cfg = Configuration(width=53, height=37, block_size=2, quantization=QuantizationMethod("qtable"))
    bad = band.copy()
    bad[5, 5] = 256
    assert pipeline.compress_band(bad, cfg) == compress_reference(bad, 2, "qtable")      # the host road takes what the device refuses


def picture(rows, cols, seed):
    """Three different bands: smooth, noise, and a mix with hard edges."""
    rng = np.random.default_rng(seed)
    i, j = np.indices((rows, cols))
    smooth = np.rint(127.5 + 120 * np.sin(i / 9.0 + 0.3) * np.cos(j / 13.0)).astype(np.uint8)
    noise = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    mix = np.where(((i // 5 + j // 11) & 1) == 1, noise, 255 - smooth).astype(np.uint8)
    return [smooth, noise, mix]


@pytest.mark.parametrize("bs", [1, 2, 4, 5])
@pytest.mark.parametrize("rows,cols", [(37, 53), (131, 257), (1080, 1920)])
def test_whole_picture_of_any_size_is_one_native_job(gpu, monkeypatch, rows, cols, bs):
    from PIL import Image
    mode, param = [("qtable", 0.0), ("divide", 40.0), ("none", 0.0), ("discard", 2.0)][(bs + rows) % 4]
    cfg = Configuration(width=cols, height=rows, block_size=bs, quantization=method(mode, param))
    bands = picture(rows, cols, 1000 * bs + rows)
    wants = [compress_reference(b, bs, mode, param) for b in bands]
    container = file_format.generate_data(cfg, CompressedData(*wants))
    image = Image.frombytes("YCbCr", (cols, rows), np.ascontiguousarray(np.dstack(bands)).tobytes())

    def no_band_road(*_args, **_kwargs):
        raise AssertionError("the picture went band by band through compress_band")
    monkeypatch.setattr(pipeline, "compress_band", no_band_road)
    assert pipeline.Jpeg(cfg).compress(image) == container                                   # packed pixels
    assert pipeline._compress_pixels(image, cfg) == container
    assert pipeline._compress_image([np.asarray(b) for b in image.split()], cfg) == container    # split bands
    assert gpu.compress_image_packed(np.asarray(image), bs, mode, param, ragged=True) == wants
    assert gpu.compress_image_native([b.astype(np.int64) for b in bands], bs, mode, param, ragged=True) == wants
    monkeypatch.undo()
    back = pipeline.Jpeg.decompress(container)
    refs = [decompress_reference(x, rows, cols, bs, mode, param) for x in wants]
    assert back.mode == "YCbCr" and back.size == (cols, rows)
    assert np.array_equal(np.asarray(back), np.dstack(refs).astype(np.uint8))


@pytest.mark.parametrize("dtype,bs", [("uint8", 2), ("float32", 1)])
def test_batch_codec_on_ragged_planes(gpu, dtype, bs):
    """Five 45 x 77 planes in a jpegx_padded_shape buffer: jpegx_pad_edges, then jpegx_batch_compress on the same stream;
    jpegx_batch_decompress writes planes of the padded shape, of which the caller reads 45 x 77."""
    rows, cols, n = 45, 77, 5
    mode, param = "qtable", 0.0
    rng = np.random.default_rng(4577 + bs)
    planes = [rng.integers(0, 256, (rows, cols)).astype(dtype) for _ in range(n)]
    planes[1] = np.rint(127.5 + 100 * np.sin(np.indices((rows, cols))[0] / 7.0)).astype(dtype)
    h, w = gpu.padded_shape(rows, cols, bs)
    assert (h, w) == tuple(8 * v for v in blocks_of(rows, cols, bs))
    buf, hraw, wraw = stacked(gpu, planes, bs, 0)
    elem = buf.dtype.itemsize
    L = gpu.lib()
    cap = gpu.batch_max_bytes(n, h, w)
    din, dws, dout = gpu.DeviceBuffer(buf.nbytes), gpu.DeviceBuffer(gpu.batch_workspace_bytes(n, h, w)), gpu.DeviceBuffer(cap + 16)
    dws2 = dback = None
    try:
        din.upload(buf)
        gpu.check(L.jpegx_memset(dout.ptr, 0, cap + 16, None), "jpegx_memset")
        gpu.check(L.jpegx_pad_edges(din.ptr, elem, n, rows, cols, bs, wraw, None), "jpegx_pad_edges")
        gpu.batch_compress_device(din.ptr, elem, n, h, w, dws.ptr, dout.ptr, cap, mode, param,
                                  gpu.F_PIXEL_INPUT if elem == 4 else 0, pitch=wraw, block_size=bs)
        rc, total, off = gpu.batch_compress_status(dws.ptr, n, h, w)
        assert rc == 0 and total == int(off[n])
        blob = dout.download((total,), np.uint8).tobytes()
        wants = [compress_reference(p, bs, mode, param) for p in planes]
        for p in range(n):
            assert blob[int(off[p]):int(off[p + 1])] == wants[p], p
        dws2 = gpu.DeviceBuffer(max(256, gpu.batch_decompress_workspace_bytes(total, n, h, w)))
        dback = gpu.DeviceBuffer(n * hraw * wraw)
        gpu.batch_decompress_device(dout.ptr, off, n, h, w, dws2.ptr, dback.ptr, wraw, bs, mode, param, 0, gpu.OUT_U8)
        back = dback.download((n, hraw, wraw), np.uint8)
        for p in range(n):
            assert np.array_equal(back[p, :rows, :cols], decompress_reference(wants[p], rows, cols, bs, mode, param)), p
    finally:
        for b in (din, dws, dout, dws2, dback):
            if b is not None:
                b.free()


def test_aligned_shapes_do_not_change(gpu):
    """64 x 64 with block_size 2: the ragged entry and the entry for whole tiles give identical bytes, band and picture."""
    rng = np.random.default_rng(6464)
    bands = [rng.integers(0, 256, (64, 64)).astype(np.uint8) for _ in range(3)]
    for _suffix, mode, param in MODES:
        old = gpu.compress_plane_native(bands[0], 2, mode, param)
        assert old is not None and old == gpu.compress_plane_native(bands[0], 2, mode, param, ragged=True)
        assert old == compress_reference(bands[0], 2, mode, param)
        olds = gpu.compress_image_native(bands, 2, mode, param)
        assert olds == gpu.compress_image_native(bands, 2, mode, param, ragged=True)
        pixels = np.ascontiguousarray(np.dstack(bands))
        assert olds == gpu.compress_image_packed(pixels, 2, mode, param) == gpu.compress_image_packed(pixels, 2, mode, param, ragged=True)
    # a plane that is not whole tiles is still None without `ragged`
    assert gpu.compress_plane_native(np.zeros((37, 53), np.uint8), 2, "qtable", 0.0) is None
