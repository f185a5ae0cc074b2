"""GPU: every road a user calls -- compress_band, decompress_band(_u8), Jpeg.compress / decompress and the jpegx
plane and picture entries behind them -- against the independent end-to-end oracle (tests/codec_oracle.py), over a
deterministic matrix of block sizes, band shapes, quantisers, contents and band dtypes.  Every comparison is exact.

The decompressing roads are fed the oracle's byte streams, so the decoders are also checked on streams the product
did not write.  Where the oracle raises (an amplitude beyond 15 bits) every road raises the reference's type:
util.BadRleCodeError from the pipeline API, jpegx.JpegxError from jpegx.*; none returns bytes."""
import ctypes
import mmap

import numpy as np
import pytest

import file_format
import pipeline
import util
from codec_oracle import BadRleCodeError, blocks_of, compress_reference, decompress_reference, edge_pad
from pipeline import CompressedData, Configuration, QuantizationMethod, compress_band, decompress_band, decompress_band_u8

pytestmark = pytest.mark.gpu

# (mode, parameter): divide 0.5 / 0.49 stand either side of the uint8 kernels' gate (jpegx.u8_path_ok), divide 0.02
# drives amplitudes beyond 15 bits
QUANTISERS = [("qtable", 0.0), ("none", 0.0), ("divide", 40.0), ("divide", 7.0), ("divide", 3.3), ("divide", 0.5),
              ("divide", 0.49), ("divide", 0.02), ("discard", 1.0), ("discard", 2.0), ("discard", 8.0)]
CONTENTS = ["noise", "smooth", "const0", "const255", "checker", "halfties"]
DTYPES = ["uint8", "int32", "int64", "uint16", "int64wide", "float64frac"]
BLOCK_SIZES = [1, 2, 3, 4, 5, 7, 8, 16]
KINDS = ["exact", "ragged", "row", "col", "medium"]


def shape_of(kind, bs):
    if kind == "exact":
        return 16 * bs, 32 * bs
    if kind == "ragged":        # rows: Padding (bs > 1) and DCTPadding; columns: the same from below
        return 16 * bs + 1, 31 * bs - 1
    if kind == "row":
        return 1, 24 * bs + 1
    if kind == "col":
        return 8 * bs + 3, 1
    if kind == "medium":        # thousands of blocks: many 64-block waves, many 4096-byte decoder chunks
        return (256 * bs, 512 * bs) if bs <= 4 else (256 * bs, 256 * bs)
    if kind == "w24":           # block_size 1, width not a multiple of 16: the uint8 road refuses it
        return 16, 24
    raise ValueError(kind)


def make_content(kind, h, w, bs, rng):
    """Integer samples 0..255, (h, w)."""
    i, j = np.indices((h, w))
    if kind == "noise":
        return rng.integers(0, 256, (h, w))
    if kind == "smooth":
        return np.rint(127.5 + 120 * np.sin(i / (5.0 * bs) + 0.3) * np.cos(j / (7.0 * bs))).astype(np.int64)
    if kind == "const0":
        return np.zeros((h, w), np.int64)
    if kind == "const255":
        return np.full((h, w), 255, np.int64)
    if kind == "checker":       # 0/255 checkerboard of bs x bs tiles: the pooled samples alternate, the largest AC
        return 255 * ((i // bs + j // bs) & 1)
    if kind == "halfties":
        a = rng.integers(0, 255, (h, w))
        # bs even: every whole tile sums to bs^2 / 2 (mod bs^2), its mean ends in exactly .5; bs 1: every whole 8x8 block
        # sums to 8 (mod 16), the qtable DC lands on an exact .5; odd bs > 1 has no such ties (plain noise)
        t, m = (bs, bs * bs // 2) if bs % 2 == 0 else (8, 8) if bs == 1 else (0, 0)
        if t and h >= t and w >= t:
            th, tw = h // t, w // t
            sums = a[:th * t, :tw * t].reshape(th, t, tw, t).sum(axis=(1, 3))
            r = (m - sums) % (2 * m)
            ii, jj = np.indices((th * t, tw * t))
            a[:th * t, :tw * t] += (ii % t) * t + jj % t < r[ii // t, jj // t]
        return a
    raise ValueError(kind)


def with_dtype(a, dtype):
    if dtype == "int64wide":    # samples outside 0..255
        return a.astype(np.int64) * 2 - 100
    if dtype == "float64frac":  # fractions that are not fp32 numbers
        return a.astype(np.float64) * 0.75 + 0.1
    return a.astype(dtype)


def method(mode, param):
    if mode == "divide":
        return QuantizationMethod("divide", divisor=param)
    if mode == "discard":
        return QuantizationMethod("discard", keep=int(param))
    return QuantizationMethod(mode)


def eight_bit(band):
    return band.dtype.kind in "ui" and band.min() >= 0 and band.max() <= 255


def native_takes(band, bs, mode, param):
    """Whether jpegx_host_compress_begin / _image take this (already padded) plane: an 8-bit band in a uint8 /
    int32 / int64 array of whole 8 * bs tiles; at block sizes 1, 2, 4 also rows of a multiple of 16 bytes and a
    quantiser the uint8 kernels accept."""
    hh, ww = band.shape
    if band.dtype not in (np.uint8, np.int32, np.int64) or hh % (8 * bs) or ww % (8 * bs) or not eight_bit(band):
        return False
    return not (bs in (1, 2, 4) and (ww % 16 or (mode == "divide" and abs(param) < 0.5)))


def reference(band, bs, mode, param):
    try:
        return compress_reference(band, bs, mode, param)
    except BadRleCodeError:
        return None


def check_band_roads(gpu, band, bs, mode, param, tag):
    """compress_band / decompress_band / decompress_band_u8 and the plane entries of jpegx against the oracle."""
    h, w = band.shape
    cfg = Configuration(width=w, height=h, block_size=bs, quantization=method(mode, param))
    want = reference(band, bs, mode, param)
    if want is None:
        with pytest.raises(util.BadRleCodeError):
            compress_band(band, cfg)
    else:
        got = compress_band(band, cfg)
        assert isinstance(got, bytes) and got == want, tag
    padded = np.ascontiguousarray(edge_pad(band, bs)) if bs > 1 else band
    takes = native_takes(padded, bs, mode, param)
    if want is None and takes:
        with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
            gpu.compress_plane_native(padded, bs, mode, param)
    elif want is None:
        assert gpu.compress_plane_native(padded, bs, mode, param) is None, tag
    else:
        assert gpu.compress_plane_native(padded, bs, mode, param) == (want if takes else None), tag
    if takes or (bs in (1, 2, 4) and eight_bit(padded) and not (padded.shape[0] % (8 * bs) or padded.shape[1] % (8 * bs))):
        if want is None:
            with pytest.raises(gpu.JpegxError):
                gpu.compress_plane(padded, bs, mode, param)
        else:
            assert gpu.compress_plane(padded, bs, mode, param) == want, tag
    if want is None:
        return None
    ref = decompress_reference(want, h, w, bs, mode, param)
    got = decompress_band(want, cfg)
    assert got.dtype == np.int64 and got.shape == (h, w) and np.array_equal(got, ref), tag
    got = decompress_band_u8(want, cfg)
    assert got.dtype == np.uint8 and np.array_equal(got, ref), tag
    hb, wb = blocks_of(h, w, bs)
    got = gpu.decompress_plane_i64(want, hb * 8, wb * 8, bs, mode, param, h, w)
    assert got.shape == (h, w) and np.array_equal(got, ref), tag
    full = gpu.decompress_plane(want, hb * 8, wb * 8, bs, mode, param)
    assert full.shape == (hb * 8 * bs, wb * 8 * bs) and np.array_equal(full[:h, :w], ref), tag
    return ref


def check_picture_roads(gpu, bands, bs, mode, param, tag):
    """compress_image_native / _packed, Jpeg.compress, decompress_image_native and Jpeg.decompress on a picture of
    three different bands."""
    from PIL import Image
    h, w = bands[0].shape
    cfg = Configuration(width=w, height=h, block_size=bs, quantization=method(mode, param))
    wants = [reference(b, bs, mode, param) for b in bands]
    fails = any(x is None for x in wants)
    padded = [np.ascontiguousarray(edge_pad(b, bs)) if bs > 1 else b for b in bands]
    takes = native_takes(padded[0], bs, mode, param)
    if fails and takes:
        with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
            gpu.compress_image_native(padded, bs, mode, param)
    elif not takes:
        assert gpu.compress_image_native(padded, bs, mode, param) is None, tag
    else:
        assert gpu.compress_image_native(padded, bs, mode, param) == wants, tag
    if not all(eight_bit(b) for b in bands):
        return
    pixels = np.ascontiguousarray(np.dstack(bands).astype(np.uint8))
    if native_takes(pixels[..., 0], bs, mode, param) and h <= 65535:
        if fails:
            with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
                gpu.compress_image_packed(pixels, bs, mode, param)
        else:
            assert gpu.compress_image_packed(pixels, bs, mode, param) == wants, tag
    else:
        assert gpu.compress_image_packed(pixels, bs, mode, param) is None, tag
    image = Image.frombytes("YCbCr", (w, h), pixels.tobytes())
    if fails:
        with pytest.raises(util.BadRleCodeError):
            pipeline.Jpeg(cfg).compress(image)
        return
    container = file_format.generate_data(cfg, CompressedData(*wants))
    assert pipeline.Jpeg(cfg).compress(image) == container, tag
    refs = np.stack([decompress_reference(x, h, w, bs, mode, param) for x in wants]).astype(np.uint8)
    hb, wb = blocks_of(h, w, bs)
    got = gpu.decompress_image_native(wants, hb * 8, wb * 8, bs, mode, param, h, w, interleave=True)
    assert np.array_equal(got, np.moveaxis(refs, 0, 2)), tag
    got = gpu.decompress_image_native(wants, hb * 8, wb * 8, bs, mode, param, h, w, interleave=False)
    assert np.array_equal(got, refs), tag
    back = pipeline.Jpeg.decompress(container)
    assert back.mode == "YCbCr" and np.array_equal(np.asarray(back), np.moveaxis(refs, 0, 2)), tag


def matrix_pairs():
    pairs = [(bs, kind) for bs in BLOCK_SIZES for kind in KINDS]
    return pairs + [(1, "w24")]


@pytest.mark.parametrize("bs,kind", matrix_pairs(), ids=lambda v: str(v))
def test_every_road_meets_the_oracle(gpu, bs, kind):
    """One (block size, shape kind) pair against every quantiser; content and dtype rotate from quantiser to
    quantiser (the medium band keeps to the dtypes the native roads take: the others run step by step on the host)."""
    h, w = shape_of(kind, bs)
    bsi, ki = BLOCK_SIZES.index(bs), (KINDS + ["w24"]).index(kind)
    for qi, (mode, param) in enumerate(QUANTISERS):
        content = CONTENTS[(qi + bsi + ki) % len(CONTENTS)]
        dtype = DTYPES[(5 * qi + 3 * ki + bsi) % len(DTYPES)]
        if kind == "medium":
            dtype = DTYPES[(5 * qi + bsi) % 4]
        rng = np.random.default_rng(100000 * bs + 1000 * ki + qi)
        base = make_content(content, h, w, bs, rng)
        planes = [with_dtype(a, dtype) for a in (base, np.ascontiguousarray(base[::-1]), 255 - base)]
        tag = "bs %d %s %dx%d %s %g %s %s" % (bs, kind, h, w, mode, param, content, dtype)
        check_band_roads(gpu, planes[0], bs, mode, param, tag)
        check_picture_roads(gpu, planes, bs, mode, param, tag)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("bs", [1, 2, 3])
def test_small_bands_full_cross_product(gpu, bs, content, dtype):
    """Every content with every dtype at block sizes 1-3, on a ragged or an exact small band; the quantiser rotates."""
    ci, di = CONTENTS.index(content), DTYPES.index(dtype)
    mode, param = QUANTISERS[(6 * ci + di + bs) % len(QUANTISERS)]
    h, w = (8 * bs + 3, 16 * bs - 1) if (ci + di) % 2 else (8 * bs, 16 * bs)
    rng = np.random.default_rng(7000 + 100 * bs + 10 * ci + di)
    band = with_dtype(make_content(content, h, w, bs, rng), dtype)
    check_band_roads(gpu, band, bs, mode, param, "bs %d %dx%d %s %g %s %s" % (bs, h, w, mode, param, content, dtype))


def test_block_size_255_one_block(gpu):
    """2040 x 2040 samples pool to a single 8 x 8 block."""
    for qi, (mode, param) in enumerate(QUANTISERS):
        content = CONTENTS[qi % len(CONTENTS)]
        rng = np.random.default_rng(255 + qi)
        band = with_dtype(make_content(content, 2040, 2040, 255, rng), ["uint8", "int32", "int64"][qi % 3])
        tag = "bs 255 %s %g %s" % (mode, param, content)
        check_band_roads(gpu, band, 255, mode, param, tag)
        if qi < 3:
            check_picture_roads(gpu, [band, np.ascontiguousarray(band[::-1]), np.ascontiguousarray(band[:, ::-1])],
                                255, mode, param, tag)


def test_packed_picture_row_limit(gpu):
    """compress_image_packed takes at most 65535 rows; a taller picture goes band by band, same bytes."""
    rng = np.random.default_rng(65535)
    for h in (65528, 65536):
        bands = [make_content("smooth", h, 16, 1, rng).astype(np.uint8) for _ in range(3)]
        bands[1] = np.ascontiguousarray(bands[1][::-1])
        bands[2] = np.ascontiguousarray(255 - bands[2])
        wants = [compress_reference(b, 1, "qtable") for b in bands]
        got = gpu.compress_image_packed(np.ascontiguousarray(np.dstack(bands)), 1, "qtable", 0.0)
        assert got == (wants if h <= 65535 else None), h
        assert gpu.compress_image_native(bands, 1, "qtable", 0.0) == wants, h
        if h > 65535:
            continue                                        # the container's header holds 16-bit sizes
        from PIL import Image
        cfg = Configuration(width=16, height=h, block_size=1, quantization=QuantizationMethod("qtable"))
        image = Image.frombytes("YCbCr", (16, h), np.dstack(bands).tobytes())
        assert pipeline.Jpeg(cfg).compress(image) == file_format.generate_data(cfg, CompressedData(*wants)), h


@pytest.mark.parametrize("interleave,nbands,pitch", [(0, 1, 8192), (1, 3, 16384)])
def test_decompress_image_into_a_strided_destination(gpu, interleave, nbands, pitch):
    """jpegx_host_decompress_image with rows `pitch` bytes apart writes the samples and nothing else: the bytes between
    the rows (and behind the last one) keep what the caller put there.  The destination is fresh anonymous memory
    whose sample pages are not resident yet (only the gap pages were written), so the library's page-touching
    helper takes it for a fresh result array."""
    rows, cols = 1024, 4096
    rng = np.random.default_rng(4096)
    bands = [make_content("smooth" if k % 2 == 0 else "noise", rows, cols, 1, rng).astype(np.uint8) for k in range(nbands)]
    blobs = [compress_reference(b, 1, "qtable") for b in bands]
    refs = [decompress_reference(x, rows, cols, 1, "qtable").astype(np.uint8) for x in blobs]
    row_bytes = cols * nbands if interleave else cols
    nrows = rows if interleave else nbands * rows
    span = nrows * pitch
    assert pitch > row_bytes and span >= (8 << 20)
    mm = mmap.mmap(-1, span)
    canvas = np.frombuffer(mm, dtype=np.uint8).reshape(nrows, pitch)
    canvas[:, row_bytes:] = 0xA5                       # the gap pages only: the sample pages stay cold
    L = gpu.lib()
    ptrs = (ctypes.c_void_p * nbands)(*[ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p).value for x in blobs])
    sizes = (ctypes.c_size_t * nbands)(*[len(x) for x in blobs])
    gpu.check(L.jpegx_host_decompress_image(ptrs, sizes, nbands, rows, cols, 1, gpu.mode_of("qtable"), 0.0,
                                            canvas.ctypes.data, pitch, rows, cols, interleave), "jpegx_host_decompress_image")
    if interleave:
        assert np.array_equal(canvas[:, :row_bytes].reshape(rows, cols, nbands), np.dstack(refs))
    else:
        assert np.array_equal(canvas[:, :row_bytes], np.concatenate(refs))
    assert np.all(canvas[:, row_bytes:] == 0xA5), "%d gap bytes overwritten" % int(np.count_nonzero(canvas[:, row_bytes:] != 0xA5))
    del canvas
    mm.close()


def damage_padding(blob, zz):
    """The stream with a 1 in the last padding bit of every block whose code string does not end on a byte boundary:
    the reference's sequential parser skips padding unread (rle_byte_stream.py BitDecoder.skip_padding), the device
    decoder refuses such streams and the roads fall back to the host parser."""
    import oracle
    out, at, hit = bytearray(blob), 0, 0
    for block in np.asarray(zz).reshape(-1, 64):
        bits = sum(8 + (t[1] if len(t) == 3 and not (t[0] == 15 and t[1] == 0) else 0) for t in oracle.rle_block_tuples(block))
        at += (bits + 7) // 8
        if bits % 8:
            out[at - 1] |= 1
            hit += 1
    assert at == len(blob) and hit
    return bytes(out)


@pytest.mark.parametrize("bs,h,w,mode,param", [(1, 40, 56, "qtable", 0.0), (2, 37, 53, "divide", 7.0), (3, 44, 70, "none", 0.0),
                                                 (5, 23, 41, "discard", 2.0)])
def test_streams_with_damaged_padding_take_the_host_parser(gpu, bs, h, w, mode, param):
    """decompress_band, decompress_band_u8 and Jpeg.decompress on streams the device decoder refuses: the host parser
    and the fused inverse (pipeline._back_end_fused) give the reference's band."""
    import codec_oracle
    rng = np.random.default_rng(bs * 1000 + h)
    bands = [make_content(c, h, w, bs, rng).astype(np.uint8) for c in ("noise", "smooth", "halfties")]
    blobs, refs = [], []
    for b in bands:
        blob = damage_padding(compress_reference(b, bs, mode, param), codec_oracle.forward_zigzag(b, bs, mode, param))
        ref = decompress_reference(blob, h, w, bs, mode, param)
        assert np.array_equal(ref, decompress_reference(compress_reference(b, bs, mode, param), h, w, bs, mode, param))
        blobs.append(blob)
        refs.append(ref)
    cfg = Configuration(width=w, height=h, block_size=bs, quantization=method(mode, param))
    for blob, ref in zip(blobs, refs):
        got = decompress_band(blob, cfg)
        assert got.dtype == np.int64 and np.array_equal(got, ref)
        assert np.array_equal(decompress_band_u8(blob, cfg), ref)
    back = pipeline.Jpeg.decompress(file_format.generate_data(cfg, CompressedData(*blobs)))
    assert np.array_equal(np.asarray(back), np.dstack(refs).astype(np.uint8))
