"""The colour conversion's entries and the RGB forms of Jpeg and the command line, as far as no GPU is needed: every
argument check of the two device entries and the four host entries answers before a device is touched; at dct_size 4 on a
small picture compress_rgb / decompress_rgb are the host road and equal the Pillow lines they stand for; the command line
keeps its present line for pictures that are not mode RGB.  CPU only."""
import ctypes

import numpy as np
import pytest

from pipeline import Configuration, Jpeg, QuantizationMethod

INVALID, UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def L():
    import jpegx
    return jpegx.lib()


@pytest.fixture(scope="module")
def buf():
    """Host memory standing in for pointers: an entry that passed its checks would need a device; none here may."""
    b = ctypes.create_string_buffer(4096)
    return ctypes.addressof(b), b


ALLOC_CALLS = []


@pytest.fixture(scope="module")
def alloc():
    import jpegx

    def never(_user, nbytes):
        ALLOC_CALLS.append(nbytes)
        return None
    return jpegx.ALLOC_FN(never)


@pytest.mark.parametrize("name", ["jpegx_rgb_to_ycbcr_u8", "jpegx_ycbcr_to_rgb_u8"])
@pytest.mark.parametrize("on", [False, True])
def test_device_entries_check_their_arguments_first(L, buf, name, on):
    p = buf[0]
    call = getattr(L, name)
    if on:
        # the _on twin makes the device current first: without one it says so; with one it gives the plain entry's answer
        import jpegx
        twin = getattr(L, name + "_on")
        if jpegx.device_count() == 0:
            assert twin(0, None, 3, 1, 1, p, 3, None) != 0
            return

        def call(*a):
            return twin(0, *a)
    assert call(None, 3, 1, 1, p, 3, None) == INVALID and b"null" in L.jpegx_last_error()
    assert call(p, 3, 1, 1, None, 3, None) == INVALID
    assert call(p, 3, 0, 1, p, 3, None) == INVALID
    assert call(p, 3, 1, 0, p, 3, None) == INVALID
    assert call(p, 3, -1, 1, p, 3, None) == INVALID
    assert call(p, 14, 1, 5, p, 15, None) == INVALID and b"pitch" in L.jpegx_last_error()
    assert call(p, 15, 1, 5, p, 14, None) == INVALID and b"pitch" in L.jpegx_last_error()
    assert call(p, 1 << 20, 65536, 32768, p, 1 << 20, None) == INVALID and b"2^31" in L.jpegx_last_error()     # 2^31 pixels


def test_compress_rgb_entries_check_their_arguments_first(L, buf, alloc):
    p = buf[0]
    sizes = (ctypes.c_size_t * 3)()
    tail = (None, 0, 1, alloc, None, sizes)
    q = (3, 0.0)                                        # qtable
    assert L.jpegx_host_compress_image_rgb(None, 16, 16, 48, 1, *q, *tail) == INVALID
    assert L.jpegx_host_compress_image_rgb(p, 16, 16, 48, 1, *q, None, 0, 1, None, None, sizes) == INVALID      # no allocator
    assert L.jpegx_host_compress_image_rgb(p, 16, 16, 48, 1, *q, None, 0, 1, alloc, None, None) == INVALID      # no sizes
    assert L.jpegx_host_compress_image_rgb(p, 16, 16, 48, 1, *q, None, 5, 1, alloc, None, sizes) == INVALID     # prefix length without prefix
    assert L.jpegx_host_compress_image_rgb(p, 0, 16, 48, 1, *q, *tail) == INVALID
    assert L.jpegx_host_compress_image_rgb(p, 16, 0, 48, 1, *q, *tail) == INVALID
    assert L.jpegx_host_compress_image_rgb(p, 16, 16, 47, 1, *q, *tail) == INVALID and b"pitch" in L.jpegx_last_error()
    assert L.jpegx_host_compress_image_rgb(p, 16, 16, 48, 0, *q, *tail) == UNSUPPORTED
    assert L.jpegx_host_compress_image_rgb(p, 16, 16, 48, 256, *q, *tail) == UNSUPPORTED
    assert L.jpegx_host_compress_image_rgb(p, 65536, 16, 48, 1, *q, *tail) == UNSUPPORTED                       # the packed jobs' row limit
    n = (2, 40.0)                                       # divide 40
    assert L.jpegx_host_compress_image_rgb_n(None, 16, 16, 48, 1, 4, *n, *tail) == INVALID
    assert L.jpegx_host_compress_image_rgb_n(p, 16, 16, 48, 1, 4, *n, None, 0, 1, None, None, sizes) == INVALID
    assert L.jpegx_host_compress_image_rgb_n(p, 16, 16, 48, 1, 4, *n, None, 0, 1, alloc, None, None) == INVALID
    assert L.jpegx_host_compress_image_rgb_n(p, 0, 16, 48, 1, 4, *n, *tail) == INVALID
    assert L.jpegx_host_compress_image_rgb_n(p, 16, 16, 47, 1, 4, *n, *tail) == INVALID and b"pitch" in L.jpegx_last_error()
    assert L.jpegx_host_compress_image_rgb_n(p, 16, 16, 48, 0, 4, *n, *tail) == UNSUPPORTED
    assert L.jpegx_host_compress_image_rgb_n(p, 16, 16, 48, 1, 1, *n, *tail) == INVALID                         # dct_size 1
    assert L.jpegx_host_compress_image_rgb_n(p, 16, 16, 48, 1, 33, *n, *tail) == INVALID
    assert L.jpegx_host_compress_image_rgb_n(p, 16, 16, 48, 1, 4, 3, 0.0, *tail) == INVALID                     # qtable at dct_size 4
    assert L.jpegx_host_compress_image_rgb_n(p, 16, 16, 48, 1, 4, 2, 0.0, *tail) == INVALID                     # divide by zero
    assert L.jpegx_host_compress_image_rgb_n(p, 65536, 32768, 3 * 32768, 1, 4, *n, *tail) == INVALID            # 2^31 samples
    assert ALLOC_CALLS == []


def test_decompress_rgb_entries_check_their_arguments_first(L, buf):
    p = buf[0]
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    sizes = (ctypes.c_size_t * 3)(64, 64, 64)
    q = (3, 0.0)
    assert L.jpegx_host_decompress_image_rgb(None, sizes, 16, 16, 1, *q, p, 48, 16, 16) == INVALID
    assert L.jpegx_host_decompress_image_rgb(ptrs, None, 16, 16, 1, *q, p, 48, 16, 16) == INVALID
    assert L.jpegx_host_decompress_image_rgb(ptrs, sizes, 16, 16, 1, *q, None, 48, 16, 16) == INVALID
    assert L.jpegx_host_decompress_image_rgb((ctypes.c_void_p * 3)(p, None, p), sizes, 16, 16, 1, *q, p, 48, 16, 16) == INVALID
    assert L.jpegx_host_decompress_image_rgb(ptrs, sizes, 12, 16, 1, *q, p, 48, 12, 16) == INVALID              # H no multiple of 8
    assert L.jpegx_host_decompress_image_rgb(ptrs, sizes, 16, 16, 0, *q, p, 48, 16, 16) == UNSUPPORTED
    assert L.jpegx_host_decompress_image_rgb(ptrs, sizes, 16, 16, 1, *q, p, 48, 17, 16) == INVALID              # more rows than the plane
    assert L.jpegx_host_decompress_image_rgb(ptrs, sizes, 16, 16, 1, *q, p, 48, 16, 0) == INVALID
    assert L.jpegx_host_decompress_image_rgb(ptrs, sizes, 16, 16, 1, *q, p, 47, 16, 16) == INVALID and b"pitch" in L.jpegx_last_error()
    n = (2, 40.0)
    assert L.jpegx_host_decompress_image_rgb_n(None, sizes, 16, 16, 1, 4, *n, p, 48) == INVALID
    assert L.jpegx_host_decompress_image_rgb_n(ptrs, None, 16, 16, 1, 4, *n, p, 48) == INVALID
    assert L.jpegx_host_decompress_image_rgb_n(ptrs, sizes, 16, 16, 1, 4, *n, None, 48) == INVALID
    assert L.jpegx_host_decompress_image_rgb_n((ctypes.c_void_p * 3)(p, p, None), sizes, 16, 16, 1, 4, *n, p, 48) == INVALID
    assert L.jpegx_host_decompress_image_rgb_n(ptrs, sizes, 0, 16, 1, 4, *n, p, 48) == INVALID
    assert L.jpegx_host_decompress_image_rgb_n(ptrs, sizes, 16, 16, 256, 4, *n, p, 48) == UNSUPPORTED
    assert L.jpegx_host_decompress_image_rgb_n(ptrs, sizes, 16, 16, 1, 40, *n, p, 48) == INVALID
    assert L.jpegx_host_decompress_image_rgb_n(ptrs, sizes, 16, 16, 1, 4, 3, 0.0, p, 48) == INVALID
    assert L.jpegx_host_decompress_image_rgb_n(ptrs, sizes, 16, 16, 1, 4, *n, p, 47) == INVALID and b"pitch" in L.jpegx_last_error()
    assert L.jpegx_host_decompress_image_rgb_n(ptrs, (ctypes.c_size_t * 3)(64, 0, 64), 16, 16, 1, 4, *n, p, 48) == INVALID      # an empty stream


def test_binding_refuses_a_colour_it_does_not_know():
    import jpegx
    px = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(jpegx.JpegxError, match="colour"):
        jpegx.compress_image_packed(px, 1, "qtable", 0.0, ragged=True, colour="lab")
    with pytest.raises(jpegx.JpegxError, match="three bands"):
        jpegx.compress_image_packed_n(np.zeros((16, 16, 2), np.uint8), 1, 4, colour="rgb")
    with pytest.raises(jpegx.JpegxError, match="three bands"):
        jpegx.decompress_image_n([b"\0", b"\0"], 16, 16, 1, 4, colour="rgb")
    with pytest.raises(jpegx.JpegxError, match="interleaved"):
        jpegx.decompress_image_native([b"\0"] * 3, 16, 16, 1, "qtable", 0.0, 16, 16, interleave=False, colour="rgb")


def picture(rows, cols, seed=3):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    smooth = np.stack([(yy * 3 + xx * 2) % 256, (yy * 5 + 40) % 256, (xx * 7 + yy) % 256], axis=-1)
    return Image.fromarray(((smooth + rng.integers(0, 24, smooth.shape)) % 256).astype(np.uint8), mode="RGB")


@pytest.mark.parametrize("quantization", [None, QuantizationMethod("divide", divisor=40)], ids=["none", "divide40"])
def test_rgb_forms_are_the_pillow_lines_on_the_host_road(quantization):
    """dct_size 4 on a 40 x 56 picture: below every device gate, so with or without a GPU this is the host road."""
    im = picture(40, 56)
    cfg = Configuration(width=56, height=40, block_size=2, dct_size=4, quantization=quantization)
    data = Jpeg(cfg).compress_rgb(im)
    assert data == Jpeg(cfg).compress(im.convert("YCbCr"))
    back = Jpeg.decompress_rgb(data)
    want = Jpeg.decompress(data).convert("RGB")
    assert back.mode == "RGB" and back.size == want.size
    assert np.array_equal(np.asarray(back), np.asarray(want))


def test_compress_rgb_converts_whatever_mode_it_is_handed():
    """A picture that is not mode RGB is not a case for the device road: it is converted by Pillow, like the command line does."""
    im = picture(40, 56).convert("L")
    cfg = Configuration(width=56, height=40, block_size=1, dct_size=4)
    assert Jpeg(cfg).compress_rgb(im) == Jpeg(cfg).compress(im.convert("YCbCr"))


@pytest.mark.parametrize("mode", ["L", "RGBA", "P"])
def test_cli_keeps_its_line_for_pictures_that_are_not_rgb(tmp_path, mode):
    from PIL import Image
    import compress
    src, out = tmp_path / ("in_%s.png" % mode), tmp_path / "out.bin"
    im = picture(40, 56)
    if mode == "RGBA":
        im = im.convert("RGBA")
        im.putalpha(Image.fromarray(np.asarray(im)[:, :, 0]))
    else:
        im = im.convert(mode)
    im.save(src)
    assert Image.open(src).mode == mode
    q = QuantizationMethod("divide", divisor=40)
    compress.compress(str(src), str(out), block_size=2, dct_size=4, transform="DCT", quantization=q)
    cfg = Configuration(width=56, height=40, block_size=2, dct_size=4, quantization=q)
    assert out.read_bytes() == Jpeg(cfg).compress(Image.open(src).convert("YCbCr"))


def test_cli_round_trip_of_an_rgb_file_on_the_host_road(tmp_path):
    from PIL import Image
    import compress
    import decompress
    src, out, back = tmp_path / "in.png", tmp_path / "out.bin", tmp_path / "back.png"
    picture(40, 56).save(src)
    q = QuantizationMethod("divide", divisor=40)
    compress.compress(str(src), str(out), block_size=1, dct_size=4, transform="DCT", quantization=q)
    cfg = Configuration(width=56, height=40, block_size=1, dct_size=4, quantization=q)
    assert out.read_bytes() == Jpeg(cfg).compress(Image.open(src).convert("YCbCr"))
    decompress.decompress(str(out), str(back))
    got = Image.open(back)
    assert got.mode == "RGB"
    assert np.array_equal(np.asarray(got), np.asarray(Jpeg.decompress(out.read_bytes()).convert("RGB")))
