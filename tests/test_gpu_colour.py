"""GPU: Pillow's RGB <-> YCbCr conversion on the device (csrc/jpegx_colour.hip) and the picture jobs that run it inside.

The two kernels against Pillow on every colour and on the shapes, pitches and base offsets at which a lane changes between
its 16-byte and its byte path; Jpeg.compress_rgb / Jpeg.decompress_rgb and the command line against the Pillow lines they
stand for, byte for byte, with a count of the native _rgb entries' calls (a test that passes through the fallback proves
nothing); the native entries into a wider canvas; a refused stream.

The device-pointer helper below follows tests/dctn_dev.py (its fill value, its check that the slack was left alone); that
module's own helpers each call one dct_size-N entry and cannot be pointed at another."""
import ctypes
import functools

import numpy as np
import pytest

import colour_model
from dctn_dev import SLACK_I
from pipeline import Configuration, Jpeg, QuantizationMethod

pytestmark = pytest.mark.gpu

RGB_ENTRIES = ("jpegx_host_compress_image_rgb", "jpegx_host_decompress_image_rgb", "jpegx_host_compress_image_rgb_n",
               "jpegx_host_decompress_image_rgb_n")
CANARY = 64


class NativeCalls:
    """Counts the calls of the native _rgb entries where the binding makes them: on the loaded library object."""

    def __init__(self, gpu, monkeypatch):
        self.counts = {}
        L = gpu.lib()
        for name in RGB_ENTRIES:
            monkeypatch.setattr(L, name, self._counting(name, getattr(L, name)))

    def _counting(self, name, real):
        def entry(*args):
            self.counts[name] = self.counts.get(name, 0) + 1
            return real(*args)
        return entry

    def take(self):
        counts, self.counts = self.counts, {}
        return counts


@pytest.fixture
def native(gpu, monkeypatch):
    return NativeCalls(gpu, monkeypatch)


def pillow(pixels, src, dst):
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(pixels), mode=src).convert(dst))


# ---- the kernels ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def every():
    a = colour_model.all_colours()
    a.setflags(write=False)
    return a


def test_every_colour_forward(gpu, every):
    got = gpu.rgb_to_ycbcr(every)
    assert got.dtype == np.uint8 and got.shape == every.shape
    assert int(np.count_nonzero(got != pillow(every, "RGB", "YCbCr"))) == 0


def test_every_colour_inverse(gpu, every):
    got = gpu.ycbcr_to_rgb(every)
    assert got.dtype == np.uint8 and got.shape == every.shape
    assert int(np.count_nonzero(got != pillow(every, "YCbCr", "RGB"))) == 0


class Arena:
    """Two device spans reused by every edge case (a hipMalloc per case would be most of the test's time)."""

    def __init__(self, gpu, nbytes):
        self.gpu, self.nbytes = gpu, nbytes
        self.a, self.b = gpu.DeviceBuffer(nbytes), gpu.DeviceBuffer(nbytes)

    def free(self):
        self.a.free()
        self.b.free()


@pytest.fixture(scope="module")
def arena(gpu):
    ar = Arena(gpu, 2 * CANARY + 16 + 3 * (3 * 257 + 13))
    yield ar
    ar.free()


def convert_dev(arena, name, pixels, gap, offset, in_place, on=False):
    """One device entry on pixels stored `offset` bytes into a span, rows 3 * cols + gap bytes apart, CANARY bytes of
    SLACK_I on either side and in every gap: the converted pixels, after asserting that nothing but the pixels' own bytes
    changed on the output side and nothing at all on the input side when it is another span."""
    gpu = arena.gpu
    rows, cols, _ = pixels.shape
    row, pitch = 3 * cols, 3 * cols + gap
    span = (rows - 1) * pitch + row
    total = CANARY + offset + span + CANARY
    assert total <= arena.nbytes
    stored = np.full(total, SLACK_I, np.uint8)
    at = CANARY + offset
    inside = np.zeros(total, bool)
    for y in range(rows):
        stored[at + y * pitch: at + y * pitch + row] = pixels[y].ravel()
        inside[at + y * pitch: at + y * pitch + row] = True
    arena.a.upload(stored)
    dst = arena.a
    if not in_place:
        dst = arena.b
        dst.upload(np.full(total, SLACK_I, np.uint8))
    L = gpu.lib()
    args = (arena.a.ptr + at, pitch, rows, cols, dst.ptr + at, pitch, None)
    gpu.check(getattr(L, name + "_on")(0, *args) if on else getattr(L, name)(*args), name)
    gpu.check(L.jpegx_stream_synchronize(None), "sync")
    res = dst.download((total,), np.uint8)
    assert np.all(res[~inside] == SLACK_I), "bytes outside the pixels were written"
    if not in_place:
        assert np.array_equal(arena.a.download((total,), np.uint8), stored), "the input was written"
    return np.stack([res[at + y * pitch: at + y * pitch + row].reshape(cols, 3) for y in range(rows)])


@pytest.mark.parametrize("name, src, dst", [("jpegx_rgb_to_ycbcr_u8", "RGB", "YCbCr"), ("jpegx_ycbcr_to_rgb_u8", "YCbCr", "RGB")])
def test_edges_of_the_lanes_paths(gpu, arena, name, src, dst):
    rng = np.random.default_rng(11)
    for rows in (1, 3):
        for cols in (1, 2, 5, 15, 16, 17, 31, 33, 257):
            pixels = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
            want = pillow(pixels, src, dst)
            for gap in (0, 1, 13):
                for offset in (0, 1, 3):
                    for in_place in (True, False):
                        got = convert_dev(arena, name, pixels, gap, offset, in_place)
                        assert np.array_equal(got, want), (name, rows, cols, gap, offset, in_place)
    # the explicit-device twin, once per path
    for cols, gap, offset in ((33, 0, 0), (17, 13, 3)):
        pixels = rng.integers(0, 256, (3, cols, 3)).astype(np.uint8)
        assert np.array_equal(convert_dev(arena, name, pixels, gap, offset, True, on=True), pillow(pixels, src, dst))


def test_more_than_one_workgroup_and_more_than_one_chunk_per_lane(gpu):
    """1024 workgroups of 256 lanes walk the chunks: 700 x 6001 pixels are 262 544 chunks of 16, just past one per lane, the
    last chunk a partial one."""
    rng = np.random.default_rng(12)
    pixels = rng.integers(0, 256, (700, 6001, 3)).astype(np.uint8)
    assert np.array_equal(gpu.rgb_to_ycbcr(pixels), pillow(pixels, "RGB", "YCbCr"))
    assert np.array_equal(gpu.ycbcr_to_rgb(pixels), pillow(pixels, "YCbCr", "RGB"))


# ---- the jobs -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def picture(rows, cols):
    """A smooth RGB picture with some noise on it, read-only; the PIL image is made from it per use."""
    rng = np.random.default_rng(rows * 4099 + cols)
    yy, xx = np.mgrid[0:rows, 0:cols]
    smooth = np.stack([(yy * 3 + xx * 2) // 4 % 256, (yy // 2 + 40 + xx // 8) % 256, (xx * 5 // 8 + yy // 3) % 256], axis=-1)
    a = ((smooth + rng.integers(0, 24, smooth.shape)) % 256).astype(np.uint8)
    a.setflags(write=False)
    return a


def image_of(pixels, mode="RGB"):
    from PIL import Image
    return Image.fromarray(pixels, mode=mode)


def config_of(rows, cols, bs, n, quantization):
    return Configuration(width=cols, height=rows, block_size=bs, dct_size=n, quantization=quantization)


def quantiser(name):
    return {"qtable": lambda: QuantizationMethod("qtable"), "none": lambda: None, "divide40": lambda: QuantizationMethod("divide", divisor=40),
            "divide1000": lambda: QuantizationMethod("divide", divisor=1000)}[name]()


def both_ways(native, rows, cols, bs, n, qname, forward_entry, back_entry):
    """The three assertions of a job case: compress_rgb's bytes, decompress_rgb's pixels, the native entries' calls."""
    pixels = picture(rows, cols)
    cfg = config_of(rows, cols, bs, n, quantiser(qname))
    want = Jpeg(cfg).compress(image_of(pixels).convert("YCbCr"))
    assert native.take() == {}, "the Pillow road called an _rgb entry"
    data = Jpeg(cfg).compress_rgb(image_of(pixels))
    assert native.take() == ({forward_entry: 1} if forward_entry else {})
    assert isinstance(data, bytes) and data == want
    want_back = Jpeg.decompress(data).convert("RGB")
    assert native.take() == {}
    back = Jpeg.decompress_rgb(data)
    assert native.take() == ({back_entry: 1} if back_entry else {})
    assert back.mode == "RGB" and back.size == want_back.size == (cols, rows)
    assert np.asarray(back).tobytes() == np.asarray(want_back).tobytes()
    return data


@pytest.mark.parametrize("rows, cols", [(64, 64), (72, 104)])
@pytest.mark.parametrize("bs, qname", [(1, "qtable"), (2, "qtable"), (4, "none")])
def test_jobs_at_8x8(gpu, native, rows, cols, bs, qname):
    both_ways(native, rows, cols, bs, 8, qname, "jpegx_host_compress_image_rgb", "jpegx_host_decompress_image_rgb")


@pytest.mark.parametrize("rows, cols, bs, n, qname", [(192, 192, 1, 4, "divide40"), (192, 192, 1, 16, "divide40"),
                                                      (1000, 1000, 5, 24, "divide1000"), (999, 998, 5, 24, "divide1000")])
def test_jobs_at_other_dct_sizes(gpu, native, rows, cols, bs, n, qname):
    both_ways(native, rows, cols, bs, n, qname, "jpegx_host_compress_image_rgb_n", "jpegx_host_decompress_image_rgb_n")


def test_a_picture_below_the_gates_takes_the_pillow_road(gpu, native):
    both_ways(native, 64, 64, 1, 4, "divide40", None, None)


def test_a_picture_that_is_not_rgb_takes_the_pillow_road(gpu, native):
    pixels = picture(72, 104)
    cfg = config_of(72, 104, 2, 8, quantiser("qtable"))
    for im in (image_of(pixels).convert("L"), image_of(pixels).convert("RGBA"), image_of(pixels, "YCbCr")):
        assert Jpeg(cfg).compress_rgb(im) == Jpeg(cfg).compress(im.convert("YCbCr"))
        assert native.take() == {}


# ---- the native entries ---------------------------------------------------------------------------------------------------
def bands_of(container):
    import file_format
    cfg, data = file_format.read_data(container)
    return cfg, [data.y, data.cb, data.cr]


def blob_args(blobs):
    bufs = [np.frombuffer(b, np.uint8) for b in blobs]
    return bufs, (ctypes.c_void_p * 3)(*[b.ctypes.data for b in bufs]), (ctypes.c_size_t * 3)(*[b.size for b in bufs])


def native_decompress_rgb(gpu, blobs, rows, cols, bs, n, mode, param, out, at, pitch, on=False):
    """jpegx_host_decompress_image_rgb (n == 8) or _rgb_n into `out` (a flat uint8 array) from byte `at`, rows pitch apart."""
    import pipeline
    _keep, ptrs, sizes = blob_args(blobs)
    L = gpu.lib()
    dst = out.ctypes.data + at
    if n == 8:
        hb, wb = pipeline._blocks(config_of(rows, cols, bs, 8, None))
        args = (ptrs, sizes, hb * 8, wb * 8, bs, gpu.mode_of(mode), float(param), dst, pitch, rows, cols)
        return L.jpegx_host_decompress_image_rgb_on(0, *args) if on else L.jpegx_host_decompress_image_rgb(*args)
    args = (ptrs, sizes, rows, cols, bs, n, gpu.mode_of(mode), float(param), dst, pitch)
    return L.jpegx_host_decompress_image_rgb_n_on(0, *args) if on else L.jpegx_host_decompress_image_rgb_n(*args)


STRIDED = [(72, 104, 2, 8, "qtable", "qtable", 0.0), (192, 192, 1, 4, "divide40", "divide", 40.0)]


@pytest.mark.parametrize("rows, cols, bs, n, qname, mode, param", STRIDED)
def test_strided_destination(gpu, rows, cols, bs, n, qname, mode, param):
    """Into the rows of a wider, pre-filled canvas: the picture is right and every canvas byte outside it is unchanged."""
    pixels = picture(rows, cols)
    cfg = config_of(rows, cols, bs, n, quantiser(qname))
    data = Jpeg(cfg).compress(image_of(pixels).convert("YCbCr"))
    want = np.asarray(Jpeg.decompress(data).convert("RGB"))
    _, blobs = bands_of(data)
    for on in (False, True):
        pitch, top, left = 3 * cols + 37, 5, 11                                # the picture sits 5 rows down, 11 bytes in
        canvas = np.full((rows + 9) * pitch, 0xA5, np.uint8)
        at = top * pitch + left
        assert native_decompress_rgb(gpu, blobs, rows, cols, bs, n, mode, param, canvas, at, pitch, on) == 0, gpu.lib().jpegx_last_error()
        inside = np.zeros(canvas.size, bool)
        for y in range(rows):
            inside[at + y * pitch: at + y * pitch + 3 * cols] = True
        assert np.all(canvas[~inside] == 0xA5), "canvas bytes outside the picture were written"
        assert np.array_equal(canvas[inside].reshape(rows, cols, 3), want)


def test_strided_source(gpu):
    """The compress entries from pixels stored wider than their rows, and through their twins: the Pillow road's bytes."""
    import file_format
    for rows, cols, bs, n, qname, mode, param in STRIDED:
        pixels = picture(rows, cols)
        cfg = config_of(rows, cols, bs, n, quantiser(qname))
        want = Jpeg(cfg).compress(image_of(pixels).convert("YCbCr"))
        prefix = file_format.create_header(cfg)
        for gap, on in ((0, False), (7, False), (13, True)):
            pitch = 3 * cols + gap
            stored = np.full((rows, pitch), 0x5A, np.uint8)
            stored[:, :3 * cols] = pixels.reshape(rows, 3 * cols)
            box = []

            def alloc(_user, nbytes):
                box.append(ctypes.create_string_buffer(max(nbytes, 1)))
                box.append(nbytes)
                return ctypes.addressof(box[0])
            cb = gpu.ALLOC_FN(alloc)
            sizes = (ctypes.c_size_t * 3)()
            head = (stored.ctypes.data, rows, cols, pitch, bs) + ((n,) if n != 8 else ())
            args = head + (gpu.mode_of(mode), float(param), prefix, len(prefix), 1, cb, None, sizes)
            name = "jpegx_host_compress_image_rgb" + ("_n" if n != 8 else "") + ("_on" if on else "")
            rc = getattr(gpu.lib(), name)(*(((0,) if on else ()) + args))
            assert rc == 0, gpu.lib().jpegx_last_error()
            assert box[0].raw[:box[1]] == want, (name, gap)
            assert np.all(stored[:, 3 * cols:] == 0x5A)


def outcome(fn):
    try:
        result = fn()
    except Exception as exc:
        return (type(exc), str(exc))
    return ("picture", np.asarray(result).tobytes())


@pytest.mark.parametrize("rows, cols, bs, n, qname, mode, param", STRIDED)
def test_refused_stream(gpu, native, rows, cols, bs, n, qname, mode, param):
    """One band's stream loses its last byte: decompress_rgb ends as decompress does; at the C entry of the dct_size-N job,
    whose parent promises it, the destination is left as it was (the 8 x 8 parent copies down before its verdicts and
    promises nothing of the kind: there only the refusal is asserted)."""
    import file_format
    import pipeline
    pixels = picture(rows, cols)
    cfg = config_of(rows, cols, bs, n, quantiser(qname))
    data = Jpeg(cfg).compress(image_of(pixels).convert("YCbCr"))
    _, good = bands_of(data)
    blobs = [good[0], good[1][:-1], good[2]]
    container = file_format.generate_data(cfg, pipeline.CompressedData(*blobs))
    native.take()
    after = outcome(lambda: Jpeg.decompress_rgb(container))
    assert sum(native.take().values()) == 1, "the job was not asked"
    assert after == outcome(lambda: Jpeg.decompress(container).convert("RGB"))      # an exception, or what the host parser makes of it
    out =np.full(rows * cols * 3, 0xA5, np.uint8)
    assert native_decompress_rgb(gpu, blobs, rows, cols, bs, n, mode, param, out, 0, 3 * cols) == -1
    if n != 8:
        assert np.all(out == 0xA5), "a refused band wrote the caller's pixels"
    # the context is given back: the next good job succeeds
    assert native_decompress_rgb(gpu, good, rows, cols, bs, n, mode, param, out, 0, 3 * cols) == 0
    assert np.array_equal(out.reshape(rows, cols, 3), np.asarray(Jpeg.decompress(data).convert("RGB")))


# ---- the command line -----------------------------------------------------------------------------------------------------
CLI = [(72, 104, 2, 8, "qtable", "jpegx_host_compress_image_rgb", "jpegx_host_decompress_image_rgb"),
       (192, 192, 1, 4, "divide40", "jpegx_host_compress_image_rgb_n", "jpegx_host_decompress_image_rgb_n")]


@pytest.mark.parametrize("rows, cols, bs, n, qname, forward_entry, back_entry", CLI)
def test_cli_files(gpu, native, tmp_path, rows, cols, bs, n, qname, forward_entry, back_entry):
    from PIL import Image
    import compress
    import decompress
    from jpegx import synth
    if (rows, cols) == (72, 104):                        # the picture of test_gpu_pipeline.test_cli_compress_decompress_files
        rgb = np.dstack([synth.generate_plane("smooth", rows, cols, seed=s, dtype=np.uint8) for s in (4, 5, 6)])
    else:
        rgb = picture(rows, cols)
    src, packed, back = tmp_path / "in.png", tmp_path / "out.bin", tmp_path / "back.png"
    Image.fromarray(rgb, mode="RGB").save(src)
    compress.compress(str(src), str(packed), block_size=bs, dct_size=n, transform="DCT", quantization=quantiser(qname))
    assert native.take() == {forward_entry: 1}
    cfg = config_of(rows, cols, bs, n, quantiser(qname))
    assert packed.read_bytes() == Jpeg(cfg).compress(Image.open(src).convert("YCbCr"))
    native.take()
    decompress.decompress(str(packed), str(back))
    assert native.take() == {back_entry: 1}
    got = Image.open(back)
    assert got.mode == "RGB"
    assert np.array_equal(np.asarray(got), np.asarray(Jpeg.decompress(packed.read_bytes()).convert("RGB")))
