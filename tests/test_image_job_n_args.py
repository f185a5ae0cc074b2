"""The four entries of the dct_size-N picture job (jpegx_band_planes_packed_n, jpegx_inflate_crop_pack_u8,
jpegx_host_compress_image_packed_n, jpegx_host_decompress_image_n): every bad argument refused before a device is needed,
with the return code the band entries give for the same fault; the binding's entries; and Jpeg.compress / Jpeg.decompress
keeping the per-band roads while the two picture gates are None or above the plane.  CPU only."""
import ctypes

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -4
NONE, DISCARD, DIVIDE, QTABLE = 0, 1, 2, 3
NAMES = ("jpegx_band_planes_packed_n", "jpegx_inflate_crop_pack_u8", "jpegx_host_compress_image_packed_n", "jpegx_host_decompress_image_n")


def _aligned(nbytes=4096):
    buf = ctypes.create_string_buffer(nbytes + 256)
    return buf, (ctypes.addressof(buf) + 255) & ~255


class Calls:
    """The four entries with one valid-looking argument list each (12 x 20 pixels, 3 bands, block_size 3, N 4: a 4 x 8
    plane); a call replaces arguments by name.  Nothing here may reach a device: every call below is refused first."""

    def __init__(self, jpegx, on=False):
        self.L = jpegx.lib()
        self.keep, p = _aligned()
        self.p = p
        self.ptrs = (ctypes.c_void_p * 4)(p, p, p, p)
        self.sizes = (ctypes.c_size_t * 4)(10, 10, 10, 10)
        self.out_sizes = (ctypes.c_size_t * 4)()

        def never(_user, _n):
            raise AssertionError("the allocator was asked")
        self.cb = jpegx.ALLOC_FN(never)
        self.on = on

    def _call(self, name, order, kw):
        unknown = set(kw) - {k for k, _ in order}
        assert not unknown, unknown
        args = [kw.get(k, d) for k, d in order]
        fn = getattr(self.L, name + ("_on" if self.on else ""))
        return fn(0, *args) if self.on else fn(*args)

    def gather(self, **kw):
        return self._call(NAMES[0], (("pixels", self.p), ("nbands", 3), ("rows", 12), ("cols", 20), ("pitch", 60), ("bs", 3), ("N", 4),
                                     ("planes", self.ptrs), ("out_pitch", 8), ("stream", None)), kw)

    def scatter(self, **kw):
        return self._call(NAMES[1], (("planes", self.ptrs), ("nbands", 3), ("pitch", 8), ("rows", 12), ("cols", 20), ("bs", 3),
                                     ("out", self.p), ("out_pitch", 60), ("stream", None)), kw)

    def compress(self, **kw):
        return self._call(NAMES[2], (("pixels", self.p), ("nbands", 3), ("rows", 12), ("cols", 20), ("pitch", 60), ("bs", 3), ("N", 4),
                                     ("mode", NONE), ("param", 0.0), ("prefix", None), ("prefix_len", 0), ("length_prefixes", 1),
                                     ("alloc", self.cb), ("user", None), ("nbytes", self.out_sizes)), kw)

    def decompress(self, **kw):
        return self._call(NAMES[3], (("bytes", self.ptrs), ("sizes", self.sizes), ("nbands", 3), ("rows", 12), ("cols", 20), ("bs", 3),
                                     ("N", 4), ("mode", NONE), ("param", 0.0), ("out", self.p), ("out_pitch", 60), ("interleave", 1)), kw)

    def err(self):
        return self.L.jpegx_last_error()


def _refusals(c):
    every = (c.gather, c.scatter, c.compress, c.decompress)
    with_n = (c.gather, c.compress, c.decompress)
    jobs = (c.compress, c.decompress)
    # null pointers
    assert c.gather(pixels=None) == INVALID and b"null" in c.err()
    assert c.gather(planes=None) == INVALID and b"null" in c.err()
    assert c.gather(planes=(ctypes.c_void_p * 4)(c.p, None, c.p, c.p)) == INVALID and b"null" in c.err()
    assert c.scatter(planes=None) == INVALID and b"null" in c.err()
    assert c.scatter(planes=(ctypes.c_void_p * 4)(c.p, c.p, None, c.p)) == INVALID and b"null" in c.err()
    assert c.scatter(out=None) == INVALID and b"null" in c.err()
    assert c.compress(pixels=None) == INVALID and b"null" in c.err()
    assert c.compress(alloc=None) == INVALID and b"null" in c.err()
    assert c.compress(nbytes=None) == INVALID and b"null" in c.err()
    assert c.compress(prefix=None, prefix_len=4) == INVALID and b"null" in c.err()
    assert c.decompress(bytes=None) == INVALID and b"null" in c.err()
    assert c.decompress(sizes=None) == INVALID and b"null" in c.err()
    assert c.decompress(out=None) == INVALID and b"null" in c.err()
    assert c.decompress(bytes=(ctypes.c_void_p * 4)(c.p, None, c.p, c.p)) == INVALID and b"null" in c.err()
    for call in every:
        for nb in (0, 5, -1):
            assert call(nbands=nb) == INVALID and b"bands" in c.err(), (call.__name__, nb)
        for kw in ({"rows": 0}, {"cols": 0}, {"rows": -3}):
            assert call(**kw) == INVALID and b"rows and cols" in c.err(), (call.__name__, kw)
        for bs in (0, 256):
            assert call(bs=bs) == UNSUPPORTED and b"block_size" in c.err(), (call.__name__, bs)
    for call in with_n:
        for n in (1, 33):
            assert call(N=n) == INVALID and b"2 .. 32" in c.err(), (call.__name__, n)
    # exactly 2^31 samples in a band: at block_size 1 the plane is as large; at block_size 2 only the band is
    big = dict(rows=1 << 16, cols=1 << 15)
    wide = 3 << 15
    assert c.gather(bs=1, pitch=wide, out_pitch=1 << 15, **big) == INVALID and b"2^31" in c.err()
    assert c.gather(bs=2, pitch=wide, out_pitch=1 << 15, **big) == INVALID and b"2^31" in c.err()
    assert c.scatter(bs=2, pitch=1 << 15, out_pitch=wide, **big) == INVALID and b"2^31" in c.err()
    assert c.compress(bs=1, pitch=wide, **big) == INVALID and b"2^31" in c.err()
    assert c.compress(bs=2, pitch=wide, **big) == INVALID and b"2^31" in c.err()
    assert c.decompress(bs=1, out_pitch=wide, **big) == INVALID and b"2^31" in c.err()
    assert c.decompress(bs=2, out_pitch=wide, **big) == INVALID and b"2^31" in c.err()
    # a packed pitch below cols * nbands
    assert c.gather(pitch=59) == INVALID and b"pitch" in c.err()
    assert c.scatter(out_pitch=59) == INVALID and b"pitch" in c.err()
    assert c.compress(pitch=59) == INVALID and b"pitch" in c.err()
    assert c.decompress(out_pitch=59) == INVALID and b"pitch" in c.err()
    assert c.decompress(out_pitch=19, interleave=0) == INVALID and b"pitch" in c.err()
    assert c.gather(nbands=4, pitch=79) == INVALID and b"pitch" in c.err()
    # a plane pitch below the plane's row: W = 8 doubles on the way in, ceil(20 / 3) = 7 bytes on the way back
    assert c.gather(out_pitch=7) == INVALID and b"pitch" in c.err()
    assert c.scatter(pitch=6) == INVALID and b"pitch" in c.err()
    assert c.scatter(bs=1, pitch=19) == INVALID and b"pitch" in c.err()
    # a plane pointer off 8 bytes
    assert c.gather(planes=(ctypes.c_void_p * 4)(c.p, c.p + 4, c.p, c.p)) == INVALID and b"misaligned" in c.err()
    for call in jobs:
        assert call(mode=QTABLE) == INVALID and b"quantisers" in c.err(), call.__name__      # the luminance table needs dct_size 8
        assert call(mode=7) == INVALID and b"quantisers" in c.err(), call.__name__
        assert call(mode=DISCARD, param=2.5) == INVALID and b"keep" in c.err(), call.__name__
        assert call(mode=DISCARD, param=-1.0) == INVALID and b"keep" in c.err(), call.__name__
        assert call(mode=DIVIDE, param=0.0) == INVALID and b"divisor" in c.err(), call.__name__
        assert call(mode=DIVIDE, param=float("nan")) == INVALID and b"divisor" in c.err(), call.__name__
    assert c.decompress(sizes=(ctypes.c_size_t * 4)(10, 0, 10, 10)) == INVALID and b"empty" in c.err()


def test_every_entry_validates_before_any_device_work():
    import jpegx
    c = Calls(jpegx)
    _refusals(c)
    assert c.L.jpegx_host_compress_finish(None) == INVALID                 # nothing here took a job context


def test_the_explicit_device_twins_refuse_as_well():
    import jpegx
    c = Calls(jpegx, on=True)
    if jpegx.device_count() > 0:                    # the twins make device 0 current first: with one they refuse with the same codes
        _refusals(c)
    else:
        assert c.gather(pixels=None) != 0 and c.scatter(bs=0) != 0 and c.compress(N=33) != 0 and c.decompress(nbands=5) != 0


def test_the_band_entries_give_the_same_codes():
    """The faults the picture entries share with the band entries, at the band entries: the codes asserted above are theirs."""
    import jpegx
    L = jpegx.lib()
    keep, p = _aligned()
    nbytes = ctypes.c_size_t(0)
    plane = lambda **kw: L.jpegx_band_plane_n(*[kw.get(k, d) for k, d in (
        ("band", p), ("rows", 12), ("cols", 20), ("pitch", 20), ("bs", 3), ("N", 4), ("out", p), ("out_pitch", 8), ("stream", None))])
    crop = lambda **kw: L.jpegx_inflate_crop_u8(*[kw.get(k, d) for k, d in (
        ("plane", p), ("pitch", 8), ("rows", 12), ("cols", 20), ("bs", 3), ("out", p), ("out_pitch", 20), ("stream", None))])
    begin = lambda **kw: L.jpegx_host_compress_begin_band_n(*[kw.get(k, d) for k, d in (
        ("band", p), ("elem", 1), ("rows", 12), ("cols", 20), ("pitch", 20), ("bs", 3), ("N", 4), ("mode", NONE), ("param", 0.0),
        ("nbytes", ctypes.byref(nbytes)))])
    back = lambda **kw: L.jpegx_host_decompress_band_n(*[kw.get(k, d) for k, d in (
        ("bytes", p), ("nbytes", 10), ("rows", 12), ("cols", 20), ("bs", 3), ("N", 4), ("mode", NONE), ("param", 0.0), ("out", p), ("pitch", 20))])
    for call in (plane, crop, begin, back):
        assert call(rows=0) == INVALID and call(cols=0) == INVALID
        assert call(bs=0) == UNSUPPORTED and call(bs=256) == UNSUPPORTED
    for call in (plane, begin, back):
        assert call(N=1) == INVALID and call(N=33) == INVALID
    assert plane(band=None) == INVALID and crop(out=None) == INVALID and begin(band=None) == INVALID and back(out=None) == INVALID
    assert plane(pitch=19) == INVALID and plane(out_pitch=7) == INVALID and crop(pitch=6) == INVALID and crop(out_pitch=19) == INVALID
    assert begin(pitch=19) == INVALID and back(pitch=19) == INVALID
    for call in (begin, back):
        assert call(mode=QTABLE) == INVALID and call(mode=DISCARD, param=2.5) == INVALID and call(mode=DIVIDE, param=0.0) == INVALID
    del keep


def test_signatures_hold_the_new_entries():
    import jpegx
    for name in NAMES:
        assert name in jpegx.SIGNATURES and name + "_on" in jpegx.SIGNATURES
        assert jpegx.SIGNATURES[name + "_on"] == [ctypes.c_int] + jpegx.SIGNATURES[name]
    for name in ("band_planes_packed_n", "inflate_crop_pack_u8", "compress_image_packed_n", "decompress_image_n"):
        assert callable(getattr(jpegx, name))


def test_python_wrappers_refuse_bad_arguments():
    import jpegx
    with pytest.raises(jpegx.JpegxError, match="uint8 pixels"):
        jpegx.band_planes_packed_n(np.zeros((4, 4)), 1, 4)
    with pytest.raises(jpegx.JpegxError, match="uint8 pixels"):
        jpegx.band_planes_packed_n(np.zeros((4, 4, 5), np.uint8), 1, 4)
    with pytest.raises(jpegx.JpegxError, match="2 .. 32"):
        jpegx.band_planes_packed_n(np.zeros((4, 4, 3), np.uint8), 1, 33)
    with pytest.raises(jpegx.JpegxError, match="pitch"):
        jpegx.band_planes_packed_n(np.zeros((4, 4, 3), np.uint8), 1, 4, pitch=11)
    with pytest.raises(jpegx.JpegxError, match="planes of one shape"):
        jpegx.inflate_crop_pack_u8([np.zeros((4, 4), np.uint8), np.zeros((4, 5), np.uint8)], 4, 4, 1)
    with pytest.raises(jpegx.JpegxError, match="planes of one shape"):
        jpegx.inflate_crop_pack_u8([], 4, 4, 1)
    with pytest.raises(jpegx.JpegxError, match="smaller than the pooled band"):
        jpegx.inflate_crop_pack_u8([np.zeros((4, 4), np.uint8)], 9, 8, 2)
    with pytest.raises(jpegx.JpegxError, match="block_size"):
        jpegx.inflate_crop_pack_u8([np.zeros((4, 4), np.uint8)], 4, 4, 0)
    with pytest.raises(jpegx.JpegxError, match="rows and cols"):
        jpegx.inflate_crop_pack_u8([np.zeros((4, 4), np.uint8)], 0, 4, 1)
    assert jpegx.compress_image_packed_n(np.zeros((4, 4, 3), np.int32), 1, 4) is None
    assert jpegx.compress_image_packed_n(np.zeros((4, 4), np.uint8), 1, 4) is None
    assert jpegx.compress_image_packed_n(np.zeros((4, 8, 3), np.uint8)[:, ::2], 1, 4) is None
    with pytest.raises(jpegx.JpegxError, match="2 .. 32"):
        jpegx.compress_image_packed_n(np.zeros((4, 4, 3), np.uint8), 1, 64)
    with pytest.raises(jpegx.JpegxError, match="quantisers"):
        jpegx.compress_image_packed_n(np.zeros((4, 4, 3), np.uint8), 1, 4, "qtable")
    with pytest.raises(jpegx.JpegxError, match="1..4 bands"):
        jpegx.decompress_image_n([], 4, 4, 1, 4)
    with pytest.raises(jpegx.JpegxError, match="rows and cols"):
        jpegx.decompress_image_n([b"\x00"] * 3, 0, 4, 1, 4)
    with pytest.raises(jpegx.JpegxError, match="null"):                 # an empty blob has no address
        jpegx.decompress_image_n([b"\x00", b"", b"\x00"], 4, 4, 1, 4)
    with pytest.raises(jpegx.JpegxError, match="block_size"):
        jpegx.decompress_image_n([b"\x00"] * 3, 4, 4, 256, 4, interleave=False)


def test_no_cpu_fallback_without_a_device():
    import jpegx
    if jpegx.device_count() > 0:
        pytest.skip("a GPU is present; the loud-failure path is covered on the CPU container")
    with pytest.raises(jpegx.JpegxError):
        jpegx.band_planes_packed_n(np.zeros((4, 4, 3), np.uint8), 1, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.inflate_crop_pack_u8([np.zeros((4, 4), np.uint8)] * 3, 4, 4, 1)
    with pytest.raises(jpegx.JpegxError):
        jpegx.compress_image_packed_n(np.zeros((4, 4, 3), np.uint8), 1, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.decompress_image_n([bytes(16)] * 3, 16, 16, 1, 4)


def _boom(what):
    def boom(*a, **k):
        raise AssertionError(what)
    return boom


def test_the_gates_are_there_and_not_below_their_floor():
    import pipeline
    for name in ("DCTN_IMAGE_JOB_MIN_SAMPLES", "DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES"):
        gate = getattr(pipeline, name)
        assert gate is None or gate >= 16384, name


def test_what_the_jobs_are_not_asked_for(monkeypatch):
    """_compress_pixels_n's and _decompress_image_n's own conditions, checked before a device is asked about: each answers
    None without a call -- whatever the machine."""
    import jpegx
    import pipeline
    from PIL import Image
    from pipeline.base import AlgorithmStep, step_classes
    monkeypatch.setattr(jpegx, "compress_image_packed_n", _boom("the picture job was asked"))
    monkeypatch.setattr(jpegx, "decompress_image_n", _boom("the picture decode job was asked"))
    monkeypatch.setattr(pipeline, "_device_usable", lambda: True)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    monkeypatch.setattr(pipeline, "DCTN_IMAGE_JOB_MIN_SAMPLES", 0)
    monkeypatch.setattr(pipeline, "DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES", 0)
    q = lambda **kw: pipeline.QuantizationMethod("divide", **kw)
    cfg = lambda **kw: pipeline.Configuration(**dict(dict(width=20, height=12, block_size=1, dct_size=4, quantization=q(divisor=10)), **kw))
    image = Image.fromarray(np.zeros((12, 20, 3), np.uint8), mode="YCbCr")
    pack, unpack = pipeline._compress_pixels_n, pipeline._decompress_image_n
    blobs = (b"\x00", b"\x00", b"\x00")
    with pytest.raises(AssertionError, match="picture job was asked"):          # the controls: these are the jobs'
        pack(image, cfg())
    with pytest.raises(AssertionError, match="decode job was asked"):
        unpack(blobs, cfg())
    # the picture
    assert pack(image, cfg(height=13)) is None                                  # not the configured size
    assert pack(Image.fromarray(np.zeros((12, 20), np.uint8)), cfg()) is None   # one band
    assert pack(Image.fromarray(np.zeros((12, 20, 4), np.uint8), mode="CMYK"), cfg()) is None
    assert pack(object(), cfg()) is None
    # the configuration
    for bad in (dict(dct_size=8), dict(dct_size=33), dict(transform="DFT"), dict(block_size=0), dict(block_size=256), dict(block_size=2.0),
                dict(quantization=q(divisor=1e-9))):                            # 255 * 16 / 1e-9 leaves the int32 range
        assert pack(image, cfg(**bad)) is None, bad
    for bad in (dict(dct_size=8), dict(dct_size=33), dict(transform="DFT"), dict(block_size=0), dict(block_size=256), dict(block_size=2.0),
                dict(quantization=q(divisor=2.5)), dict(height=0), dict(width=20.0), dict(height=1 << 16, width=1 << 15, block_size=2)):
        assert unpack(blobs, cfg(**bad)) is None, bad
    assert unpack((b"\x00", b"", b"\x00"), cfg()) is None
    assert unpack((b"\x00", np.zeros(4), b"\x00"), cfg()) is None
    # the gates and the other constants
    for name, call in (("DCTN_IMAGE_JOB_MIN_SAMPLES", lambda: pack(image, cfg())), ("DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES", lambda: unpack(blobs, cfg()))):
        for gate in (None, 12 * 20 + 1, 1 << 40):
            with monkeypatch.context() as m:
                m.setattr(pipeline, name, gate)
                assert call() is None, (name, gate)
        with monkeypatch.context() as m:
            m.setattr(pipeline, "DCTN_MIN_SAMPLES", 1 << 20)                    # dctn_on_device
            assert call() is None, name
        with monkeypatch.context() as m:
            m.setattr(pipeline, "_device_usable", lambda: False)
            assert call() is None, name
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_ENTROPY_MIN_SAMPLES", 0)                      # that plane is compress_plane_n's
        assert pack(image, cfg()) is None
    stock = list(step_classes)
    try:
        class PassThrough(AlgorithmStep):
            step_index = 9.5

            def execute(self, array):
                return array

            def invert(self, array):
                return array
        assert not pipeline._stock_registry()
        assert pack(image, cfg()) is None and unpack(blobs, cfg()) is None
    finally:
        step_classes[:] = stock


def test_gates_off_or_above_the_plane_keep_the_roads_of_before(monkeypatch):
    """With either gate at None, above the plane or as shipped, a small picture takes neither job -- whatever the machine --
    and the container and the picture are the same each time."""
    import jpegx
    import pipeline
    from PIL import Image
    monkeypatch.setattr(jpegx, "compress_image_packed_n", _boom("Jpeg.compress took the picture job"))
    monkeypatch.setattr(jpegx, "decompress_image_n", _boom("Jpeg.decompress took the picture job"))
    h, w, bs, n = 31, 43, 3, 5                                             # a 15 x 15 plane
    pixels = np.random.default_rng(5).integers(0, 256, (h, w, 3)).astype(np.uint8)
    cfg = pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n, quantization=pipeline.QuantizationMethod("divide", divisor=10))
    seen = []
    for gates in ((pipeline.DCTN_IMAGE_JOB_MIN_SAMPLES, pipeline.DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES), (None, None), (226, 226), (1 << 40, 1 << 40)):
        monkeypatch.setattr(pipeline, "DCTN_IMAGE_JOB_MIN_SAMPLES", gates[0])
        monkeypatch.setattr(pipeline, "DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES", gates[1])
        data = pipeline.Jpeg(cfg).compress(Image.fromarray(pixels, mode="YCbCr"))
        seen.append((data, np.asarray(pipeline.Jpeg.decompress(data))))
    for data, back in seen:
        assert data == seen[0][0] and back.shape == (h, w, 3) and np.array_equal(back, seen[0][1])
    with pytest.raises(ValueError, match="not enough values"):
        pipeline.Jpeg(cfg).compress(Image.fromarray(pixels[:, :, 0]))
