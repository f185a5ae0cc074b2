"""The entries of the dct_size-N band DECODE job (jpegx_inflate_crop_u8, jpegx_host_decompress_band_n,
jpegx_host_decompress_band_i64_n): every bad argument refused with its code and a telling message before a device is
needed, the Python wrappers' own refusals, and decompress_band / decompress_band_u8 keeping the road of before while
pipeline.DCTN_BAND_DECODE_JOB_MIN_SAMPLES is None or above the plane.  CPU only."""
import ctypes

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -4


def _aligned(nbytes=4096):
    buf = ctypes.create_string_buffer(nbytes + 256)
    return buf, (ctypes.addressof(buf) + 255) & ~255


def test_inflate_crop_validates_before_any_device_work():
    import jpegx
    L = jpegx.lib()
    keep, p = _aligned()
    err = lambda: L.jpegx_last_error()
    crop = lambda **kw: L.jpegx_inflate_crop_u8(*[kw.get(k, d) for k, d in (
        ("plane", p), ("pitch", 8), ("rows", 12), ("cols", 20), ("bs", 3), ("out", p), ("out_pitch", 20), ("stream", None))])
    assert crop(plane=None) == INVALID and b"null" in err()
    assert crop(out=None) == INVALID and b"null" in err()
    assert crop(rows=0) == INVALID and b"rows and cols" in err()
    assert crop(cols=0) == INVALID and b"rows and cols" in err()
    assert crop(rows=-1) == INVALID and b"rows and cols" in err()
    assert crop(bs=0) == UNSUPPORTED and b"block_size" in err()
    assert crop(bs=256) == UNSUPPORTED and b"block_size" in err()
    assert crop(pitch=6) == INVALID and b"pitch" in err()                   # ceil(20 / 3) is 7
    assert crop(bs=1, pitch=19) == INVALID and b"pitch" in err()
    assert crop(out_pitch=19) == INVALID and b"pitch" in err()
    assert crop(rows=1 << 16, cols=1 << 15, pitch=1 << 15, out_pitch=1 << 15) == INVALID and b"2^31" in err()      # exactly 2^31 samples
    assert crop(rows=2 ** 31 - 1, cols=2 ** 31 - 1, pitch=1 << 31, out_pitch=1 << 31) == INVALID and b"2^31" in err()
    assert L.jpegx_inflate_crop_u8_on(0, None, 8, 12, 20, 3, p, 20, None) != 0
    del keep


def _job_cases(call, err, with_pitch):
    assert call(bytes=None) == INVALID and b"null" in err()
    assert call(out=None) == INVALID and b"null" in err()
    assert call(rows=0) == INVALID and b"rows and cols" in err()
    assert call(cols=0) == INVALID and b"rows and cols" in err()
    assert call(cols=-5) == INVALID and b"rows and cols" in err()
    assert call(bs=0) == UNSUPPORTED and b"block_size" in err()
    assert call(bs=256) == UNSUPPORTED and b"block_size" in err()
    assert call(N=1) == INVALID and b"2 .. 32" in err()
    assert call(N=33) == INVALID and b"2 .. 32" in err()
    assert call(mode=3) == INVALID and b"quantisers" in err()               # JPEGX_Q_QTABLE needs dct_size 8
    assert call(mode=2, param=0.0) == INVALID and b"divisor" in err()
    assert call(mode=1, param=-1.0) == INVALID and b"keep" in err()
    assert call(nbytes=0) == INVALID and b"empty" in err()
    # the plane holds 2^29 samples, the band 2^31; and a plane that itself is too large
    assert call(rows=1 << 16, cols=1 << 15, bs=2, pitch=1 << 15) == INVALID and b"2^31" in err()
    assert call(rows=1 << 16, cols=1 << 15, pitch=1 << 15) == INVALID and b"2^31" in err()
    if with_pitch:
        assert call(pitch=19) == INVALID and b"pitch" in err()


def test_band_jobs_validate_before_any_device_work():
    import jpegx
    L = jpegx.lib()
    keep, p = _aligned()
    err = lambda: L.jpegx_last_error()
    names = (("bytes", p), ("nbytes", 10), ("rows", 12), ("cols", 20), ("bs", 1), ("N", 4), ("mode", 0), ("param", 0.0), ("out", p))
    u8 = lambda **kw: L.jpegx_host_decompress_band_n(*[kw.get(k, d) for k, d in names + (("pitch", 20),)])
    i64 = lambda **kw: L.jpegx_host_decompress_band_i64_n(*[kw.get(k, d) for k, d in names])
    u8_on = lambda **kw: L.jpegx_host_decompress_band_n_on(0, *[kw.get(k, d) for k, d in names + (("pitch", 20),)])
    i64_on = lambda **kw: L.jpegx_host_decompress_band_i64_n_on(0, *[kw.get(k, d) for k, d in names])
    _job_cases(u8, err, True)
    _job_cases(i64, err, False)
    if jpegx.device_count() > 0:                    # the twins make device 0 current first: with one they refuse with the same codes
        _job_cases(u8_on, err, True)
        _job_cases(i64_on, err, False)
    else:
        assert u8_on(bytes=None) != 0 and i64_on(bytes=None) != 0 and u8_on(bs=0) != 0 and i64_on(N=33) != 0
    assert L.jpegx_host_compress_finish(None) == INVALID                   # nothing here took a job context
    del keep


def test_python_wrappers_refuse_bad_arguments():
    import jpegx
    with pytest.raises(jpegx.JpegxError, match="out must be"):
        jpegx.decompress_band_n(b"\x00", 4, 4, 1, 4, out="f32")
    with pytest.raises(jpegx.JpegxError, match="out must be"):
        jpegx.decompress_band_n(b"\x00", 4, 4, 1, 4, out="i32")
    with pytest.raises(jpegx.JpegxError, match="2 .. 32"):
        jpegx.decompress_band_n(b"\x00", 4, 4, 1, 64)
    with pytest.raises(jpegx.JpegxError, match="block_size"):
        jpegx.decompress_band_n(b"\x00", 4, 4, 256, 4, out="i64")
    with pytest.raises(jpegx.JpegxError, match="null"):                 # an empty blob has no address
        jpegx.decompress_band_n(b"", 4, 4, 1, 4)
    with pytest.raises(jpegx.JpegxError, match="uint8 plane"):
        jpegx.inflate_crop_u8(np.zeros((4, 4)), 1, 4, 4)
    with pytest.raises(jpegx.JpegxError, match="smaller than the pooled band"):
        jpegx.inflate_crop_u8(np.zeros((4, 4), np.uint8), 2, 9, 8)
    with pytest.raises(jpegx.JpegxError, match="block_size"):
        jpegx.inflate_crop_u8(np.zeros((4, 4), np.uint8), 0, 4, 4)
    with pytest.raises(jpegx.JpegxError, match="rows and cols"):
        jpegx.inflate_crop_u8(np.zeros((4, 4), np.uint8), 1, 0, 4)


def test_signatures_hold_the_new_entries():
    import jpegx
    for name in ("jpegx_inflate_crop_u8", "jpegx_host_decompress_band_n", "jpegx_host_decompress_band_i64_n"):
        assert name in jpegx.SIGNATURES and name + "_on" in jpegx.SIGNATURES
        assert jpegx.SIGNATURES[name + "_on"] == [ctypes.c_int] + jpegx.SIGNATURES[name]


def test_no_cpu_fallback_without_a_device():
    import jpegx
    if jpegx.device_count() > 0:
        pytest.skip("a GPU is present; the loud-failure path is covered on the CPU container")
    with pytest.raises(jpegx.JpegxError):
        jpegx.inflate_crop_u8(np.zeros((4, 4), np.uint8), 2, 8, 8)
    for out in ("u8", "i64"):
        with pytest.raises(jpegx.JpegxError):
            jpegx.decompress_band_n(bytes(16), 16, 16, 1, 4, out=out)


def test_gate_off_or_above_the_plane_keeps_the_road_of_before(monkeypatch):
    """With the gate at None, and with planes below a set gate, decompress_band_n is never called -- whatever the machine."""
    import jpegx
    import pipeline
    assert hasattr(pipeline, "DCTN_BAND_DECODE_JOB_MIN_SAMPLES")
    shipped = pipeline.DCTN_BAND_DECODE_JOB_MIN_SAMPLES
    assert shipped is None or shipped > 262144

    def boom(*a, **k):
        raise AssertionError("decompress_band took the band decode job")
    monkeypatch.setattr(jpegx, "decompress_band_n", boom)
    for bs, n, h, w in ((1, 4, 12, 20), (3, 5, 31, 43)):
        cfg = pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n,
                                     quantization=pipeline.QuantizationMethod("divide", divisor=10))
        blob = pipeline.compress_band(np.random.default_rng(h * w).integers(0, 256, (h, w)), cfg)
        pooled = [-(-v // bs) for v in (h, w)]
        samples = (-(-pooled[0] // n) * n) * (-(-pooled[1] // n) * n)
        got = []
        for gate in (shipped, None, samples + 1, 1 << 40):
            monkeypatch.setattr(pipeline, "DCTN_BAND_DECODE_JOB_MIN_SAMPLES", gate)
            got.append((pipeline.decompress_band(blob, cfg), pipeline.decompress_band_u8(blob, cfg)))
        for band, band_u8 in got:
            assert band.shape == band_u8.shape == (h, w) and band.dtype == np.dtype(int) and band_u8.dtype == np.uint8
            assert np.array_equal(band, got[0][0]) and np.array_equal(band_u8, got[0][1])
        if jpegx.device_count() == 0:                                   # without a usable device the constant changes nothing
            monkeypatch.setattr(pipeline, "DCTN_BAND_DECODE_JOB_MIN_SAMPLES", 0)
            assert np.array_equal(pipeline.decompress_band(blob, cfg), got[0][0])
            assert np.array_equal(pipeline.decompress_band_u8(blob, cfg), got[0][1])


def test_what_the_job_is_not_asked_for(monkeypatch):
    """_band_decode_job_n's own conditions, checked before a device is asked about: each answers None without a call."""
    import jpegx
    import pipeline

    def boom(*a, **k):
        raise AssertionError("the band decode job was asked")
    monkeypatch.setattr(jpegx, "decompress_band_n", boom)
    monkeypatch.setattr(pipeline, "DCTN_BAND_DECODE_JOB_MIN_SAMPLES", 0)
    monkeypatch.setattr(pipeline, "_device_usable", lambda: True)
    q = lambda **kw: pipeline.QuantizationMethod("divide", **kw)
    cfg = lambda **kw: pipeline.Configuration(**dict(dict(width=20, height=12, block_size=1, dct_size=4, quantization=q(divisor=10)), **kw))
    job = pipeline._band_decode_job_n
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    for out in ("u8", "i64"):
        with pytest.raises(AssertionError, match="was asked"):                  # the control: this one is the job's
            job(b"\x00", cfg(), out)
        assert job(b"", cfg(), out) is None
        assert job(np.zeros(4), cfg(), out) is None
        assert job(b"\x00", cfg(quantization=q(divisor=2.5)), out) is None       # the reference truncates: _whole_divisor
        assert job(b"\x00", cfg(block_size=0), out) is None
        assert job(b"\x00", cfg(block_size=256), out) is None
        assert job(b"\x00", cfg(block_size=2.0), out) is None
        assert job(b"\x00", cfg(height=0), out) is None
        assert job(b"\x00", cfg(width=20.0), out) is None
        assert job(b"\x00", cfg(height=1 << 16, width=1 << 15, block_size=2), out) is None
        assert job(b"\x00", cfg(dct_size=8), out) is None                       # dct_size 8 has its own roads
        monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1 << 20)
        assert job(b"\x00", cfg(), out) is None                                 # dctn_on_device
        monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
