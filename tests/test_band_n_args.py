"""The entries of the dct_size-N band job (jpegx_band_shape_n, jpegx_band_plane_n, jpegx_host_compress_begin_band_n):
the shape arithmetic against pipeline.geometry, every bad argument refused before a device is needed, and -- on a
machine without a GPU -- errors instead of numbers, with compress_band keeping its road.  CPU only."""
import ctypes

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -4


def _aligned(nbytes=4096):
    buf = ctypes.create_string_buffer(nbytes + 256)
    return buf, (ctypes.addressof(buf) + 255) & ~255


def test_band_shape_n_is_band_geometry():
    import jpegx
    import pipeline
    from pipeline import geometry
    for bs in range(1, 7):
        for n in range(2, 10):
            for rows in range(1, 41):
                cfgs = [pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n) for cols in range(1, 41)]
                want = [geometry.band_geometry(cfg)[3] for cfg in cfgs]
                got = [jpegx.band_shape_n(rows, cols, bs, n) for cols in range(1, 41)]
                assert got == want, (bs, n, rows)


def test_band_shape_n_refuses_bad_arguments():
    import jpegx
    L = jpegx.lib()
    h, w = ctypes.c_int(-7), ctypes.c_int(-7)
    H, W = ctypes.byref(h), ctypes.byref(w)
    err = lambda: L.jpegx_last_error()
    assert L.jpegx_band_shape_n(10, 10, 1, 4, None, W) == INVALID and b"null" in err()
    assert L.jpegx_band_shape_n(10, 10, 1, 4, H, None) == INVALID and b"null" in err()
    assert L.jpegx_band_shape_n(0, 10, 1, 4, H, W) == INVALID and b"rows and cols" in err()
    assert L.jpegx_band_shape_n(10, 0, 1, 4, H, W) == INVALID and b"rows and cols" in err()
    assert L.jpegx_band_shape_n(10, -3, 1, 4, H, W) == INVALID
    assert L.jpegx_band_shape_n(10, 10, 0, 4, H, W) == UNSUPPORTED and b"block_size" in err()
    assert L.jpegx_band_shape_n(10, 10, 256, 4, H, W) == UNSUPPORTED and b"block_size" in err()
    assert L.jpegx_band_shape_n(10, 10, 1, 1, H, W) == INVALID and b"2 .. 32" in err()
    assert L.jpegx_band_shape_n(10, 10, 1, 33, H, W) == INVALID and b"2 .. 32" in err()
    assert L.jpegx_band_shape_n(1 << 16, 1 << 15, 1, 4, H, W) == INVALID and b"2^31" in err()      # exactly 2^31 samples
    assert L.jpegx_band_shape_n(2 ** 31 - 1, 2 ** 31 - 1, 1, 2, H, W) == INVALID and b"2^31" in err()
    assert (h.value, w.value) == (-7, -7)                               # a refusal writes nothing
    # the largest planes that are taken: 2^31 - 4 samples, and a band of 2^31 - 1 rows at the largest block_size
    assert L.jpegx_band_shape_n((1 << 30) - 3, 1, 1, 2, H, W) == 0 and (h.value, w.value) == ((1 << 30) - 2, 2)
    assert L.jpegx_band_shape_n(2 ** 31 - 1, 1, 255, 2, H, W) == 0 and (h.value, w.value) == (8421506, 2)
    assert L.jpegx_band_shape_n(46340 * 255, 46339 * 255 + 1, 255, 2, H, W) == 0 and (h.value, w.value) == (46340, 46340)
    with pytest.raises(jpegx.JpegxError, match="2 .. 32"):
        jpegx.band_shape_n(4, 4, 1, 64)


def test_band_plane_n_validates_before_any_device_work():
    import jpegx
    L = jpegx.lib()
    keep, p = _aligned()
    err = lambda: L.jpegx_last_error()
    plane = lambda **kw: L.jpegx_band_plane_n(*[kw.get(k, d) for k, d in (
        ("band", p), ("rows", 12), ("cols", 20), ("pitch", 20), ("bs", 1), ("N", 4), ("out", p), ("out_pitch", 20), ("stream", None))])
    assert plane(band=None) == INVALID and b"null" in err()
    assert plane(out=None) == INVALID and b"null" in err()
    assert plane(rows=0) == INVALID and b"rows and cols" in err()
    assert plane(cols=0) == INVALID and b"rows and cols" in err()
    assert plane(bs=0) == UNSUPPORTED and b"block_size" in err()
    assert plane(bs=256) == UNSUPPORTED and b"block_size" in err()
    assert plane(N=1) == INVALID and b"2 .. 32" in err()
    assert plane(N=33) == INVALID and b"2 .. 32" in err()
    assert plane(pitch=19) == INVALID and b"pitch" in err()
    assert plane(out_pitch=19) == INVALID and b"pitch" in err()
    assert plane(cols=21, pitch=21, out_pitch=23) == INVALID and b"pitch" in err()      # W is 24 after DCT padding
    assert plane(rows=1 << 16, cols=1 << 15, pitch=1 << 15, out_pitch=1 << 15) == INVALID and b"2^31" in err()
    assert plane(out=p + 4) == INVALID and b"misaligned" in err()
    assert L.jpegx_band_plane_n_on(0, None, 12, 20, 20, 1, 4, p, 20, None) != 0
    del keep


def test_band_job_validates_before_any_device_work():
    import jpegx
    L = jpegx.lib()
    keep, p = _aligned()
    n = ctypes.c_size_t(0)
    err = lambda: L.jpegx_last_error()
    job = lambda **kw: L.jpegx_host_compress_begin_band_n(*[kw.get(k, d) for k, d in (
        ("band", p), ("elem", 1), ("rows", 12), ("cols", 20), ("pitch", 20), ("bs", 1), ("N", 4), ("mode", 0), ("param", 0.0),
        ("nbytes", ctypes.byref(n)))])
    assert job(band=None) == INVALID and b"null" in err()
    assert job(nbytes=None) == INVALID and b"null" in err()
    assert job(elem=2) == UNSUPPORTED and b"uint8, int32 or int64" in err()
    assert job(elem=0) == UNSUPPORTED
    assert job(rows=0) == INVALID and b"rows and cols" in err()
    assert job(cols=0) == INVALID and b"rows and cols" in err()
    assert job(bs=0) == UNSUPPORTED and b"block_size" in err()
    assert job(bs=256) == UNSUPPORTED and b"block_size" in err()
    assert job(N=1) == INVALID and b"2 .. 32" in err()
    assert job(N=33) == INVALID and b"2 .. 32" in err()
    assert job(pitch=19) == INVALID and b"pitch" in err()
    assert job(rows=1 << 16, cols=1 << 15, pitch=1 << 15) == INVALID and b"2^31" in err()
    assert job(mode=3) == INVALID and b"quantisers" in err()                # qtable needs dct_size 8
    assert job(mode=7) == INVALID and b"quantisers" in err()
    assert job(mode=2, param=0.0) == INVALID and b"divisor" in err()
    assert job(mode=2, param=float("nan")) == INVALID and b"divisor" in err()
    assert job(mode=2, param=float("inf")) == INVALID and b"divisor" in err()
    assert job(mode=1, param=-1.0) == INVALID and b"keep" in err()
    assert job(mode=1, param=1.5) == INVALID and b"keep" in err()
    assert L.jpegx_host_compress_finish(None) == INVALID                   # none of these left a job open
    assert L.jpegx_host_compress_begin_band_n_on(0, None, 1, 12, 20, 20, 1, 4, 0, 0.0, ctypes.byref(n)) != 0
    del keep


def test_the_shared_quantiser_checks_still_guard_the_older_entries():
    """jpegx_host_compress_begin_n and jpegx_host_decompress_plane_n share one check of the quantiser with the band job."""
    import jpegx
    L = jpegx.lib()
    keep, p = _aligned()
    n = ctypes.c_size_t(0)
    err = lambda: L.jpegx_last_error()
    for mode, param, word in ((3, 0.0, b"quantisers"), (2, 0.0, b"divisor"), (1, -1.0, b"keep")):
        assert L.jpegx_host_compress_begin_n(p, 16, 16, 16, 4, mode, param, ctypes.byref(n)) == INVALID and word in err()
        assert L.jpegx_host_decompress_plane_n(p, 10, 16, 16, 4, mode, param, 0, p, 16) == INVALID and word in err()
    del keep


def test_python_wrappers_refuse_what_is_no_8_bit_band():
    import jpegx
    with pytest.raises(jpegx.JpegxError, match="integer dtype"):
        jpegx.band_plane_n(np.zeros((4, 4)), 1, 4)
    with pytest.raises(jpegx.JpegxError, match="integer dtype"):
        jpegx.band_plane_n(np.zeros((0, 4), np.uint8), 1, 4)
    with pytest.raises(jpegx.JpegxError, match="0..255"):
        jpegx.band_plane_n(np.full((4, 4), 256), 1, 4)
    with pytest.raises(jpegx.JpegxError, match="block_size"):
        jpegx.band_plane_n(np.zeros((4, 4), np.uint8), 0, 4)
    # compress_band_n answers None where the native entry would say "not an 8-bit band", and raises for the rest
    assert jpegx.compress_band_n(np.zeros((4, 4)), 1, 4) is None
    assert jpegx.compress_band_n(np.zeros((4, 4), np.int16), 1, 4) is None
    assert jpegx.compress_band_n(np.zeros((0, 4), np.uint8), 1, 4) is None
    assert jpegx.compress_band_n(np.zeros((4, 4), np.uint8), 256, 4) is None
    with pytest.raises(jpegx.JpegxError, match="2 .. 32"):
        jpegx.compress_band_n(np.zeros((4, 4), np.uint8), 1, 33)
    with pytest.raises(jpegx.JpegxError, match="divisor"):
        jpegx.compress_band_n(np.zeros((4, 4), np.uint8), 1, 4, "divide", 0.0)


def test_no_cpu_fallback_without_a_device():
    import jpegx
    if jpegx.device_count() > 0:
        pytest.skip("a GPU is present; the loud-failure path is covered on the CPU container")
    band = np.arange(240, dtype=np.uint8).reshape(12, 20)
    with pytest.raises(jpegx.JpegxError):
        jpegx.band_plane_n(band, 1, 4)
    for b in (band, band.astype(np.int32), band.astype(np.int64)):
        with pytest.raises(jpegx.JpegxError):
            jpegx.compress_band_n(b, 1, 4, "divide", 10.0)
    assert jpegx.lib().jpegx_host_compress_finish(None) == INVALID         # and no job is open afterwards


def test_without_a_device_the_gate_changes_nothing(monkeypatch):
    import jpegx
    import pipeline
    assert hasattr(pipeline, "DCTN_BAND_JOB_MIN_SAMPLES")
    if jpegx.device_count() > 0:
        pytest.skip("a GPU is present; tests/test_gpu_band_job_n.py compares the roads there")

    def boom(*a, **k):
        raise AssertionError("compress_band took the device job")
    monkeypatch.setattr(jpegx, "compress_band_n", boom)
    for bs, n, h, w in ((1, 4, 12, 20), (3, 5, 31, 43)):
        cfg = pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n,
                                     quantization=pipeline.QuantizationMethod("divide", divisor=10))
        band = np.random.default_rng(h * w).integers(0, 256, (h, w))
        got = {}
        for gate in (None, 0):
            monkeypatch.setattr(pipeline, "DCTN_BAND_JOB_MIN_SAMPLES", gate)
            got[gate] = pipeline.compress_band(band, cfg)
        assert isinstance(got[None], bytes) and got[0] == got[None]
        assert np.array_equal(pipeline.decompress_band(got[0], cfg).shape, (h, w))
