"""The entries of the run-time block length device decoder refuse bad arguments before any device work, size their
workspace from the arguments alone, and -- on a machine without a GPU -- raise instead of computing.  CPU only."""
import ctypes

import numpy as np
import pytest


def _aligned(nbytes=256):
    buf = ctypes.create_string_buffer(nbytes + 256)
    return buf, (ctypes.addressof(buf) + 255) & ~255


def test_device_entry_validates_before_any_device_work():
    import jpegx
    L = jpegx.lib()
    keep, p = _aligned()
    err = lambda: L.jpegx_last_error()
    assert L.jpegx_entropy_decode_n(None, 10, 1, 16, p, p, None) == -1 and b"null" in err()
    assert L.jpegx_entropy_decode_n(p, 10, 1, 16, None, p, None) == -1 and b"null" in err()
    assert L.jpegx_entropy_decode_n(p, 10, 1, 16, p, None, None) == -1 and b"null" in err()
    assert L.jpegx_entropy_decode_n(p, 10, 0, 16, p, p, None) == -1 and b"block count" in err()
    assert L.jpegx_entropy_decode_n(p, 10, 1, 0, p, p, None) == -1 and b"1 .. 1024" in err()
    assert L.jpegx_entropy_decode_n(p, 10, 1, 1025, p, p, None) == -1 and b"1 .. 1024" in err()
    assert L.jpegx_entropy_decode_n(p, 10, 1 << 21, 1024, p, p, None) == -1 and b"2^31" in err()
    assert L.jpegx_entropy_decode_n(p, 0, 1, 16, p, p, None) == -1 and b"empty" in err()
    assert L.jpegx_entropy_decode_n(p, (1 << 32) - 4096, 1, 16, p, p, None) == -1 and b"2^32" in err()
    assert L.jpegx_entropy_decode_n(p + 1, 10, 1, 16, p, p, None) == -1 and b"aligned" in err()
    assert L.jpegx_entropy_decode_n(p, 10, 1, 16, p, p + 2, None) == -1 and b"aligned" in err()
    assert L.jpegx_entropy_decode_n(p, 10, 1, 16, p + 4, p, None) == -1 and b"aligned" in err()
    assert L.jpegx_entropy_decode_status_n(None, None) == -1 and b"null" in err()
    assert L.jpegx_entropy_decode_n_on(0, None, 10, 1, 16, p, p, None) != 0
    del keep


def test_workspace_size_is_a_function_of_the_arguments_within_the_bound():
    import jpegx
    L = jpegx.lib()
    for nbytes, nblocks, block_len in [(1, 1, 1), (7, 3, 4), (4096, 130, 16), (95780, 67, 576), (1 << 24, 1 << 16, 1024),
                                       ((1 << 32) - 4097, 1 << 20, 64)]:
        ws = L.jpegx_entropy_decode_workspace_bytes_n(nbytes, nblocks, block_len)
        assert ws == L.jpegx_entropy_decode_workspace_bytes_n(nbytes, nblocks, block_len)
        assert 12 * nbytes + 4 * nblocks <= ws <= 16 * nbytes + 8 * nblocks + 4096 and ws % 16 == 0
    for bad in [(0, 1, 16), (10, 0, 16), (10, 1, 0), (10, 1, 1025), (10, 1 << 21, 1024), ((1 << 32) - 4096, 1, 16)]:
        assert L.jpegx_entropy_decode_workspace_bytes_n(*bad) == 0


def test_host_entries_validate_before_any_device_work():
    import jpegx
    L = jpegx.lib()
    keep, p = _aligned(4096)
    err = lambda: L.jpegx_last_error()
    assert L.jpegx_host_entropy_decode_n_gpu(None, 10, 1, 16, p) == -1 and b"null" in err()
    assert L.jpegx_host_entropy_decode_n_gpu(p, 10, 1, 16, None) == -1 and b"null" in err()
    assert L.jpegx_host_entropy_decode_n_gpu(p, 10, 1, 2000, p) == -1 and b"1 .. 1024" in err()
    assert L.jpegx_host_entropy_decode_n_gpu(p, 0, 1, 16, p) == -1 and b"empty" in err()
    plane = lambda **kw: L.jpegx_host_decompress_plane_n(*[kw.get(k, d) for k, d in (
        ("bytes", p), ("nbytes", 10), ("H", 16), ("W", 16), ("N", 4), ("mode", 0), ("param", 0.0), ("flags", 0), ("out", p), ("pitch", 16))])
    assert plane(bytes=None) == -1 and b"null" in err()
    assert plane(out=None) == -1 and b"null" in err()
    assert plane(N=1) == -1 and b"2 .. 32" in err()
    assert plane(N=33) == -1 and b"2 .. 32" in err()
    assert plane(H=18) == -1 and b"multiples of dct_size" in err()
    assert plane(W=0) == -1 and b"multiples of dct_size" in err()
    assert plane(pitch=15) == -1 and b"pitch" in err()
    assert plane(H=1 << 16, W=1 << 16, pitch=1 << 16) == -1 and b"2^31" in err()
    assert plane(mode=3) == -1 and b"quantisers" in err()                   # qtable needs dct_size 8
    assert plane(mode=2, param=0.0) == -1 and b"divisor" in err()
    assert plane(mode=1, param=-1.0) == -1 and b"keep" in err()
    assert plane(flags=4) == -1 and b"JPEGX_F_CLAMP_U8" in err()
    assert plane(nbytes=0) == -1 and b"empty" in err()
    assert L.jpegx_host_decompress_plane_n_on(0, None, 10, 16, 16, 4, 0, 0.0, 0, p, 16) != 0
    del keep


def test_python_wrappers_refuse_bad_arguments():
    import jpegx
    with pytest.raises(jpegx.JpegxError, match="out must be"):
        jpegx.decompress_plane_n(b"\x00", 4, 4, 4, out="f32")
    with pytest.raises(jpegx.JpegxError, match="2 .. 32"):
        jpegx.decompress_plane_n(b"\x00", 4, 4, 64)
    with pytest.raises(jpegx.JpegxError, match="1 .. 1024"):
        jpegx.entropy_decode_n_gpu(b"\x00", 1, 4096)
    with pytest.raises(jpegx.JpegxError, match="null"):                 # an empty blob has no address
        jpegx.entropy_decode_n_gpu(b"", 1, 16)


def test_no_cpu_fallback_without_a_device():
    import jpegx
    if jpegx.device_count() > 0:
        pytest.skip("a GPU is present; the loud-failure path is covered on the CPU container")
    with pytest.raises(jpegx.JpegxError):
        jpegx.entropy_decode_n_gpu(bytes(4), 4, 16)
    with pytest.raises(jpegx.JpegxError):
        jpegx.decompress_plane_n(bytes(16), 16, 16, 4)


def test_small_planes_keep_the_road_of_before(monkeypatch):
    """Below pipeline.DCTN_ENTROPY_DECODE_MIN_SAMPLES (and below DCTN_MIN_SAMPLES) decompress_band never starts the job."""
    import jpegx
    import pipeline
    gate = pipeline.DCTN_ENTROPY_DECODE_MIN_SAMPLES
    assert gate is None or gate > 240

    def boom(*a, **k):
        raise AssertionError("decompress_band took the device job")
    monkeypatch.setattr(jpegx, "decompress_plane_n", boom)
    cfg = pipeline.Configuration(width=20, height=12, block_size=1, dct_size=4,
                                 quantization=pipeline.QuantizationMethod("divide", divisor=10))
    band = np.random.default_rng(5).integers(0, 256, (12, 20))
    blob = pipeline.compress_band(band, cfg)
    back = pipeline.decompress_band(blob, cfg)
    assert back.shape == (12, 20) and np.array_equal(pipeline.decompress_band_u8(blob, cfg), back.astype(np.uint8))
    for setting in (None, 0):                                           # without a usable device the constant changes nothing
        monkeypatch.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", setting)
        if setting is None or jpegx.device_count() == 0:
            assert np.array_equal(pipeline.decompress_band(blob, cfg), back)
