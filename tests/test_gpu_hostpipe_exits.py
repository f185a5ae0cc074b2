"""GPU: the ways out of the pooled host jobs (csrc/jpegx_hostpipe.cpp).  Every refusal -- before anything is enqueued, in
the middle of a band's work, after a decode that the device turned down -- hands its job context back idle and unlocked:
the calling thread holds none afterwards and the next jobs on it give the golden bytes and bands.  And the host threads
that widen a result to int64 are at least one, whatever JPEGX_WIDEN_THREADS says."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import pipeline
from conftest import PKG
from pipeline import Configuration, QuantizationMethod

pytestmark = pytest.mark.gpu

# 127 single-byte blocks (all coefficients zero) where the 64 x 128 plane has 128: one block short.  (128 zero bytes ARE
# that plane, all zero -- tests/test_gpu_entropy.py decodes 300 of them -- so the stream that is refused is the one a byte
# shorter.)
SHORT = bytes(127)
NOT_BLOCKS = b"well-formed blocks"


def test_every_refusal_gives_the_context_back_idle(gpu, golden):
    L = gpu.lib()
    n = ctypes.c_size_t(0)
    qtable = gpu.mode_of("qtable")

    def refused(rc, code, text):
        msg = L.jpegx_last_error()
        print("refusal: %d %r" % (rc, msg))
        assert rc == code and text in msg, (rc, msg)
        assert L.jpegx_host_pool_release() == 0, L.jpegx_last_error()      # JPEGX_E_INVALID while this thread holds a context

    # a sample outside 8 bits, found while the band's strips are already on their way to the device
    band = np.random.default_rng(2028).integers(0, 256, (20, 28)).astype(np.int64)
    band[11, 17] = 256
    refused(L.jpegx_host_compress_begin_ragged(band.ctypes.data, 8, 20, 28, 28, 1, qtable, 0.0, ctypes.byref(n)), -4, b"0..255")

    # a stream the device decoder turns down, behind the inverse and the copy down that were enqueued with it
    short = np.frombuffer(SHORT, dtype=np.uint8)
    plane = np.empty((64, 128), np.uint8)
    refused(L.jpegx_host_decompress_plane(short.ctypes.data, short.size, 64, 128, 1, qtable, 0.0, plane.ctypes.data, 128), -1, NOT_BLOCKS)
    zz = np.empty((128, 64), np.int16)
    refused(L.jpegx_host_entropy_decode_gpu(short.ctypes.data, short.size, 128, zz.ctypes.data), -1, NOT_BLOCKS)

    # a picture with one good band and one such band: two streams in flight
    noise = golden("noise64")
    good = np.frombuffer(oracle.rle_bytestream(noise["zz_qtable"]), dtype=np.uint8)
    bad = np.frombuffer(bytes(63), dtype=np.uint8)                        # 64 blocks in the plane
    ptrs = (ctypes.c_void_p * 2)(good.ctypes.data, bad.ctypes.data)
    sizes = (ctypes.c_size_t * 2)(good.size, bad.size)
    picture = np.empty((2, 64, 64), np.uint8)
    refused(L.jpegx_host_decompress_image(ptrs, sizes, 2, 64, 64, 1, qtable, 0.0, picture.ctypes.data, 64, 64, 64, 0), -1, NOT_BLOCKS)

    # an amplitude beyond 15 bits (DC = 4e6), known once the sizes have come back from the device
    flat = np.full((16, 16), 1e6)
    refused(L.jpegx_host_compress_begin_n(flat.ctypes.data, 16, 16, 16, 4, gpu.mode_of("none"), 0.0, ctypes.byref(n)), -1, b"BadRleCodeError")

    for name in ("noise64", "ragged20x28"):
        case = golden(name)
        rows, cols = case["input"].shape
        cfg = Configuration(width=cols, height=rows, block_size=int(case["block_size"]), quantization=QuantizationMethod("qtable"))
        blob = pipeline.compress_band(case["input"], cfg)
        assert blob == oracle.rle_bytestream(case["zz_qtable"]), name
        assert np.array_equal(pipeline.decompress_band(blob, cfg), case["band_qtable"]), name


WIDEN_CHILD = """
import sys
import numpy as np
sys.path[:0] = [%r]
import pipeline
cfg = pipeline.Configuration(width=1024, height=1024, block_size=1, quantization=pipeline.QuantizationMethod("qtable"))
np.save(sys.argv[2], pipeline.decompress_band(open(sys.argv[1], "rb").read(), cfg))
""" % PKG


def test_widening_with_a_thread_count_of_zero(gpu, tmp_path, monkeypatch):
    """1024 x 1024 samples is the smallest band whose result is widened by JPEGX_WIDEN_THREADS threads; with 0 of them the
    loop used to start none and hand back the array as np.empty left it."""
    monkeypatch.delenv("JPEGX_WIDEN_THREADS", raising=False)
    band = np.random.default_rng(1024).integers(0, 256, (1024, 1024), dtype=np.uint8)
    cfg = Configuration(width=1024, height=1024, block_size=1, quantization=QuantizationMethod("qtable"))
    blob = pipeline.compress_band(band, cfg)
    want = pipeline.decompress_band(blob, cfg)
    assert want.dtype == np.int64 and np.array_equal(want, pipeline.decompress_band_u8(blob, cfg))      # written, by another road too
    (tmp_path / "blob").write_bytes(blob)
    res = subprocess.run([sys.executable, "-c", WIDEN_CHILD, str(tmp_path / "blob"), str(tmp_path / "band.npy")],
                         env=dict(os.environ, JPEGX_WIDEN_THREADS="0"), capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert np.array_equal(np.load(tmp_path / "band.npy"), want)
