"""CPU: the geometry of the fused edge padding -- the new C entries are declared and exported, jpegx_padded_shape is the
geometry of the oracle, and jpegx.edge_source_indices (the written specification of the margin-fill kernel,
csrc/jpegx_pad.hip) turns a band of any shape into a plane whose tile means are what the reference pools and pads:
edge_pad(block_size) -> mean -> edge_pad(8), codec_oracle.pre_transform.  Every comparison is exact."""
import ctypes
import glob
import os

import numpy as np
import pytest

from codec_oracle import blocks_of, pre_transform
from conftest import GOLDEN, REPO

NEW_ENTRIES = ["jpegx_padded_shape", "jpegx_pad_edges", "jpegx_host_compress_begin_ragged",
               "jpegx_host_compress_image_ragged", "jpegx_host_compress_image_packed_ragged"]
ON_FORMS = [n + "_on" for n in NEW_ENTRIES[1:]]          # jpegx_padded_shape is host arithmetic: it has no device to name
BLOCK_SIZES = [1, 2, 3, 4, 5, 7, 16]
SHAPES = [(1, 17), (37, 53), (23, 41), (9, 130), (7, 300), (29, 1), (1080, 1920), (50, 50), (8, 8), (33, 64)]


def test_new_entries_are_declared_exported_and_bound():
    import jpegx
    header = open(os.path.join(REPO, "include", "jpegx.h")).read()
    lib = ctypes.CDLL(jpegx.LIB_PATH)
    for name in NEW_ENTRIES + ON_FORMS:
        assert "int %s(" % name in header, name
        assert hasattr(lib, name), "libjpegx.so does not export %s" % name
        assert name in jpegx.SIGNATURES, name
    for name in ("padded_shape", "pad_edges", "edge_source_indices"):
        assert callable(getattr(jpegx, name)), name
    import inspect
    for name in ("compress_plane_native", "compress_image_native", "compress_image_packed"):
        assert "ragged" in inspect.signature(getattr(jpegx, name)).parameters, name


def test_padded_shape_is_the_oracles_geometry():
    """The C function itself (host arithmetic, no device): rows, cols in 1..70, eight block sizes."""
    import jpegx
    for bs in BLOCK_SIZES + [255]:
        for rows in range(1, 71):
            for cols in range(1, 71):
                hb, wb = blocks_of(rows, cols, bs)
                assert jpegx.padded_shape(rows, cols, bs) == (hb * 8, wb * 8), (rows, cols, bs)


def test_padded_shape_refuses_bad_arguments():
    import jpegx
    L = jpegx.lib()
    h, w = ctypes.c_int(0), ctypes.c_int(0)
    for rows, cols, bs in [(0, 5, 1), (5, 0, 1), (-1, 5, 2), (5, 5, 0), (5, 5, 256), (2 ** 31 - 1, 8, 1)]:
        assert L.jpegx_padded_shape(rows, cols, bs, ctypes.byref(h), ctypes.byref(w)) == -1, (rows, cols, bs)
    assert L.jpegx_padded_shape(5, 5, 1, None, ctypes.byref(w)) == -1
    # validation of the enqueue entry happens before any device work
    assert L.jpegx_pad_edges(None, 1, 1, 5, 5, 1, 8, None) == -1
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    assert L.jpegx_pad_edges(p, 2, 1, 5, 5, 1, 8, None) == -4           # element size
    assert L.jpegx_pad_edges(p, 1, 0, 5, 5, 1, 8, None) == -1           # no planes
    assert L.jpegx_pad_edges(p, 1, 1, 5, 5, 1, 7, None) == -1           # pitch below the padded row
    assert L.jpegx_pad_edges(p, 1, 1, 8, 16, 1, 16, None) == 0          # no margin: JPEGX_OK without a launch, even without a device


def gathered_means(band, bs):
    """The padded raw plane as the kernel builds it, then the exact bs x bs tile means."""
    import jpegx
    band = np.asarray(band)
    sy, sx = jpegx.edge_source_indices(band.shape[0], bs), jpegx.edge_source_indices(band.shape[1], bs)
    padded = band[sy][:, sx].astype(np.int64)
    hh, ww = padded.shape
    hb, wb = blocks_of(band.shape[0], band.shape[1], bs)
    assert (hh, ww) == (hb * 8 * bs, wb * 8 * bs)
    assert np.array_equal(padded[:band.shape[0], :band.shape[1]], band)         # the identity inside the band
    assert sy.max() < band.shape[0] and sx.max() < band.shape[1] and sy.min() >= 0 and sx.min() >= 0
    sums = padded.reshape(hh // bs, bs, ww // bs, bs).sum(axis=(1, 3))
    return sums / float(bs * bs)                                                  # one division of the exact sum, like np.mean


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_edge_source_indices_reproduce_pre_transform(bs):
    for k, (rows, cols) in enumerate(SHAPES):
        rng = np.random.default_rng(1000 * bs + k)
        band = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
        assert np.array_equal(gathered_means(band, bs), pre_transform(band, bs)), (rows, cols, bs)


def test_edge_source_indices_on_the_golden_ragged_bands():
    files = sorted(glob.glob(os.path.join(GOLDEN, "case_ragged*.npz")))
    assert len(files) >= 9
    for f in files:
        case = np.load(f)
        band, bs = case["input"], int(case["block_size"])
        got = gathered_means(band, bs)
        assert np.array_equal(got, pre_transform(band, bs)), f
        assert np.array_equal(got, case["pre"]), f
