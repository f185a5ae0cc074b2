"""The batch codec for a set of pictures of unequal sizes, dct_size != 8: every argument check of the entries answers before
a device is touched.  CPU only: the pointers are host addresses that a call which got past its checks would hand to HIP, which
on a machine without a device fails with JPEGX_E_HIP (-2) or JPEGX_E_NODEVICE (-3) -- never -1 or -4."""
import ctypes

import numpy as np
import pytest

import jpegx

INVALID, UNSUPPORTED = -1, -4
Q_NONE, Q_DIVIDE, Q_QTABLE = jpegx.MODE_BY_NAME["none"], jpegx.MODE_BY_NAME["divide"], jpegx.MODE_BY_NAME["qtable"]
SIZES = [(10, 13), (7, 30)]                               # at bs 2, N 4: planes of 8 x 8 and 4 x 16, 4 blocks a band each


@pytest.fixture(scope="module")
def mem():
    buf = ctypes.create_string_buffer(8192)
    return (ctypes.addressof(buf) + 15) & ~15, buf


def table(nbands=3):
    return jpegx.picture_set_table(SIZES, nbands, 2, 4)


def gather(p, t, null=None, p0=0, k=2, colour=0, skew=0, tskew=0, tab=None):
    args = [p, t.ptr if tab is None else tab, p + tskew, p0, k, colour, p + skew, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_picture_set_blocks_n(*args)


def scatter(p, t, null=None, p0=0, k=2, colour=0, tskew=0, tab=None):
    args = [p, t.ptr if tab is None else tab, p + tskew, p0, k, colour, p, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_picture_set_pixels_u8(*args)


def compress(p, t, null=None, colour=0, mode=Q_NONE, param=0.0, gs=0, skew=0, tskew=0, out=True, cap=64, tab=None):
    args = [p, t.ptr if tab is None else tab, p + tskew, colour, mode, param, gs, p + skew, p if out else None, cap, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_compress_picture_set_n(*args)


def emit(p, t, null=None, gs=0, skew=0, tskew=0, tab=None):
    args = [p + skew, t.ptr if tab is None else tab, p + tskew, gs, p, 64, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_emit_set_n(*args)


def status(p, t, null=None, gs=0, tab=None):
    total = ctypes.c_ulonglong(0)
    args = [p, t.ptr if tab is None else tab, gs, ctypes.byref(total), None, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_compress_status_set_n(*args)


def decompress(p, t, off=None, null=None, colour=0, mode=Q_NONE, param=0.0, gs=0, skew=0, tskew=0, tab=None):
    if off is None:
        off = np.arange(t.npictures * t.nbands + 1, dtype=np.uint64) * 100
    args = [p, off.ctypes.data, t.ptr if tab is None else tab, p + tskew, mode, param, colour, gs, p + skew, p, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_decompress_picture_set_n(*args)


def test_null_pointers(mem):
    p, _ = mem
    t, L = table(), jpegx.lib()
    for call, nulls in ((gather, (0, 1, 2, 6)), (scatter, (0, 1, 2, 6)), (compress, (0, 1, 2, 7)), (emit, (0, 1, 2, 4)), (status, (0, 1, 3)),
                        (decompress, (0, 1, 2, 3, 8, 9))):
        for k in nulls:
            assert call(p, t, null=k) == INVALID and b"null" in L.jpegx_last_error(), (call.__name__, k)
    assert L.jpegx_batch_set_workspace_bytes_n(None, 0) == 0 and L.jpegx_batch_set_max_bytes_n(None) == 0
    assert L.jpegx_batch_decompress_set_workspace_bytes_n(100, None, 0) == 0


def test_a_blob_that_is_no_table(mem):
    p, _ = mem
    t, L = table(), jpegx.lib()
    junk = np.zeros(64, np.uint64)
    for call in (gather, scatter, compress, emit, status, decompress):
        assert call(p, t, tab=junk.ctypes.data) == INVALID and b"table" in L.jpegx_last_error(), call.__name__
    assert L.jpegx_batch_set_workspace_bytes_n(junk.ctypes.data, 0) == 0 and L.jpegx_batch_set_max_bytes_n(junk.ctypes.data) == 0
    assert L.jpegx_batch_decompress_set_workspace_bytes_n(100, junk.ctypes.data, 0) == 0


def test_alignment(mem):
    p, _ = mem
    t, L = table(), jpegx.lib()
    assert gather(p, t, skew=8) == INVALID and b"16-byte" in L.jpegx_last_error()           # the strip
    for call in (compress, emit, decompress):
        assert call(p, t, skew=8) == INVALID and b"workspace must be 16-byte aligned" in L.jpegx_last_error(), call.__name__
    for call in (gather, scatter, compress, emit, decompress):
        assert call(p, t, tskew=4) == INVALID and b"d_table" in L.jpegx_last_error(), call.__name__


def test_ranges_of_the_gather_and_the_scatter(mem):
    p, _ = mem
    t, L = table(), jpegx.lib()
    for call in (gather, scatter):
        for p0, k in ((-1, 1), (0, 0), (0, 3), (1, 2), (2, 1), (0, -1), (2 ** 31 - 1, 2)):
            assert call(p, t, p0=p0, k=k) == INVALID and b"pictures" in L.jpegx_last_error(), (call.__name__, p0, k)


def test_colour_and_quantisers(mem):
    p, _ = mem
    L = jpegx.lib()
    for call in (gather, scatter, compress, decompress):
        for t, colour in ((table(), 2), (table(), -1), (table(2), 1), (table(4), 1), (table(1), 1)):
            assert call(p, t, colour=colour) == INVALID and b"colour" in L.jpegx_last_error(), (call.__name__, colour)
    t = table()
    for call in (compress, decompress):
        assert call(p, t, mode=Q_QTABLE) == INVALID and b"qtable" in L.jpegx_last_error()
        assert call(p, t, mode=7) == INVALID
        assert call(p, t, mode=Q_DIVIDE, param=0.0) == INVALID
        assert call(p, t, mode=jpegx.MODE_BY_NAME["discard"], param=1.5) == INVALID


def test_group_samples_and_a_capacity_without_a_destination(mem):
    p, _ = mem
    t, L = table(), jpegx.lib()
    for call in (compress, emit, status, decompress):
        assert call(p, t, gs=-1) == INVALID and b"group_samples" in L.jpegx_last_error(), call.__name__
    assert L.jpegx_batch_set_workspace_bytes_n(t.ptr, -1) == 0 and L.jpegx_batch_decompress_set_workspace_bytes_n(100, t.ptr, -1) == 0
    assert compress(p, t, out=False, cap=64) == INVALID and b"capacity" in L.jpegx_last_error()


def test_offsets_that_decrease_or_cannot_be_the_blocks(mem):
    p, _ = mem
    t, L = table(), jpegx.lib()                           # 12 blocks a picture
    assert decompress(p, t, off=np.array([0, 50, 40, 90, 100, 150, 200], np.uint64)) == INVALID and b"must not decrease" in L.jpegx_last_error()
    assert decompress(p, t, off=np.array([0, 10, 20, 30, 33, 36, 40], np.uint64), gs=1) == INVALID      # picture 1: 10 bytes for 12 blocks
    assert b"pictures 1..1" in L.jpegx_last_error()
    assert decompress(p, t, off=np.array([0, 4, 8, 12, 15, 18, 22], np.uint64)) == INVALID
    assert b"pictures 0..1" in L.jpegx_last_error()


def test_the_good_arguments_pass_every_check_and_the_sizes(mem):
    """The counterpart: with nothing wrong the entries get as far as the device -- so the refusals above are the checks'."""
    p, _ = mem
    L = jpegx.lib()
    for t, colour in ((table(), 0), (table(), 1), (table(1), 0), (table(2), 0), (table(4), 0)):
        blocks = t.total_blocks
        assert blocks == 8 * t.nbands
        assert L.jpegx_batch_set_max_bytes_n(t.ptr) == blocks * ((23 * 16 + 15) // 8) + 64
        ws = L.jpegx_batch_set_workspace_bytes_n(t.ptr, 0)
        assert ws >= blocks * 16 * (4 + 8) + L.jpegx_entropy_workspace_bytes_n(blocks, 16) and ws % 256 == 0
        # one picture a group needs the float64 strip of the larger picture alone
        assert L.jpegx_batch_set_workspace_bytes_n(t.ptr, 1) == ws - 256 * ((blocks * 16 * 8 + 255) // 256) + 256 * ((blocks * 8 * 8 + 255) // 256)
        assert L.jpegx_batch_decompress_set_workspace_bytes_n(1000, t.ptr, 0) > 0
        assert L.jpegx_batch_decompress_set_workspace_bytes_n(0, t.ptr, 0) == 0
        if jpegx.device_count() > 0:
            continue                                      # with a GPU the calls would run on host pointers
        for call in (gather, scatter, compress, decompress):
            assert call(p, t, colour=colour) not in (INVALID, UNSUPPORTED), (call.__name__, L.jpegx_last_error())
        assert compress(p, t, out=False, cap=0) not in (INVALID, UNSUPPORTED)
        assert emit(p, t) not in (INVALID, UNSUPPORTED) and status(p, t) not in (INVALID, UNSUPPORTED)


def test_the_python_conveniences_refuse_before_a_device_is_needed():
    a, b = np.zeros((4, 4, 3), np.uint8), np.zeros((5, 2, 3), np.uint8)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_picture_set_n([a, b], 0, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_picture_set_n([a, b], 1, 33)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_picture_set_n([a, b.astype(np.float32)], 1, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_picture_set_n([a, b[..., :2]], 1, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_picture_set_n([], 1, 4)
    with pytest.raises(jpegx.JpegxError, match="group_samples"):
        jpegx.batch_compress_picture_set_n([a, b], 1, 4, group_samples=-1)
    with pytest.raises(jpegx.JpegxError, match="colour"):
        jpegx.batch_compress_picture_set_n([a, b], 1, 4, colour="bgr")
    with pytest.raises(jpegx.JpegxError, match="three bands"):
        jpegx.batch_compress_picture_set_n([a[..., :2], b[..., :2]], 1, 4, colour="rgb")
    with pytest.raises(jpegx.JpegxError, match="unknown quantiser"):
        jpegx.batch_compress_picture_set_n([a, b], 1, 4, "huffman")
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_decompress_picture_set_n([[b"\x00"] * 3] * 2, [(4, 4), (5, 2)], 1, 1)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_decompress_picture_set_n([], [], 1, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_decompress_picture_set_n([[b"\x00"] * 3, [b"\x00"] * 2], [(4, 4), (5, 2)], 1, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_decompress_picture_set_n([[b"\x00"] * 3] * 2, [(4, 4)], 1, 4)
    with pytest.raises(jpegx.JpegxError, match="group_samples"):
        jpegx.batch_decompress_picture_set_n([[b"\x00"] * 3] * 2, [(4, 4), (5, 2)], 1, 4, group_samples=-2)
