"""The batch codec for whole pictures, dct_size != 8: every argument check of the new entries answers before a device is
touched, the recommended group is what its rule says, and the sizes that are shared with the band batch are the band
batch's at nbands * npictures planes.  CPU only: the pointers are host addresses that a call which got past its checks
would hand to HIP, which on this machine fails with JPEGX_E_HIP (-2) -- never -1 or -4."""
import ctypes

import numpy as np
import pytest

import jpegx

INVALID, UNSUPPORTED = -1, -4
Q_NONE, Q_DIVIDE, Q_QTABLE = jpegx.MODE_BY_NAME["none"], jpegx.MODE_BY_NAME["divide"], jpegx.MODE_BY_NAME["qtable"]


@pytest.fixture(scope="module")
def mem():
    buf = ctypes.create_string_buffer(4096)
    return (ctypes.addressof(buf) + 15) & ~15, buf


def good(**over):
    """Arguments every entry admits: 2 pictures of 3 bands of 10 x 13 at bs 2, N 4, one picture a group."""
    a = dict(npictures=2, nbands=3, rows=10, cols=13, pitch=39, bs=2, n=4, mode=Q_NONE, param=0.0, colour=0, gp=3)
    a.update(over)
    return a


def gather(p, a, pixels=True, out=True, skew=0, opitch=None):
    h, w = 8, 8                                           # of 10 x 13 at bs 2, N 4
    return jpegx.lib().jpegx_band_planes_packed_stacked_n(p if pixels else None, a["npictures"], a["nbands"], a["rows"], a["cols"], a["pitch"],
                                                          a["colour"], a["bs"], a["n"], p + skew if out else None, w if opitch is None else opitch, None)


def scatter(p, a, planes=True, out=True, h=8, pitch=8):
    return jpegx.lib().jpegx_inflate_crop_pack_stacked_u8(p if planes else None, a["npictures"], a["nbands"], h, pitch, a["rows"], a["cols"], a["bs"],
                                                          a["colour"], p if out else None, a["pitch"], None)


def compress(p, a, ws=True, out=True, pixels=True, skew=0):
    return jpegx.lib().jpegx_batch_compress_pictures_n(p if pixels else None, a["npictures"], a["nbands"], a["rows"], a["cols"], a["pitch"], a["colour"],
                                                       a["bs"], a["n"], a["mode"], a["param"], a["gp"], p + skew if ws else None, p if out else None, 64, None)


def decompress(p, a, off=None, null=None, skew=0):
    if off is None:
        off = np.arange(max(a["npictures"] * a["nbands"], 0) + 1, dtype=np.uint64) * 100
    args = [p, off.ctypes.data, a["npictures"], a["nbands"], a["rows"], a["cols"], a["bs"], a["n"], a["mode"], a["param"], a["colour"], a["gp"],
            p + skew, p, a["pitch"], None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_decompress_pictures_n(*args)


def groups(a, off=None):
    if off is None:
        off = np.arange(max(a["npictures"] * a["nbands"], 0) + 1, dtype=np.uint64) * 100
    n = ctypes.c_int(0)
    return jpegx.lib().jpegx_batch_groups_pictures_n(off.ctypes.data, a["npictures"], a["nbands"], a["rows"], a["cols"], a["bs"], a["n"], a["gp"], None,
                                                     ctypes.byref(n))


def dws(a, nbytes=1000):
    return jpegx.lib().jpegx_batch_decompress_pictures_workspace_bytes_n(nbytes, a["npictures"], a["nbands"], a["rows"], a["cols"], a["bs"], a["n"], a["gp"])


REFUSALS = [("no pictures", dict(npictures=0), INVALID), ("negative pictures", dict(npictures=-2), INVALID),
            ("no bands", dict(nbands=0), INVALID), ("five bands", dict(nbands=5, pitch=65, gp=5), INVALID),
            ("bs 0", dict(bs=0), UNSUPPORTED), ("bs 256", dict(bs=256), UNSUPPORTED), ("N 1", dict(n=1), INVALID), ("N 33", dict(n=33), INVALID),
            ("no rows", dict(rows=0), INVALID), ("no cols", dict(cols=0), INVALID),
            ("2^31 samples", dict(npictures=1 << 25), INVALID)]      # 3 * 2^25 planes of 64 samples


@pytest.mark.parametrize("what,over,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_shape_refusals_of_every_entry(mem, what, over, code):
    p, _ = mem
    a = good(**over)
    for call in (gather, scatter, compress, decompress):
        if call is scatter and ("n" in over or what == "2^31 samples"):
            continue                                      # the scatter takes no N, and H in place of H * W
        assert call(p, a) == code, (what, call.__name__, jpegx.lib().jpegx_last_error())
    if a["npictures"] <= 1 << 20:
        assert groups(a) == code
    assert dws(a) == 0


COLOURS = [("colour 1 with two bands", dict(nbands=2, colour=1, gp=2)), ("colour 2", dict(colour=2)), ("colour -1", dict(colour=-1))]


@pytest.mark.parametrize("what,over", COLOURS, ids=[c[0] for c in COLOURS])
def test_colour_refusals(mem, what, over):
    p, _ = mem
    for call in (gather, scatter, compress, decompress):
        assert call(p, good(**over)) == INVALID, (what, call.__name__)
        assert b"colour" in jpegx.lib().jpegx_last_error()


@pytest.mark.parametrize("gp", [0, 4, -3, 1, 2])
def test_group_planes_must_be_a_positive_multiple_of_the_band_count(mem, gp):
    p, _ = mem
    a = good(gp=gp)
    assert compress(p, a) == INVALID and b"group_planes" in jpegx.lib().jpegx_last_error()
    assert decompress(p, a) == INVALID and b"group_planes" in jpegx.lib().jpegx_last_error()
    assert groups(a) == INVALID and b"group_planes" in jpegx.lib().jpegx_last_error()
    assert dws(a) == 0


def test_the_good_arguments_pass_every_check(mem):
    """The counterpart: with nothing wrong the entries get as far as the device, which this machine has none of -- so the
    refusals above are the checks', not an accident of the call."""
    p, _ = mem
    for a in (good(), good(colour=1), good(gp=6), good(gp=300), good(nbands=1, pitch=13, gp=1), good(nbands=4, pitch=52, gp=8)):
        assert dws(a) > 0 and groups(a) == 0
        if jpegx.device_count() > 0:
            continue                                      # with a GPU the calls would run on host pointers
        for call in (gather, scatter, compress, decompress):
            assert call(p, a) not in (INVALID, UNSUPPORTED), (call.__name__, jpegx.lib().jpegx_last_error())


def test_null_pointers_pitches_and_alignment(mem):
    p, _ = mem
    a = good()
    L = jpegx.lib()
    assert gather(p, a, pixels=False) == INVALID and b"null" in L.jpegx_last_error()
    assert gather(p, a, out=False) == INVALID and b"null" in L.jpegx_last_error()
    assert scatter(p, a, planes=False) == INVALID and scatter(p, a, out=False) == INVALID
    assert compress(p, a, pixels=False) == INVALID and b"null" in L.jpegx_last_error()
    assert compress(p, a, ws=False) == INVALID
    for k in (0, 1, 12, 13):
        assert decompress(p, a, null=k) == INVALID and b"null" in L.jpegx_last_error()
    n = ctypes.c_int(0)
    assert L.jpegx_batch_groups_pictures_n(None, 2, 3, 10, 13, 2, 4, 3, None, ctypes.byref(n)) == INVALID
    assert L.jpegx_batch_groups_pictures_n(np.zeros(7, np.uint64).ctypes.data, 2, 3, 10, 13, 2, 4, 3, None, None) == INVALID
    # a pitch below the row: 13 pixels of 3 bytes
    for call in (gather, scatter, compress, decompress):
        assert call(p, good(pitch=38)) == INVALID and b"pitch" in L.jpegx_last_error(), call.__name__
    assert gather(p, a, opitch=7) == INVALID and b"pitch" in L.jpegx_last_error()           # W is 8
    assert scatter(p, a, pitch=6) == INVALID and b"pitch" in L.jpegx_last_error()           # ceil(13 / 2) is 7
    assert scatter(p, a, h=4) == INVALID and b"lower" in L.jpegx_last_error()               # ceil(10 / 2) is 5
    assert gather(p, a, skew=4) == INVALID and b"misaligned" in L.jpegx_last_error()        # the doubles
    assert compress(p, a, skew=8) == INVALID and b"aligned" in L.jpegx_last_error()         # the workspace
    assert decompress(p, a, skew=8) == INVALID and b"aligned" in L.jpegx_last_error()


def test_quantisers(mem):
    p, _ = mem
    for call in (compress, decompress):
        assert call(p, good(mode=Q_QTABLE)) == INVALID and b"qtable" in jpegx.lib().jpegx_last_error()
        assert call(p, good(mode=7)) == INVALID
        assert call(p, good(mode=Q_DIVIDE, param=0.0)) == INVALID
        assert call(p, good(mode=jpegx.MODE_BY_NAME["discard"], param=1.5)) == INVALID


def test_the_2_to_31_limits_at_the_last_admitted_and_the_first_refused_value(mem):
    """npictures * nbands * H * W <= 2^31 - 1: 1 x 1 pictures at N 3 are planes of 9 samples."""
    p, _ = mem
    last = (2 ** 31 - 1) // 27
    tiny = dict(rows=1, cols=1, pitch=3, bs=1, n=3)
    assert dws(good(npictures=last, **tiny), 1 << 20) > 0
    assert dws(good(npictures=last + 1, **tiny), 1 << 20) == 0
    for call in (gather, compress):
        assert call(p, good(npictures=last + 1, **tiny)) == INVALID and b"2^31" in jpegx.lib().jpegx_last_error()
    if jpegx.device_count() == 0:
        assert gather(p, good(npictures=last, **tiny), opitch=3) not in (INVALID, UNSUPPORTED)
    # one band beyond 2^31 - 1 samples before pooling: 65536 x 32768 at bs 255
    assert gather(p, good(rows=65536, cols=32768, pitch=3 * 32768, bs=255, n=2)) == INVALID and b"2^31" in jpegx.lib().jpegx_last_error()
    assert scatter(p, good(rows=65536, cols=32768, pitch=3 * 32768, bs=255, n=2), h=258, pitch=129) == INVALID
    # the rows of the stack
    assert scatter(p, good(npictures=1 << 16, rows=1 << 15, cols=1, pitch=3, bs=255, n=2), h=129, pitch=1) == INVALID
    assert b"rows" in jpegx.lib().jpegx_last_error()


def test_the_recommended_group_on_hand_computed_shapes():
    rec = jpegx.batch_group_planes_pictures_n
    # 64 x 64 at bs 1, N 4: planes of 4096 samples, 2^26 / 4096 = 16384 planes; the multiples of the band count below
    assert rec(3, 64, 64, 1, 4) == 16383
    assert rec(1, 64, 64, 1, 4) == 16384
    assert rec(2, 64, 64, 1, 4) == 16384
    assert rec(4, 64, 64, 1, 4) == 16384
    # 3000 x 4000 at bs 1, N 16: H x W = 3008 x 4000 = 12 032 000 samples, 5 planes within 2^26: one picture of three bands
    assert rec(3, 3000, 4000, 1, 16) == 3
    assert rec(2, 3000, 4000, 1, 16) == 4
    assert rec(1, 3000, 4000, 1, 16) == 5
    # 4096 x 4096 at N 4: 4 planes within 2^26 -- one picture of three or of four bands
    assert rec(3, 4096, 4096, 1, 4) == 3
    assert rec(4, 4096, 4096, 1, 4) == 4
    # 100 x 150 at bs 5, N 24: pooled 20 x 30, planes of 24 x 48 = 1152 samples, 58254 planes
    assert rec(3, 100, 150, 5, 24) == 58254
    assert rec(4, 100, 150, 5, 24) == 58252
    # a picture whose single plane exceeds 2^26 samples (8192 x 8200): the band count
    assert 8192 * 8200 > 1 << 26
    assert rec(3, 8192, 8200, 1, 4) == 3
    assert rec(1, 8192, 8200, 1, 4) == 1
    # bad shapes
    assert rec(0, 64, 64, 1, 4) == 0 and rec(5, 64, 64, 1, 4) == 0
    assert rec(3, 0, 64, 1, 4) == 0 and rec(3, 64, 64, 0, 4) == 0 and rec(3, 64, 64, 1, 33) == 0
    assert rec(3, 46341, 46341, 1, 2) == 0               # one plane beyond 2^31 - 1 samples


def test_the_shared_sizes_are_the_band_batch_at_nbands_times_npictures_planes():
    """The compress workspace, the worst case, status and emit ARE the band functions (no picture entry exists for them); the
    decompress workspace differs from the band function's in the staging area alone: it is never smaller, equal where the
    stream is short, and larger by a lone picture's worst case against a lone plane's where the stream is long."""
    L = jpegx.lib()
    for name in ("jpegx_batch_workspace_bytes_pictures_n", "jpegx_batch_max_bytes_pictures_n", "jpegx_batch_compress_status_pictures_n",
                 "jpegx_batch_emit_pictures_n"):
        assert not hasattr(L, name)
    for nb, k, rows, cols, bs, n, gp in [(3, 5, 40, 56, 1, 4, 6), (3, 7, 100, 150, 5, 24, 3), (4, 2, 64, 64, 1, 16, 8), (1, 9, 33, 17, 2, 3, 2)]:
        band = L.jpegx_batch_decompress_workspace_bytes_n(1000, nb * k, rows, cols, bs, n, gp)
        assert L.jpegx_batch_decompress_pictures_workspace_bytes_n(1000, k, nb, rows, cols, bs, n, gp) == band > 0
        for nbytes in (1 << 20, 65 << 20, 1 << 31):
            band = L.jpegx_batch_decompress_workspace_bytes_n(nbytes, nb * k, rows, cols, bs, n, gp)
            pics = L.jpegx_batch_decompress_pictures_workspace_bytes_n(nbytes, k, nb, rows, cols, bs, n, gp)
            assert pics >= band > 0
    # 2 pictures of 3 planes of 8192 x 8192 at N 32: a lone plane's worst case is 2^26 * 23 / 8 = 184 MiB + the end bytes, above
    # 64 MiB: the stage holds three of them, so the picture workspace is larger by at least two
    band = L.jpegx_batch_decompress_workspace_bytes_n(1 << 31, 6, 8192, 8192, 1, 32, 3)
    pics = L.jpegx_batch_decompress_pictures_workspace_bytes_n(1 << 31, 2, 3, 8192, 8192, 1, 32, 3)
    assert pics - band >= 2 * ((1 << 26) * 23 // 8)


def test_offsets_that_decrease_or_cannot_be_the_blocks(mem):
    p, _ = mem
    a = good()                                            # 2 x 2 blocks a plane, 12 a picture
    assert decompress(p, a, off=np.array([0, 50, 40, 90, 100, 150, 200], np.uint64)) == INVALID
    assert b"must not decrease" in jpegx.lib().jpegx_last_error()
    assert decompress(p, a, off=np.array([0, 10, 20, 30, 33, 36, 40], np.uint64)) == INVALID      # picture 1: 10 bytes for 12 blocks
    assert b"pictures 1..1" in jpegx.lib().jpegx_last_error()
    assert decompress(p, good(gp=6), off=np.array([0, 4, 8, 12, 15, 18, 22], np.uint64)) == INVALID
    assert b"pictures 0..1" in jpegx.lib().jpegx_last_error()


def test_the_python_conveniences_refuse_before_a_device_is_needed():
    px = np.zeros((2, 4, 4, 3), np.uint8)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_pictures_n(px, 0, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_pictures_n(px, 1, 33)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_pictures_n(px.astype(np.float32), 1, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_pictures_n(px[0], 1, 4)
    with pytest.raises(jpegx.JpegxError, match="group_planes"):
        jpegx.batch_compress_pictures_n(px, 1, 4, group_planes=4)
    with pytest.raises(jpegx.JpegxError, match="colour"):
        jpegx.batch_compress_pictures_n(px, 1, 4, colour="bgr")
    with pytest.raises(jpegx.JpegxError, match="three bands"):
        jpegx.batch_compress_pictures_n(px[..., :2], 1, 4, colour="rgb")
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_decompress_pictures_n([[b"\x00"] * 3] * 2, 4, 4, 1, 1)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_decompress_pictures_n([], 4, 4, 1, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_decompress_pictures_n([[b"\x00"] * 3, [b"\x00"] * 2], 4, 4, 1, 4)
    with pytest.raises(jpegx.JpegxError, match="group_planes"):
        jpegx.batch_decompress_pictures_n([[b"\x00"] * 3] * 2, 4, 4, 1, 4, group_planes=5)
