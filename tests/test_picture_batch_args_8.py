"""The batch codec for whole pictures at dct_size 8: every argument check of the new entries (jpegx_picture_planes_stacked_u8,
jpegx_batch_compress_pictures, jpegx_batch_decompress_pictures and their two workspace functions) answers with its code and
text before a device is touched, the workspace functions return 0 for what is refused, and the compress workspace begins
with the band batch's layout.  CPU only: the pointers are host addresses that a call which got past its checks would hand to
HIP, which on a machine without a device fails with JPEGX_E_HIP (-2) -- never -1 or -4."""
import ctypes

import numpy as np
import pytest

import jpegx

INVALID, UNSUPPORTED = -1, -4
Q = jpegx.MODE_BY_NAME


@pytest.fixture(scope="module")
def mem():
    buf = ctypes.create_string_buffer(8192)
    return (ctypes.addressof(buf) + 255) & ~255, buf


def good(**over):
    """Arguments every entry admits: 2 pictures of 3 bands of 10 x 13 at bs 2 (planes of 8 x 8, raw 16 x 16), one picture a group."""
    a = dict(npictures=2, nbands=3, rows=10, cols=13, pitch=39, bs=2, mode=Q["qtable"], param=0.0, colour=0, gp=3, opitch=16)
    a.update(over)
    return a


def err():
    return jpegx.lib().jpegx_last_error()


def gather(p, a, pixels=True, out=True, skew=0):
    return jpegx.lib().jpegx_picture_planes_stacked_u8(p if pixels else None, a["npictures"], a["nbands"], a["rows"], a["cols"], a["pitch"], a["colour"],
                                                       a["bs"], p + skew if out else None, a["opitch"], None)


def compress(p, a, ws=True, pixels=True, skew=0):
    return jpegx.lib().jpegx_batch_compress_pictures(p if pixels else None, a["npictures"], a["nbands"], a["rows"], a["cols"], a["pitch"], a["colour"],
                                                     a["bs"], a["mode"], a["param"], a["gp"], p + skew if ws else None, p, 64, None)


def decompress(p, a, off=None, null=None, skew=0):
    if off is None:
        off = np.arange(max(a["npictures"] * a["nbands"], 0) + 1, dtype=np.uint64) * 100
    args = [p, off.ctypes.data, a["npictures"], a["nbands"], a["rows"], a["cols"], a["bs"], a["mode"], a["param"], a["colour"], p + skew, p, a["pitch"],
            None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_decompress_pictures(*args)


def cws(a):
    return jpegx.lib().jpegx_batch_pictures_workspace_bytes(a["npictures"], a["nbands"], a["rows"], a["cols"], a["bs"], a["gp"])


def dws(a, nbytes=1000):
    return jpegx.lib().jpegx_batch_decompress_pictures_workspace_bytes(nbytes, a["npictures"], a["nbands"], a["rows"], a["cols"], a["bs"])


REFUSALS = [("no pictures", dict(npictures=0), INVALID, b"picture count"), ("negative pictures", dict(npictures=-2), INVALID, b"picture count"),
            ("no bands", dict(nbands=0), INVALID, b"bands"), ("five bands", dict(nbands=5, pitch=65, gp=5), INVALID, b"bands"),
            ("bs 0", dict(bs=0), UNSUPPORTED, b"block_size must be in 1..255"), ("bs 256", dict(bs=256), UNSUPPORTED, b"block_size must be in 1..255"),
            ("no rows", dict(rows=0), INVALID, b"rows and cols"), ("no cols", dict(cols=0), INVALID, b"rows and cols"),
            ("2^31 rows in the stack", dict(npictures=1 << 28), INVALID, b"2^31")]


@pytest.mark.parametrize("what,over,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_shape_refusals_of_every_entry(mem, what, over, code, text):
    p, _ = mem
    a = good(**over)
    for call in (gather, compress, decompress):
        assert call(p, a) == code, (what, call.__name__, err())
        assert text in err(), (what, call.__name__, err())
    assert cws(a) == 0 and dws(a) == 0


def test_the_block_and_row_limits_of_the_band_batch(mem):
    """What jpegx_batch_compress refuses for sizes, with its code: more than 2^31 - 64 blocks in one batch, more than 2^31 - 1
    rows in the stack of raw planes."""
    p, _ = mem
    a = good(npictures=1 << 27, nbands=4, pitch=128, gp=4, rows=32, cols=32)      # 2^29 planes of 4 blocks
    assert compress(p, a) == INVALID and b"2^31 - 64 blocks" in err()
    assert cws(a) == 0 and dws(a) == 0
    a = good(npictures=1000000, rows=2000, cols=1, pitch=3, bs=255)                # 3 000 000 planes of 2040 raw rows
    assert compress(p, a) == INVALID and b"rows" in err()
    assert gather(p, a) == INVALID and b"rows" in err()
    assert cws(a) == 0 and dws(a) == 0
    a = good(rows=50000, cols=50000, pitch=150000, bs=1)                           # 2.5e9 samples in one band
    assert compress(p, a) == INVALID and decompress(p, a) == INVALID and b"samples in one band" in err()
    a = good(npictures=1, rows=4096, cols=4104, pitch=12312, bs=1, gp=3 * 600)      # float64 road (W = 4104): a group is what the batch holds ...
    assert cws(a) > 0
    a = good(npictures=600, rows=4096, cols=4104, pitch=12312, bs=1, gp=3 * 600)    # ... and 1800 planes of 16.8 M samples are no group
    assert compress(p, a) == INVALID and b"group" in err() and cws(a) == 0


COLOURS = [("colour 1 with two bands", dict(nbands=2, pitch=26, colour=1, gp=2)), ("colour 2", dict(colour=2)), ("colour -1", dict(colour=-1))]


@pytest.mark.parametrize("what,over", COLOURS, ids=[c[0] for c in COLOURS])
def test_colour_refusals(mem, what, over):
    p, _ = mem
    for call in (gather, compress, decompress):
        assert call(p, good(**over)) == INVALID, (what, call.__name__)
        assert b"colour" in err()


@pytest.mark.parametrize("gp", [0, 4, -3, 1, 2])
def test_group_planes_must_be_a_positive_multiple_of_the_band_count(mem, gp):
    p, _ = mem
    for a in (good(gp=gp), good(gp=gp, bs=3, opitch=32)):                           # on both roads
        assert compress(p, a) == INVALID and b"group_planes" in err()
        assert cws(a) == 0


QUANTISERS = [("unknown mode", 9, 0.0, INVALID, b"unknown quantiser mode"), ("negative mode", -1, 0.0, INVALID, b"unknown quantiser mode"),
              ("keep -1", Q["discard"], -1.0, INVALID, b"keep must be a non-negative integer"),
              ("keep 2.5", Q["discard"], 2.5, INVALID, b"keep must be a non-negative integer"),
              ("divisor 0", Q["divide"], 0.0, INVALID, b"divisor must be finite and non-zero"),
              ("divisor inf", Q["divide"], float("inf"), INVALID, b"divisor must be finite and non-zero"),
              ("divisor nan", Q["divide"], float("nan"), INVALID, b"divisor must be finite and non-zero"),
              ("divisor 0.4", Q["divide"], 0.4, UNSUPPORTED, b"divisor below 0.5"), ("divisor -0.25", Q["divide"], -0.25, UNSUPPORTED, b"divisor below 0.5")]


@pytest.mark.parametrize("what,mode,param,code,text", QUANTISERS, ids=[q[0] for q in QUANTISERS])
def test_quantiser_refusals_on_both_roads(mem, what, mode, param, code, text):
    """What jpegx_batch_compress refuses, with its code, before any launch -- on the float64 road too, where the first group's
    gather would otherwise have run by the time the forward entry looks at the quantiser."""
    p, _ = mem
    for a in (good(mode=mode, param=param), good(mode=mode, param=param, bs=3, opitch=32), good(mode=mode, param=param, bs=1, rows=8, cols=8, pitch=24)):
        assert compress(p, a) == code, (what, err())
        assert text in err()
    if mode in (9, -1):
        assert decompress(p, good(mode=mode)) == INVALID and b"unknown quantiser mode" in err()


def test_null_pointers_pitches_and_alignment(mem):
    p, _ = mem
    a = good()
    assert gather(p, a, pixels=False) == INVALID and b"null" in err()
    assert gather(p, a, out=False) == INVALID and b"null" in err()
    assert compress(p, a, pixels=False) == INVALID and b"null" in err()
    assert compress(p, a, ws=False) == INVALID and b"null" in err()
    for k in (0, 1, 10, 11):
        assert decompress(p, a, null=k) == INVALID and b"null" in err()
    for call in (gather, compress, decompress):
        assert call(p, good(pitch=38)) == INVALID and b"pitch" in err(), call.__name__
    # the gather's planes: a pitch of at least W * bs that is a multiple of 16, a base that is 16-byte aligned
    for opitch in (15, 8, 17, 24):
        assert gather(p, good(opitch=opitch)) == INVALID and b"multiple of 16" in err(), opitch
    for skew in (1, 4, 8):
        assert gather(p, a, skew=skew) == INVALID and b"16-byte aligned" in err()
        assert compress(p, a, skew=skew) == INVALID and b"16-byte aligned" in err()
    assert decompress(p, a, skew=16) == INVALID and b"256-byte aligned" in err()


def test_decompress_refuses_offsets_before_any_device_work(mem):
    p, _ = mem
    a = good()
    off = np.arange(7, dtype=np.uint64) * 100
    off[3] = 150
    assert decompress(p, a, off=off) == INVALID and b"must not decrease" in err()
    assert decompress(p, a, off=np.zeros(7, np.uint64)) == INVALID and b"empty stream" in err()
    off = np.zeros(7, np.uint64)
    off[6] = 5                                                                   # six planes of one block cannot be five bytes
    assert decompress(p, a, off=off) == INVALID and b"cannot be their" in err()
    assert dws(a, 0) == 0 and dws(a) > 0


def test_the_good_arguments_pass_every_check(mem):
    """The counterpart: with nothing wrong the entries get as far as the device, which a CPU machine has none of -- so the
    refusals above are the checks', not an accident of the call."""
    p, _ = mem
    for a in (good(), good(colour=1), good(gp=6), good(gp=300), good(nbands=1, pitch=13, gp=1), good(nbands=4, pitch=52, gp=8),
              good(bs=3, opitch=32), good(bs=1, opitch=16), good(bs=255, opitch=8 * 255 + 8), good(mode=Q["divide"], param=0.5)):
        assert cws(a) > 0 and dws(a) > 0
        if jpegx.device_count() > 0:
            continue                                      # with a GPU the calls would run on host pointers
        for call in (gather, compress, decompress):
            assert call(p, a) not in (INVALID, UNSUPPORTED), (call.__name__, err())


ROADS = [(10, 13, 2, 3), (10, 13, 3, 3), (8, 8, 1, 3), (8, 16, 1, 6), (37, 53, 2, 3), (9, 130, 4, 3), (44, 70, 3, 6), (23, 41, 5, 3), (20, 20, 7, 9)]


@pytest.mark.parametrize("rows,cols,bs,gp", ROADS, ids=["%dx%d-bs%d-g%d" % r for r in ROADS])
def test_the_workspace_begins_with_the_band_batch_s_layout(rows, cols, bs, gp):
    """jpegx_batch_pictures_workspace_bytes = jpegx_batch_workspace_bytes(nbands * npictures, H, W) -- the part that
    jpegx_batch_compress_status and jpegx_batch_emit address -- plus the front end's scratch, rounded up to 256 bytes: the
    raw planes of the whole stack on the uint8 road, float64 planes of one group on the other."""
    k, nb = 5, 3
    h, w = jpegx.padded_shape(rows, cols, bs)
    inner = jpegx.batch_workspace_bytes(k * nb, h, w)
    assert inner > 0 and inner % 256 == 0
    u8 = bs in (1, 2, 4) and (w * bs) % 16 == 0
    front = k * nb * h * bs * w * bs if u8 else min(gp, k * nb) * h * w * 8
    assert jpegx.batch_pictures_workspace_bytes(k, nb, rows, cols, bs, gp) == inner + (front + 255) // 256 * 256
    # the way back: the band batch's workspace, then nplanes pooled planes
    inner = jpegx.batch_decompress_workspace_bytes(5000, k * nb, h, w)
    assert inner > 0
    assert jpegx.batch_decompress_pictures_workspace_bytes(5000, k, nb, rows, cols, bs) == (inner + 255) // 256 * 256 + (k * nb * h * w + 255) // 256 * 256


def test_python_conveniences_name_the_refusal_without_a_device():
    px = np.zeros((2, 10, 13, 3), np.uint8)
    with pytest.raises(jpegx.JpegxError, match="group_planes"):
        jpegx.batch_compress_pictures(px, 2, group_planes=4)
    with pytest.raises(jpegx.JpegxError, match="block_size must be in 1..255"):
        jpegx.batch_compress_pictures(px, 256)
    with pytest.raises(jpegx.JpegxError, match="colour"):
        jpegx.batch_compress_pictures(px, 2, colour="bgr")
    with pytest.raises(jpegx.JpegxError, match="three bands|colour"):
        jpegx.batch_compress_pictures(px[..., :2], 2, colour="rgb")
    with pytest.raises(jpegx.JpegxError, match="uint8 pictures"):
        jpegx.batch_compress_pictures(px[0], 2)
    with pytest.raises(jpegx.JpegxError, match="same number of bands"):
        jpegx.batch_decompress_pictures([[b"a", b"b"], [b"c"]], 10, 13, 2)
    with pytest.raises(jpegx.JpegxError, match="empty stream"):
        jpegx.batch_decompress_pictures([[b"", b"", b""]], 10, 13, 2)
    with pytest.raises(jpegx.JpegxError, match="block_size must be in 1..255"):
        jpegx.batch_decompress_pictures([[b"a", b"b", b"c"]], 10, 13, 0)
