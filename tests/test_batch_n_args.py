"""The batch codec for dct_size != 8: every argument check answers before a device is touched, and the workspace-size
functions are monotone and 0 for what the entries refuse.  CPU only: the pointers are host addresses that a call which
got past its checks would hand to HIP, which on this machine fails with JPEGX_E_HIP (-2) -- never -1 or -4."""
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
    """Arguments every entry admits: 3 planes of 10 x 13 at bs 2, N 4."""
    a = dict(nplanes=3, rows=10, cols=13, pitch=13, bs=2, n=4, mode=Q_NONE, param=0.0, gp=0)
    a.update(over)
    return a


def compress(p, a, ws=True, out=True, bands=True):
    return jpegx.lib().jpegx_batch_compress_n(p if bands else None, a["nplanes"], a["rows"], a["cols"], a["pitch"], a["bs"], a["n"], a["mode"],
                                              a["param"], a["gp"], p if ws else None, p if out else None, 64, None)


def emit(p, a, ws=True, out=True):
    return jpegx.lib().jpegx_batch_emit_n(p if ws else None, a["nplanes"], a["rows"], a["cols"], a["bs"], a["n"], a["gp"], p if out else None, 64, None)


def status(p, a, ws=True, total=True):
    t = ctypes.c_ulonglong(0)
    return jpegx.lib().jpegx_batch_compress_status_n(p if ws else None, a["nplanes"], a["rows"], a["cols"], a["bs"], a["n"], a["gp"],
                                                     ctypes.byref(t) if total else None, None, None)


def decompress(p, a, off=None, null=None):
    if off is None:
        off = np.arange(a["nplanes"] + 1, dtype=np.uint64) * 100
    args = [p, off.ctypes.data, a["nplanes"], a["rows"], a["cols"], a["bs"], a["n"], a["mode"], a["param"], a["gp"], p, p, a.get("opitch", a["cols"]), None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_decompress_n(*args)


def sizes(a, nbytes=1000):
    L = jpegx.lib()
    shape = (a["nplanes"], a["rows"], a["cols"], a["bs"], a["n"])
    return (L.jpegx_batch_workspace_bytes_n(*shape, a["gp"]), L.jpegx_batch_max_bytes_n(*shape),
            L.jpegx_batch_decompress_workspace_bytes_n(nbytes, *shape, a["gp"]))


SHAPE_REFUSALS = [("N 1", dict(n=1), INVALID), ("N 33", dict(n=33), INVALID), ("bs 0", dict(bs=0), UNSUPPORTED), ("bs 256", dict(bs=256), UNSUPPORTED),
                  ("no planes", dict(nplanes=0), INVALID), ("negative planes", dict(nplanes=-1), INVALID), ("no rows", dict(rows=0), INVALID),
                  ("no cols", dict(cols=0, pitch=1), INVALID), ("negative group", dict(gp=-1), INVALID)]


@pytest.mark.parametrize("what,over,code", SHAPE_REFUSALS, ids=[r[0] for r in SHAPE_REFUSALS])
def test_shape_refusals_of_every_entry(mem, what, over, code):
    p, _ = mem
    a = good(**over)
    for call in (compress, emit, status, decompress):
        assert call(p, a) == code, (what, call.__name__, jpegx.lib().jpegx_last_error())
    groups = ctypes.c_int(0)
    off = np.arange(max(a["nplanes"], 0) + 1, dtype=np.uint64)
    assert jpegx.lib().jpegx_batch_groups_n(off.ctypes.data, a["nplanes"], a["rows"], a["cols"], a["bs"], a["n"], a["gp"], None, ctypes.byref(groups)) == code
    assert sizes(a)[:2] == (0, 0) if what != "negative group" else sizes(a)[0] == 0
    assert sizes(a)[2] == 0


def test_the_good_arguments_pass_every_check(mem):
    """The counterpart: with nothing wrong the entries get as far as the device, which this machine has none of (or, on a
    machine with one, would run) -- so the refusals above are the checks', not an accident of the call."""
    p, _ = mem
    a = good()
    assert all(v > 0 for v in sizes(a))
    if jpegx.device_count() > 0:
        return                                            # with a GPU the calls would run on host pointers: the sizes must do
    for call in (compress, emit, status, decompress):
        assert call(p, a) not in (INVALID, UNSUPPORTED), (call.__name__, jpegx.lib().jpegx_last_error())


def test_quantisers(mem):
    p, _ = mem
    for call in (compress, decompress):
        assert call(p, good(mode=Q_QTABLE)) == INVALID and b"qtable" in jpegx.lib().jpegx_last_error()
        assert call(p, good(mode=7)) == INVALID
        assert call(p, good(mode=Q_DIVIDE, param=0.0)) == INVALID
        assert call(p, good(mode=Q_DIVIDE, param=float("inf"))) == INVALID
        assert call(p, good(mode=jpegx.MODE_BY_NAME["discard"], param=1.5)) == INVALID
        assert call(p, good(mode=jpegx.MODE_BY_NAME["discard"], param=-1.0)) == INVALID


def test_null_pointers_and_pitches(mem):
    p, _ = mem
    a = good()
    assert compress(p, a, bands=False) == INVALID and b"null" in jpegx.lib().jpegx_last_error()
    assert compress(p, a, ws=False) == INVALID
    assert emit(p, a, ws=False) == INVALID and emit(p, a, out=False) == INVALID
    assert status(p, a, ws=False) == INVALID and status(p, a, total=False) == INVALID
    for k in (0, 1, 10, 11):
        assert decompress(p, a, null=k) == INVALID and b"null" in jpegx.lib().jpegx_last_error()
    assert compress(p, good(pitch=12)) == INVALID and b"pitch" in jpegx.lib().jpegx_last_error()
    assert decompress(p, good(opitch=12)) == INVALID and b"pitch" in jpegx.lib().jpegx_last_error()
    assert compress(p + 8, a) == INVALID and b"aligned" in jpegx.lib().jpegx_last_error()       # the workspace
    groups = ctypes.c_int(0)
    assert jpegx.lib().jpegx_batch_groups_n(None, 3, 10, 13, 2, 4, 0, None, ctypes.byref(groups)) == INVALID
    off = np.zeros(4, np.uint64)
    assert jpegx.lib().jpegx_batch_groups_n(off.ctypes.data, 3, 10, 13, 2, 4, 0, None, None) == INVALID


def test_offsets_that_decrease_or_cannot_be_the_blocks(mem):
    p, _ = mem
    a = good()                                            # 2 x 2 blocks a plane
    assert decompress(p, a, off=np.array([0, 50, 40, 90], np.uint64)) == INVALID
    assert b"must not decrease" in jpegx.lib().jpegx_last_error()
    assert decompress(p, a, off=np.array([0, 4, 7, 11], np.uint64)) == INVALID       # plane 1: 3 bytes for 4 blocks
    assert b"planes 0..2" in jpegx.lib().jpegx_last_error()
    assert decompress(p, good(gp=1), off=np.array([0, 4, 7, 11], np.uint64)) == INVALID
    assert b"planes 1..1" in jpegx.lib().jpegx_last_error()
    assert decompress(p, good(nplanes=1), off=np.array([5, 5], np.uint64)) == INVALID   # an empty stream
    assert b"cannot be" in jpegx.lib().jpegx_last_error()


def test_the_2_to_31_limits_at_the_last_admitted_and_the_first_refused_value(mem):
    """nplanes * H * W <= 2^31 - 1: 1 x 1 bands at N 3 are planes of 9 samples; and nplanes * rows <= 2^31 - 1."""
    p, _ = mem
    last = (2 ** 31 - 1) // 9
    L = jpegx.lib()
    assert L.jpegx_batch_max_bytes_n(last, 1, 1, 1, 3) == last * ((23 * 9 + 15) // 8) + 64
    assert L.jpegx_batch_workspace_bytes_n(last, 1, 1, 1, 3, 0) > last * 36
    assert L.jpegx_batch_decompress_workspace_bytes_n(1 << 20, last, 1, 1, 1, 3, 0) > 0
    for call in (emit, status):
        assert call(p, good(nplanes=last + 1, rows=1, cols=1, pitch=1, bs=1, n=3)) == INVALID
        assert b"2^31" in L.jpegx_last_error()
    assert compress(p, good(nplanes=last + 1, rows=1, cols=1, pitch=1, bs=1, n=3)) == INVALID
    assert sizes(good(nplanes=last + 1, rows=1, cols=1, pitch=1, bs=1, n=3)) == (0, 0, 0)
    if jpegx.device_count() == 0:
        assert emit(p, good(nplanes=last, rows=1, cols=1, pitch=1, bs=1, n=3)) not in (INVALID, UNSUPPORTED)
    # rows: 2^16 planes of 2^15 rows x 1 column at bs 255 are 2^31 rows but few samples
    tall = dict(rows=1 << 15, cols=1, pitch=1, bs=255, n=2)
    assert sizes(good(nplanes=(1 << 16) - 1, **tall))[0] > 0
    assert sizes(good(nplanes=1 << 16, **tall)) == (0, 0, 0)
    assert compress(p, good(nplanes=1 << 16, **tall)) == INVALID and b"rows" in L.jpegx_last_error()
    # one plane beyond jpegx_band_shape_n's limit
    assert sizes(good(nplanes=1, rows=46341, cols=46341, pitch=46341, bs=1, n=2)) == (0, 0, 0)


def test_the_size_functions_are_monotone():
    """In the plane count and the stream length always; in rows and cols for a given group_planes (with group_planes 0 a
    larger plane can mean fewer planes per group, and so a smaller float64 scratch)."""
    L = jpegx.lib()
    for bs, n, gp in [(1, 4, 0), (5, 24, 0), (2, 16, 3), (3, 7, 1)]:
        prev = (0, 0, 0)
        for nplanes in (1, 2, 3, 64, 65, 4096):
            cur = (L.jpegx_batch_workspace_bytes_n(nplanes, 100, 150, bs, n, gp), L.jpegx_batch_max_bytes_n(nplanes, 100, 150, bs, n),
                   L.jpegx_batch_decompress_workspace_bytes_n(1 << 20, nplanes, 100, 150, bs, n, gp))
            assert all(c >= q > 0 or q == 0 for c, q in zip(cur, prev)) and all(c > 0 for c in cur), (bs, n, gp, nplanes)
            prev = cur
        prev = 0
        for nbytes in (1, 100, 1 << 20, 64 << 20, (64 << 20) + 1, 1 << 30, 1 << 33):
            cur = L.jpegx_batch_decompress_workspace_bytes_n(nbytes, 8, 100, 150, bs, n, gp)
            assert cur >= prev and cur > 0
            prev = cur
        assert L.jpegx_batch_decompress_workspace_bytes_n(0, 8, 100, 150, bs, n, gp) == 0
        if gp:
            prev = (0, 0, 0)
            for rows, cols in [(1, 1), (1, 150), (99, 150), (100, 150), (100, 151), (1000, 1500)]:
                cur = (L.jpegx_batch_workspace_bytes_n(8, rows, cols, bs, n, gp), L.jpegx_batch_max_bytes_n(8, rows, cols, bs, n),
                       L.jpegx_batch_decompress_workspace_bytes_n(1 << 20, 8, rows, cols, bs, n, gp))
                assert all(c >= q for c, q in zip(cur, prev)) and all(c > 0 for c in cur)
                prev = cur


def test_the_workspace_is_4_bytes_a_sample_plus_one_group():
    """Not 12 bytes a sample: 4096 planes of 64 x 64 at N 4 in groups of 16."""
    L = jpegx.lib()
    samples = 4096 * 64 * 64
    ws = L.jpegx_batch_workspace_bytes_n(4096, 64, 64, 1, 4, 16)
    ews = L.jpegx_entropy_workspace_bytes_n(samples // 16, 16)
    assert 4 * samples + 8 * 16 * 64 * 64 + ews <= ws <= 4 * samples + 8 * 16 * 64 * 64 + ews + 8 * 4097 + 2048


def test_the_python_conveniences_refuse_before_a_device_is_needed():
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_n(np.zeros((2, 4, 4), np.uint8), 0, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_n(np.zeros((2, 4, 4), np.uint8), 1, 33)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_compress_n(np.zeros((2, 4, 4), np.float32), 1, 4)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_decompress_n([b"\x00"] * 2, 4, 4, 1, 1)
    with pytest.raises(jpegx.JpegxError):
        jpegx.batch_decompress_n([], 4, 4, 1, 4)
