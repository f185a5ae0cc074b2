"""The six entries of the dct_size-8 probes (jpegx_probe_sizes_8, jpegx_probe_distortion_8, jpegx_batch_probe_pictures,
jpegx_batch_probe_distortion_pictures and the two _workspace_bytes functions): every bad argument is refused before a device is
needed, with its code and a message that names the entry and the argument; the workspace functions are pinned to their
documented formula; jpegx_padded_shape and jpegx_band_shape_n(..., 8) agree; the Python wrappers refuse as the entries do.
CPU only."""
import ctypes

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -4
NONE, DISCARD, DIVIDE, QTABLE = 0, 1, 2, 3


def _aligned(nbytes=4096):
    buf = ctypes.create_string_buffer(nbytes + 256)
    return buf, (ctypes.addressof(buf) + 255) & ~255


class Calls:
    """The four compute entries with one valid-looking argument list each; a call replaces arguments by name.  Nothing here may
    reach a device: every call below is refused first (a reached device would answer JPEGX_E_NODEVICE or JPEGX_E_HIP, never
    JPEGX_E_INVALID)."""

    def __init__(self, jpegx, on=False):
        self.L = jpegx.lib()
        self.keep, self.p = _aligned()
        self.on = on

    def _call(self, name, order, kw):
        names = [k for k, _ in order]
        unknown = set(kw) - set(names)
        assert not unknown, unknown
        args = [kw.get(k, d) for k, d in order]
        params = args[names.index("params")]
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            args[names.index("params")] = params.ctypes.data
            if "K" not in kw:
                args[names.index("K")] = params.size
        fn = getattr(self.L, name + ("_on" if self.on else ""))
        return fn(0, *args) if self.on else fn(*args)

    def sizes(self, **kw):
        return self._call("jpegx_probe_sizes_8",
                          (("planes", self.p), ("nplanes", 3), ("H", 8), ("W", 16), ("pitch", 16), ("mode", DIVIDE), ("params", [40.0]), ("K", 1),
                           ("totals", self.p), ("stream", None)), kw)

    def distortion(self, **kw):
        # a 20 x 37 band pooled 3 x 3 is 7 x 13 samples: planes of 8 x 16
        return self._call("jpegx_probe_distortion_8",
                          (("planes", self.p), ("moments", self.p), ("nplanes", 3), ("H", 8), ("W", 16), ("pitch", 16), ("mpitch", 16), ("bs", 3),
                           ("rows", 20), ("cols", 37), ("mode", DIVIDE), ("params", [40.0]), ("K", 1), ("totals", self.p), ("stream", None)), kw)

    def _batch(self, name, kw):
        return self._call(name, (("pixels", self.p), ("npictures", 2), ("nbands", 3), ("rows", 20), ("cols", 37), ("pitch", 111), ("colour", 0),
                                 ("bs", 3), ("mode", DIVIDE), ("params", [40.0]), ("K", 1), ("group_planes", 3), ("ws", self.p),
                                 ("totals", self.p), ("stream", None)), kw)

    def batch(self, **kw):
        return self._batch("jpegx_batch_probe_pictures", kw)

    def batch_distortion(self, **kw):
        return self._batch("jpegx_batch_probe_distortion_pictures", kw)

    def err(self):
        return self.L.jpegx_last_error()


NAMES = {"sizes": b"probe_sizes_8: ", "distortion": b"probe_distortion_8: ", "batch": b"batch_probe_pictures: ",
         "batch_distortion": b"batch_probe_distortion_pictures: "}


def _refusals(c):
    for which, who in NAMES.items():
        entry = getattr(c, which)
        # the candidate count
        for k in (0, 33, -1):
            assert entry(params=[40.0] * 33, K=k) == INVALID and who + b"K must be 1 .. JPEGX_PROBE_MAX_CANDIDATES (32)" == c.err(), (which, k)
        # the quantiser: all four modes pass the check (the call then ends at the device, never at INVALID with a mode message)
        assert entry(mode=7) == INVALID and who + b"mode: unknown quantiser mode" == c.err()
        assert entry(mode=-1) == INVALID and b"unknown quantiser mode" in c.err()
        for mode in (NONE, QTABLE):
            assert entry(mode=mode, params=[0.0, 0.0]) == INVALID, mode
            assert who + b"K must be 1 for the quantisers 'none' and 'qtable', which have no parameter" == c.err(), mode
        assert entry(params=None, K=1) == INVALID and who + b"h_params: null pointer" == c.err()
        for bad in (0.0, float("nan"), float("inf"), float("-inf")):
            assert entry(params=[40.0, bad, 8.0]) == INVALID, bad
            assert who + b"h_params[1]: divide: divisor must be finite and non-zero" == c.err(), bad
        for bad in (2.5, -1.0, float("nan")):
            assert entry(mode=DISCARD, params=[0.0, 1.0, bad]) == INVALID, bad
            assert who + b"h_params[2]: discard: keep must be a non-negative integer" == c.err(), bad
    # null pointers
    for name in ("planes", "totals"):
        assert c.sizes(**{name: None}) == INVALID and c.err() == b"probe_sizes_8: d_planes / d_totals: null device pointer", name
    for name in ("planes", "moments", "totals"):
        assert c.distortion(**{name: None}) == INVALID and c.err() == b"probe_distortion_8: d_planes / d_moments / d_totals: null device pointer"
    for which in ("batch", "batch_distortion"):
        for name in ("pixels", "ws", "totals"):
            assert getattr(c, which)(**{name: None}) == INVALID, (which, name)
            assert c.err() == NAMES[which] + b"d_pixels / d_workspace / d_totals: null device pointer"
    # shapes of the plane entries
    for which in ("sizes", "distortion"):
        entry, who = getattr(c, which), NAMES[which]
        assert entry(nplanes=0) == INVALID and c.err() == who + b"nplanes: the plane count must be positive"
        for change in (dict(H=12), dict(W=20, pitch=20), dict(H=0), dict(W=-8)):
            assert entry(**change) == INVALID and c.err() == who + b"H, W: plane height and width must be positive multiples of 8", change
        assert entry(pitch=15) == INVALID and c.err() == who + b"pitch smaller than width"
        assert entry(planes=c.p + 4) == INVALID and b"must be 8-byte aligned" in c.err() and who in c.err()
        assert entry(totals=c.p + 2) == INVALID and b"must be 8-byte aligned" in c.err()
    assert c.sizes(nplanes=2, H=32768, W=32768, pitch=32768) == INVALID and b"2^31 or more coefficients" in c.err()
    assert c.distortion(mpitch=15) == INVALID and c.err() == b"probe_distortion_8: mpitch smaller than width"
    assert c.distortion(moments=c.p + 4) == INVALID and b"must be 8-byte aligned" in c.err()
    for bs in (0, 256, -1):
        assert c.distortion(bs=bs) == INVALID and c.err() == b"probe_distortion_8: bs: block_size must be in 1..255", bs
    # rows and cols must give H and W: 25 rows pool to 9 samples, planes of 16 rows; 49 columns pool to 17, planes of 24
    for change in (dict(rows=25), dict(cols=49), dict(rows=0), dict(cols=-1), dict(bs=2), dict(H=16), dict(W=24, pitch=24, mpitch=24)):
        assert c.distortion(**change) == INVALID and c.err() == b"probe_distortion_8: rows, cols: they must give H, W by jpegx_padded_shape", change
    # the batch entries: the shape and limits of jpegx_batch_compress_pictures, under their own names
    for which in ("batch", "batch_distortion"):
        entry, who = getattr(c, which), NAMES[which]
        assert entry(npictures=0) == INVALID and c.err() == who + b"the picture count must be positive"
        assert entry(pitch=110) == INVALID and c.err() == who + b"pitch smaller than the row"
        for gp in (0, -3, 2, 4):
            assert entry(group_planes=gp) == INVALID and who + b"group_planes must be a positive multiple of the band count" in c.err(), gp
        assert entry(nbands=3, colour=2) == INVALID and who + b"colour must be 0" in c.err()
        assert entry(nbands=1, colour=1, pitch=37, group_planes=1) == INVALID and b"colour" in c.err()
        assert entry(nbands=0) == INVALID and b"bands" in c.err()
        assert entry(nbands=5, pitch=185, group_planes=5) == INVALID and b"bands" in c.err()
        assert entry(bs=0) == UNSUPPORTED and entry(bs=256) == UNSUPPORTED and who + b"block_size must be in 1..255" == c.err()
        assert entry(rows=0) == INVALID and entry(cols=0) == INVALID and who + b"rows and cols must be at least 1" == c.err()
        assert entry(ws=c.p + 8) == INVALID and c.err() == who + b"d_workspace must be 16-byte aligned"
        assert entry(totals=c.p + 4) == INVALID and c.err() == who + b"d_totals must be 8-byte aligned"
        # the batch may hold more than 2^31 coefficients (its limit is in blocks), ONE group of planes may not: the probes
        # are on the float64 road whatever block_size
        assert entry(npictures=2, rows=32768, cols=32768, pitch=3 * 32768, bs=1, group_planes=9) == INVALID
        assert c.err() == who + b"more than 2^31 - 1 samples in one group of planes"
        assert entry(npictures=1 << 20, rows=2048, cols=2048, pitch=3 * 2048, bs=1) == INVALID and b"2^31" in c.err()


def test_every_refusal_names_its_argument():
    import jpegx
    _refusals(Calls(jpegx))


def test_the_explicit_device_forms_exist_and_are_bound():
    import jpegx
    for name in ("jpegx_probe_sizes_8", "jpegx_probe_distortion_8", "jpegx_batch_probe_pictures", "jpegx_batch_probe_distortion_pictures"):
        assert jpegx.SIGNATURES[name + "_on"] == [ctypes.c_int] + jpegx.SIGNATURES[name]
        assert hasattr(jpegx.lib(), name + "_on")
    if jpegx.device_count() > 0:                       # the forms make the device current first: they need one
        _refusals(Calls(jpegx, on=True))


def test_a_valid_call_is_not_refused_by_the_checks():
    """The argument lists above pass every check, under all four quantisers: without a device the answer is 'no device' or a HIP
    failure, never INVALID; with one they are not sent (the pointers are host memory)."""
    import jpegx
    if jpegx.device_count() > 0:
        return
    c = Calls(jpegx)
    for entry in (c.sizes, c.distortion, c.batch, c.batch_distortion):
        assert entry() not in (0, INVALID, UNSUPPORTED)
        assert entry(mode=DISCARD, params=[0.0, 2.0, 8.0]) not in (0, INVALID, UNSUPPORTED)
        for mode in (NONE, QTABLE):                    # no parameter: h_params is not read
            assert entry(mode=mode, params=None, K=1) not in (0, INVALID, UNSUPPORTED), mode


def test_the_n_road_message_for_qtable_stays():
    import jpegx
    L = jpegx.lib()
    _, p = _aligned()
    params = np.array([40.0])
    assert L.jpegx_probe_sizes_n(p, 1, 4, 4, 4, 4, QTABLE, params.ctypes.data, 1, p, None) == INVALID
    assert L.jpegx_last_error() == b"qtable: the luminance table is 8 x 8, it needs dct_size 8 (BadQuantizationError)"


def test_padded_shape_is_band_shape_at_8():
    """The batch entries take their planes' shape from jpegx_padded_shape and their gathers run at N = 8."""
    import jpegx
    for bs in range(1, 6):
        for rows in range(1, 71):
            for cols in range(1, 71):
                assert jpegx.padded_shape(rows, cols, bs) == jpegx.band_shape_n(rows, cols, bs, 8), (rows, cols, bs)


def test_workspace_formula():
    import jpegx

    def up256(v):
        return (v + 255) // 256 * 256
    for npictures, nbands, rows, cols, bs, gp in ((2, 3, 20, 37, 3, 3), (5, 3, 37, 53, 1, 6), (5, 3, 64, 64, 4, 300), (7, 1, 100, 9, 2, 2)):
        h, w = jpegx.padded_shape(rows, cols, bs)
        one = up256(min(gp, npictures * nbands) * h * w * 8)
        assert jpegx.batch_probe_pictures_workspace_bytes(npictures, nbands, rows, cols, bs, gp) == one
        assert jpegx.batch_probe_distortion_pictures_workspace_bytes(npictures, nbands, rows, cols, bs, gp) == 2 * one
    for bad in ((0, 3, 20, 37, 3, 3), (2, 3, 20, 37, 3, 4), (2, 3, 20, 37, 0, 3), (2, 3, 0, 37, 3, 3), (2, 9, 20, 37, 3, 9)):
        assert jpegx.batch_probe_pictures_workspace_bytes(*bad) == 0, bad
        assert jpegx.batch_probe_distortion_pictures_workspace_bytes(*bad) == 0, bad


def test_the_python_wrappers_refuse_before_a_device():
    import jpegx
    pics = np.zeros((2, 20, 37, 3), np.uint8)
    for fn in (jpegx.batch_probe_pictures, jpegx.batch_probe_distortion_pictures):
        with pytest.raises(jpegx.JpegxError, match="K must be 1 .. JPEGX_PROBE_MAX_CANDIDATES"):
            fn(pics, 3, "divide", [2.0] * 33)
        with pytest.raises(jpegx.JpegxError, match="group_planes"):
            fn(pics, 3, "divide", [2.0], group_planes=4)
        with pytest.raises(jpegx.JpegxError, match="colour"):
            fn(pics, 3, "divide", [2.0], colour="bgr")
        with pytest.raises(jpegx.JpegxError, match="expected non-empty"):
            fn(np.zeros((2, 20, 37), np.uint8), 3, "divide", [2.0])
    with pytest.raises(jpegx.JpegxError, match="multiples of 8"):
        jpegx.probe_sizes_8(np.zeros((1, 12, 8)), "divide", [2.0])
    with pytest.raises(jpegx.JpegxError, match="rows, cols"):
        jpegx.probe_distortion_8(np.zeros((1, 8, 8)), np.zeros((1, 8, 8), np.uint64), 1, 9, 8, "divide", [2.0])
    with pytest.raises(jpegx.JpegxError, match="the planes' shape"):
        jpegx.probe_distortion_8(np.zeros((1, 8, 8)), np.zeros((1, 8, 16), np.uint64), 1, 8, 8, "divide", [2.0])
