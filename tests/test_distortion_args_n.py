"""The entries of the distortion probe (jpegx_band_moments_packed_stacked_n, jpegx_probe_distortion_n,
jpegx_batch_probe_distortion_pictures_workspace_bytes_n, jpegx_batch_probe_distortion_pictures_n): every bad argument is refused
before a device is needed, with a message that names it, and the workspace function is pinned to its documented formula.  CPU
only."""
import ctypes

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -4
NONE, DISCARD, DIVIDE, QTABLE = 0, 1, 2, 3


def _aligned(nbytes=4096):
    buf = ctypes.create_string_buffer(nbytes + 256)
    return buf, (ctypes.addressof(buf) + 255) & ~255


class Calls:
    """The three compute entries with one valid-looking argument list each; a call replaces arguments by name.  Nothing here may
    reach a device: every call below is refused first (this machine has none, a reached device would answer JPEGX_E_NODEVICE
    or JPEGX_E_HIP, never JPEGX_E_INVALID)."""

    def __init__(self, jpegx, on=False):
        self.L = jpegx.lib()
        self.keep, self.p = _aligned()
        self.on = on

    def _call(self, name, order, kw):
        names = [k for k, _ in order]
        unknown = set(kw) - set(names)
        assert not unknown, unknown
        args = [kw.get(k, d) for k, d in order]
        if "params" in names:
            params = np.ascontiguousarray(args[names.index("params")], dtype=np.float64)
            args[names.index("params")] = params.ctypes.data
            if "K" not in kw:
                args[names.index("K")] = params.size
        fn = getattr(self.L, name + ("_on" if self.on else ""))
        return fn(0, *args) if self.on else fn(*args)

    def moments(self, **kw):
        return self._call("jpegx_band_moments_packed_stacked_n",
                          (("pixels", self.p), ("npictures", 2), ("nbands", 3), ("rows", 12), ("cols", 20), ("pitch", 60), ("colour", 0),
                           ("bs", 3), ("N", 4), ("moments", self.p), ("out_pitch", 8), ("stream", None)), kw)

    def probe(self, **kw):
        # a 12 x 20 band pooled 3 x 3 is 4 x 7 samples: planes of 4 x 8
        return self._call("jpegx_probe_distortion_n",
                          (("planes", self.p), ("moments", self.p), ("nplanes", 3), ("H", 4), ("W", 8), ("pitch", 8), ("mpitch", 8), ("N", 4),
                           ("bs", 3), ("rows", 12), ("cols", 20), ("mode", DIVIDE), ("params", [40.0]), ("K", 1), ("totals", self.p),
                           ("stream", None)), kw)

    def batch(self, **kw):
        return self._call("jpegx_batch_probe_distortion_pictures_n",
                          (("pixels", self.p), ("npictures", 2), ("nbands", 3), ("rows", 12), ("cols", 20), ("pitch", 60), ("colour", 0),
                           ("bs", 3), ("N", 4), ("mode", DIVIDE), ("params", [40.0]), ("K", 1), ("group_planes", 3), ("ws", self.p),
                           ("totals", self.p), ("stream", None)), kw)

    def err(self):
        return self.L.jpegx_last_error()


def _refusals(c):
    for entry in (c.probe, c.batch):
        # the candidate count
        for k in (0, 33):
            assert entry(params=[40.0] * 33, K=k) == INVALID and b"K must be 1 .. JPEGX_PROBE_MAX_CANDIDATES" in c.err(), k
        # the quantiser
        assert entry(mode=QTABLE) == INVALID and b"qtable: the luminance table is 8 x 8" in c.err()
        assert entry(mode=7) == INVALID and b"unknown quantiser mode" in c.err()
        assert entry(mode=NONE, params=[0.0, 0.0]) == INVALID and b"K must be 1 for the quantiser 'none'" in c.err()
        # every parameter by the rules of the forward entry, the message naming its place
        for bad in (0.0, float("nan"), float("inf"), float("-inf")):
            assert entry(params=[40.0, bad, 8.0]) == INVALID, bad
            assert b"h_params[1]: divide: divisor must be finite and non-zero" in c.err(), bad
        for bad in (2.5, -1.0, float("nan")):
            assert entry(mode=DISCARD, params=[0.0, 1.0, bad]) == INVALID, bad
            assert b"h_params[2]: discard: keep must be a non-negative integer" in c.err(), bad
        # dct_size
        for n in (1, 33):
            assert entry(N=n) == INVALID and b"2 .. 32" in c.err(), n
    for n in (1, 33):
        assert c.moments(N=n) == INVALID and b"2 .. 32" in c.err(), n
    # null pointers
    for name in ("planes", "moments", "totals"):
        assert c.probe(**{name: None}) == INVALID and b"null" in c.err() and name.encode() in c.err(), name
    for name in ("pixels", "ws", "totals"):
        assert c.batch(**{name: None}) == INVALID and b"null" in c.err(), name
    for name in ("pixels", "moments"):
        assert c.moments(**{name: None}) == INVALID and b"null" in c.err(), name
    # shapes
    assert c.probe(nplanes=0) == INVALID and b"nplanes" in c.err()
    assert c.batch(npictures=0) == INVALID and b"picture count" in c.err()
    assert c.moments(npictures=0) == INVALID and b"picture count" in c.err()
    assert c.probe(H=6) == INVALID and b"H, W" in c.err() and b"multiples of dct_size" in c.err()
    assert c.probe(pitch=7) == INVALID and b"pitch smaller than width" in c.err() and b"mpitch" not in c.err()
    assert c.probe(mpitch=7) == INVALID and b"mpitch" in c.err()
    for bs in (0, 256, -1):
        assert c.probe(bs=bs) == INVALID and b"bs: block_size must be in 1..255" in c.err(), bs
    # rows and cols must give H and W: 13 rows pool to 5 samples, planes of 8 rows; 25 columns pool to 9, planes of 12
    for change in (dict(rows=13), dict(cols=25), dict(rows=0), dict(cols=-1), dict(bs=2), dict(H=8), dict(W=12, pitch=12, mpitch=12)):
        assert c.probe(**change) == INVALID and b"rows, cols" in c.err(), change
    assert c.batch(pitch=59) == INVALID and b"pitch smaller than the row" in c.err()
    assert c.moments(pitch=59) == INVALID and b"pitch smaller than the row" in c.err()
    assert c.moments(out_pitch=7) == INVALID and b"pitch smaller than the row" in c.err()
    for gp in (0, -3, 2, 4):
        assert c.batch(group_planes=gp) == INVALID and b"group_planes must be a positive multiple of the band count" in c.err(), gp
    for entry in (c.batch, c.moments):
        assert entry(nbands=3, colour=2) == INVALID and b"colour" in c.err()
        assert entry(nbands=0) == INVALID and b"bands" in c.err()
        assert entry(nbands=5, pitch=100) == INVALID and b"bands" in c.err()
        assert entry(bs=0) == UNSUPPORTED and entry(bs=256) == UNSUPPORTED
        assert entry(rows=0) == INVALID and entry(cols=0) == INVALID
    assert c.batch(nbands=1, colour=1, pitch=20, group_planes=1) == INVALID and b"colour" in c.err()
    assert c.moments(nbands=1, colour=1, pitch=20) == INVALID and b"three bands" in c.err()
    # a batch of 2^31 coefficients: 2 planes of 32768 x 32768; 43 pictures of 3 planes of 4096 x 4096
    assert c.probe(nplanes=2, H=32768, W=32768, pitch=32768, mpitch=32768, bs=1, rows=32768, cols=32768) == INVALID and b"2^31" in c.err()
    assert c.batch(npictures=43, rows=4096, cols=4096, pitch=3 * 4096, bs=1) == INVALID and b"2^31" in c.err()
    assert c.moments(npictures=43, rows=4096, cols=4096, pitch=3 * 4096, bs=1, out_pitch=4096) == INVALID and b"2^31" in c.err()
    # alignment
    for name in ("planes", "moments", "totals"):
        assert c.probe(**{name: c.p + 4}) == INVALID and b"8-byte aligned" in c.err(), name
    assert c.batch(ws=c.p + 8) == INVALID and b"16-byte aligned" in c.err()
    assert c.batch(totals=c.p + 4) == INVALID and b"8-byte aligned" in c.err()
    assert c.moments(moments=c.p + 4) == INVALID and b"misaligned" in c.err()


def test_every_refusal_happens_without_a_device():
    import jpegx
    _refusals(Calls(jpegx))


NAMES = ("jpegx_band_moments_packed_stacked_n", "jpegx_probe_distortion_n", "jpegx_batch_probe_distortion_pictures_n")


def test_the_explicit_device_forms_exist_and_are_bound():
    import jpegx
    for name in NAMES:
        assert jpegx.SIGNATURES[name + "_on"] == [ctypes.c_int] + jpegx.SIGNATURES[name]
        assert hasattr(jpegx.lib(), name + "_on")
    if jpegx.device_count() > 0:
        _refusals(Calls(jpegx, on=True))


def test_a_valid_call_is_not_refused_by_the_checks():
    """The argument lists above pass every check: without a device the answer is 'no device' or a HIP failure, never INVALID; with
    one they are not sent (the pointers are host memory)."""
    import jpegx
    if jpegx.device_count() > 0:
        return
    c = Calls(jpegx)
    for entry in (c.moments, c.probe, c.batch):
        assert entry() not in (0, INVALID, UNSUPPORTED)


def test_the_header_cites_the_reference_for_the_new_entries():
    import os
    from conftest import REPO
    text = open(os.path.join(REPO, "include", "jpegx.h")).read()
    at = text.index("distortion probe")
    section = text[at:text.index("jpegx_batch_probe_distortion_pictures_n(", at)]
    for needle in ("pipeline/quantization.py", "quantizers.py:23-31", "pipeline/subsampling.py:13-14", "padding.py:14-16",
                   "dct_padding.py:11-21", "Normalization.invert"):
        assert needle in section, needle


def _up256(v):
    return (v + 255) & ~255


def _blocked(rows, cols, bs, n):
    return tuple(-(-(-(-v // bs)) // n) * n for v in (rows, cols))


@pytest.mark.parametrize("npictures, nbands, rows, cols, bs, n, gp", [
    (2, 3, 12, 20, 3, 4, 3), (5, 3, 37, 45, 2, 3, 6), (5, 3, 37, 45, 2, 3, 300), (1, 1, 64, 64, 1, 16, 1), (7, 4, 130, 125, 5, 24, 8),
    (4096, 3, 64, 64, 1, 4, 3 * 1024)])
def test_workspace_is_one_group_of_planes_and_one_of_moments(npictures, nbands, rows, cols, bs, n, gp):
    import jpegx
    h, w = _blocked(rows, cols, bs, n)
    assert jpegx.band_shape_n(rows, cols, bs, n) == (h, w)
    want = 2 * _up256(min(gp, nbands * npictures) * h * w * 8)
    assert jpegx.batch_probe_distortion_pictures_workspace_bytes_n(npictures, nbands, rows, cols, bs, n, gp) == want
    assert want == 2 * jpegx.batch_probe_pictures_workspace_bytes_n(npictures, nbands, rows, cols, bs, n, gp)


def test_workspace_is_zero_for_exactly_the_refused_shapes():
    import jpegx
    ok = dict(npictures=2, nbands=3, rows=12, cols=20, bs=3, n=4, group_planes=3)
    assert jpegx.batch_probe_distortion_pictures_workspace_bytes_n(**ok) > 0
    c = Calls(jpegx)
    renamed = {"n": "N"}
    for change in (dict(n=1), dict(n=33), dict(npictures=0), dict(nbands=0), dict(nbands=5), dict(rows=0), dict(cols=0), dict(bs=0), dict(bs=256),
                   dict(group_planes=0), dict(group_planes=2), dict(group_planes=4), dict(group_planes=-3),
                   dict(npictures=43, rows=4096, cols=4096, bs=1)):
        assert jpegx.batch_probe_distortion_pictures_workspace_bytes_n(**dict(ok, **change)) == 0, change
        kw = {renamed.get(k, k): v for k, v in change.items()}
        if "cols" in kw or "nbands" in kw:
            kw["pitch"] = max(kw.get("cols", 20), 1) * max(kw.get("nbands", 3), 1)
        assert c.batch(**kw) in (INVALID, UNSUPPORTED), change
    # ... and not for the largest batch the entry takes: 42 such pictures are 2^31 - 2^25 coefficients
    assert jpegx.batch_probe_distortion_pictures_workspace_bytes_n(**dict(ok, npictures=42, rows=4096, cols=4096, bs=1)) == 2 * 3 * 4096 * 4096 * 8


def test_host_convenience_refuses_before_it_asks_for_a_device():
    import jpegx
    pics = np.zeros((2, 12, 20, 3), np.uint8)
    with pytest.raises(jpegx.JpegxError, match="K must be 1 .. JPEGX_PROBE_MAX_CANDIDATES"):
        jpegx.batch_probe_distortion_pictures_n(pics, 3, 4, "divide", [2.0] * 33)
    with pytest.raises(jpegx.JpegxError, match="group_planes"):
        jpegx.batch_probe_distortion_pictures_n(pics, 3, 4, "divide", [2.0], group_planes=4)
    with pytest.raises(jpegx.JpegxError, match="colour"):
        jpegx.batch_probe_distortion_pictures_n(pics[..., :1], 3, 4, "divide", [2.0], colour="rgb")
    with pytest.raises(jpegx.JpegxError, match="uint8"):
        jpegx.batch_probe_distortion_pictures_n(pics.astype(np.int32), 3, 4, "divide", [2.0])
