"""The three entries of the size probe (jpegx_probe_sizes_n, jpegx_batch_probe_pictures_workspace_bytes_n,
jpegx_batch_probe_pictures_n): every bad argument is refused before a device is needed, with a message that names it, and the
workspace function is pinned to its documented formula.  CPU only."""
import ctypes

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -4
NONE, DISCARD, DIVIDE, QTABLE = 0, 1, 2, 3


def _aligned(nbytes=4096):
    buf = ctypes.create_string_buffer(nbytes + 256)
    return buf, (ctypes.addressof(buf) + 255) & ~255


class Calls:
    """The two compute entries with one valid-looking argument list each; a call replaces arguments by name.  Nothing here may
    reach a device: every call below is refused first (this machine has none, a reached device would answer JPEGX_E_NODEVICE
    or JPEGX_E_HIP, never JPEGX_E_INVALID)."""

    def __init__(self, jpegx, on=False):
        self.L = jpegx.lib()
        self.keep, self.p = _aligned()
        self.on = on

    def _call(self, name, order, kw):
        unknown = set(kw) - {k for k, _ in order}
        assert not unknown, unknown
        args = [kw.get(k, d) for k, d in order]
        params = np.ascontiguousarray(args[[k for k, _ in order].index("params")], dtype=np.float64)
        args[[k for k, _ in order].index("params")] = params.ctypes.data
        if "K" not in kw:
            args[[k for k, _ in order].index("K")] = params.size
        fn = getattr(self.L, name + ("_on" if self.on else ""))
        return fn(0, *args) if self.on else fn(*args)

    def probe(self, **kw):
        return self._call("jpegx_probe_sizes_n", (("planes", self.p), ("nplanes", 3), ("H", 8), ("W", 12), ("pitch", 12), ("N", 4),
                                                  ("mode", DIVIDE), ("params", [40.0]), ("K", 1), ("totals", self.p), ("stream", None)), kw)

    def batch(self, **kw):
        return self._call("jpegx_batch_probe_pictures_n",
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
    # null pointers
    assert c.probe(planes=None) == INVALID and b"null" in c.err()
    assert c.probe(totals=None) == INVALID and b"null" in c.err()
    for name in ("pixels", "ws", "totals"):
        assert c.batch(**{name: None}) == INVALID and b"null" in c.err(), name
    # shapes
    assert c.probe(nplanes=0) == INVALID and b"nplanes" in c.err()
    assert c.batch(npictures=0) == INVALID and b"picture count" in c.err()
    assert c.probe(H=10) == INVALID and b"multiples of dct_size" in c.err()
    assert c.probe(pitch=11) == INVALID and b"pitch" in c.err()
    assert c.batch(pitch=59) == INVALID and b"pitch smaller than the row" in c.err()
    for gp in (0, -3, 2, 4):
        assert c.batch(group_planes=gp) == INVALID and b"group_planes must be a positive multiple of the band count" in c.err(), gp
    assert c.batch(nbands=3, colour=2) == INVALID and b"colour" in c.err()
    assert c.batch(nbands=1, colour=1, pitch=20, group_planes=1) == INVALID and b"colour" in c.err()
    assert c.batch(bs=0) == UNSUPPORTED
    # a batch of 2^31 coefficients: 2 planes of 32768 x 32768; 43 pictures of 3 planes of 4096 x 4096
    assert c.probe(nplanes=2, H=32768, W=32768, pitch=32768) == INVALID and b"2^31" in c.err()
    assert c.batch(npictures=43, rows=4096, cols=4096, pitch=3 * 4096, bs=1) == INVALID and b"2^31" in c.err()
    # alignment
    assert c.probe(totals=c.p + 4) == INVALID and b"8-byte aligned" in c.err()
    assert c.batch(ws=c.p + 8) == INVALID and b"16-byte aligned" in c.err()


def test_every_refusal_happens_without_a_device():
    import jpegx
    _refusals(Calls(jpegx))


def test_the_explicit_device_forms_exist_and_are_bound():
    import jpegx
    for name in ("jpegx_probe_sizes_n", "jpegx_batch_probe_pictures_n"):
        assert jpegx.SIGNATURES[name + "_on"] == [ctypes.c_int] + jpegx.SIGNATURES[name]
        assert hasattr(jpegx.lib(), name + "_on")
    if jpegx.device_count() > 0:
        _refusals(Calls(jpegx, on=True))


def _up256(v):
    return (v + 255) & ~255


def _blocked(rows, cols, bs, n):
    return tuple(-(-(-(-v // bs)) // n) * n for v in (rows, cols))


@pytest.mark.parametrize("npictures, nbands, rows, cols, bs, n, gp", [
    (2, 3, 12, 20, 3, 4, 3), (5, 3, 37, 45, 2, 3, 6), (5, 3, 37, 45, 2, 3, 300), (1, 1, 64, 64, 1, 16, 1), (7, 4, 130, 125, 5, 24, 8),
    (4096, 3, 64, 64, 1, 4, 3 * 1024)])
def test_workspace_is_one_group_of_float64_planes(npictures, nbands, rows, cols, bs, n, gp):
    import jpegx
    h, w = _blocked(rows, cols, bs, n)
    assert jpegx.band_shape_n(rows, cols, bs, n) == (h, w)
    want = _up256(min(gp, nbands * npictures) * h * w * 8)
    assert jpegx.batch_probe_pictures_workspace_bytes_n(npictures, nbands, rows, cols, bs, n, gp) == want


def test_workspace_is_zero_for_exactly_the_refused_shapes():
    import jpegx
    ok = dict(npictures=2, nbands=3, rows=12, cols=20, bs=3, n=4, group_planes=3)
    assert jpegx.batch_probe_pictures_workspace_bytes_n(**ok) > 0
    c = Calls(jpegx)
    renamed = {"n": "N"}
    for change in (dict(n=1), dict(n=33), dict(npictures=0), dict(nbands=0), dict(nbands=5), dict(rows=0), dict(cols=0), dict(bs=0), dict(bs=256),
                   dict(group_planes=0), dict(group_planes=2), dict(group_planes=4), dict(group_planes=-3),
                   dict(npictures=43, rows=4096, cols=4096, bs=1)):
        assert jpegx.batch_probe_pictures_workspace_bytes_n(**dict(ok, **change)) == 0, change
        kw = {renamed.get(k, k): v for k, v in change.items()}
        if "cols" in kw or "nbands" in kw:
            kw["pitch"] = max(kw.get("cols", 20), 1) * max(kw.get("nbands", 3), 1)
        assert c.batch(**kw) in (INVALID, UNSUPPORTED), change
    # ... and not for the largest batch the entry takes: 42 such pictures are 2^31 - 2^25 coefficients
    assert jpegx.batch_probe_pictures_workspace_bytes_n(**dict(ok, npictures=42, rows=4096, cols=4096, bs=1)) == 3 * 4096 * 4096 * 8


def test_host_convenience_refuses_before_it_asks_for_a_device():
    import jpegx
    pics = np.zeros((2, 12, 20, 3), np.uint8)
    with pytest.raises(jpegx.JpegxError, match="K must be 1 .. JPEGX_PROBE_MAX_CANDIDATES"):
        jpegx.batch_probe_pictures_n(pics, 3, 4, "divide", [2.0] * 33)
    with pytest.raises(jpegx.JpegxError, match="group_planes"):
        jpegx.batch_probe_pictures_n(pics, 3, 4, "divide", [2.0], group_planes=4)
    with pytest.raises(jpegx.JpegxError, match="colour"):
        jpegx.batch_probe_pictures_n(pics[..., :1], 3, 4, "divide", [2.0], colour="rgb")
    with pytest.raises(jpegx.JpegxError, match="uint8"):
        jpegx.batch_probe_pictures_n(pics.astype(np.int32), 3, 4, "divide", [2.0])
