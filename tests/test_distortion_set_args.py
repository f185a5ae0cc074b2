"""The entries of the distortion probe over a set of pictures of unequal sizes (jpegx_picture_set_moments_n,
jpegx_probe_distortion_set_n, jpegx_batch_probe_distortion_picture_set_workspace_bytes_n,
jpegx_batch_probe_distortion_picture_set_n): every bad argument is refused before a device is needed, with a message that names
it, and the workspace function is pinned to its documented formula.  CPU only."""
import ctypes

import numpy as np
import pytest

INVALID = -1
NONE, DISCARD, DIVIDE, QTABLE = 0, 1, 2, 3
SIZES = [(12, 20), (33, 7), (5, 5), (40, 41)]


def _aligned(nbytes=4096):
    buf = ctypes.create_string_buffer(nbytes + 256)
    return buf, (ctypes.addressof(buf) + 255) & ~255


def _up256(v):
    return (v + 255) & ~255


def _forged(jpegx, table, **fields):
    """A copy of the table's blob with fields of its head replaced."""
    blob = table.blob.copy()
    head = blob.view(np.uint8)[:32].view(jpegx.PICTURE_SET_HEAD_DTYPE)
    for k, v in fields.items():
        head[k] = v
    return blob


class Calls:
    """The three compute entries with one valid-looking argument list each; a call replaces arguments by name.  Nothing here may
    reach a device: every call below is refused first (a reached device would answer JPEGX_E_NODEVICE or JPEGX_E_HIP, never
    JPEGX_E_INVALID)."""

    def __init__(self, jpegx, nbands=3, on=False, device=0):
        self.L = jpegx.lib()
        self.keep, self.p = _aligned()
        self.on, self.device = on, device
        self.table = jpegx.picture_set_table(SIZES, nbands, 2, 4)

    def _call(self, name, order, kw):
        names = [k for k, _ in order]
        assert not set(kw) - set(names), set(kw) - set(names)
        args = [kw.get(k, d) for k, d in order]
        if "params" in names:
            params = np.ascontiguousarray(args[names.index("params")], dtype=np.float64)
            args[names.index("params")] = params.ctypes.data
            if "K" not in kw:
                args[names.index("K")] = params.size
        fn = getattr(self.L, name + ("_on" if self.on else ""))
        return fn(self.device, *args) if self.on else fn(*args)

    def moments(self, **kw):
        return self._call("jpegx_picture_set_moments_n", (("pixels", self.p), ("h_table", self.table.ptr), ("d_table", self.p), ("p0", 1), ("k", 2),
                                                          ("colour", 0), ("moments", self.p), ("stream", None)), kw)

    def probe(self, **kw):
        return self._call("jpegx_probe_distortion_set_n",
                          (("strip", self.p), ("moments", self.p), ("h_table", self.table.ptr), ("d_table", self.p), ("p0", 1), ("k", 2),
                           ("mode", DIVIDE), ("params", [40.0]), ("K", 1), ("totals", self.p), ("stream", None)), kw)

    def batch(self, **kw):
        return self._call("jpegx_batch_probe_distortion_picture_set_n",
                          (("pixels", self.p), ("h_table", self.table.ptr), ("d_table", self.p), ("colour", 0), ("mode", DIVIDE),
                           ("params", [40.0]), ("K", 1), ("group_samples", 0), ("ws", self.p), ("totals", self.p), ("stream", None)), kw)

    def err(self):
        return self.L.jpegx_last_error()


def _refusals(jpegx, c):
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
        # alignment of the totals
        assert entry(totals=c.p + 4) == INVALID and b"8-byte aligned" in c.err()
        assert entry(totals=None) == INVALID and b"null" in c.err()
    assert b"probe_distortion_set_n" in (c.probe(mode=7), c.err())[1]
    for entry in (c.moments, c.probe, c.batch):
        # a forged head
        for fields in (dict(magic=0x12345678), dict(nbands=0), dict(nbands=5)):
            forged = _forged(jpegx, c.table, **fields)
            assert entry(h_table=forged.ctypes.data) == INVALID and b"is not a table of jpegx_picture_set_table" in c.err(), fields
        # null pointers
        for name in ("h_table", "d_table"):
            assert entry(**{name: None}) == INVALID and b"null" in c.err(), name
        assert entry(d_table=c.p + 4) == INVALID and b"d_table must be 8-byte aligned" in c.err()
    for entry in (c.probe, c.batch):
        for fields in (dict(N=1), dict(N=33)):
            forged = _forged(jpegx, c.table, **fields)
            assert entry(h_table=forged.ctypes.data) == INVALID and b"is not a table of jpegx_picture_set_table" in c.err(), fields
    # the probe's two strips
    for name in ("strip", "moments"):
        assert c.probe(**{name: None}) == INVALID and b"null" in c.err(), name
        assert c.probe(**{name: c.p + 4}) == INVALID and b"8-byte aligned" in c.err(), name
    # the gather's pointers: the moments strip takes 16-byte stores
    for name in ("pixels", "moments"):
        assert c.moments(**{name: None}) == INVALID and b"null" in c.err(), name
    assert c.moments(moments=c.p + 8) == INVALID and b"16-byte aligned" in c.err()
    assert c.moments(colour=2) == INVALID and b"colour" in c.err()
    for name in ("pixels", "ws"):
        assert c.batch(**{name: None}) == INVALID and b"null" in c.err(), name
    assert c.batch(ws=c.p + 8) == INVALID and b"16-byte aligned" in c.err()
    # the range of pictures
    n = len(SIZES)
    for p0, k in ((-1, 1), (0, 0), (0, -1), (n, 1), (0, n + 1), (n - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1)):
        for entry in (c.probe, c.moments):
            assert entry(p0=p0, k=k) == INVALID and b"are not pictures of the table's" in c.err(), (p0, k)
    # the groups and the colour
    for gs in (-1, -2 ** 40):
        assert c.batch(group_samples=gs) == INVALID and b"group_samples must be 0 (2^26) or positive" in c.err(), gs
    assert c.batch(colour=2) == INVALID and b"colour" in c.err()
    one = Calls(jpegx, nbands=1, on=c.on)
    assert one.batch(colour=1) == INVALID and b"colour must be 0" in one.err()
    assert one.moments(colour=1) == INVALID and b"colour must be 0" in one.err()


def test_every_refusal_happens_without_a_device():
    import jpegx
    _refusals(jpegx, Calls(jpegx))


def test_the_explicit_device_forms_exist_and_are_bound():
    import jpegx
    for name in ("jpegx_picture_set_moments_n", "jpegx_probe_distortion_set_n", "jpegx_batch_probe_distortion_picture_set_n"):
        assert jpegx.SIGNATURES[name + "_on"] == [ctypes.c_int] + jpegx.SIGNATURES[name]
        assert hasattr(jpegx.lib(), name + "_on")
    assert jpegx.RESTYPES["jpegx_batch_probe_distortion_picture_set_workspace_bytes_n"] is ctypes.c_size_t
    if jpegx.device_count() > 0:
        _refusals(jpegx, Calls(jpegx, on=True))


def test_the_explicit_device_forms_refuse_a_bad_device_index():
    import jpegx
    for device in (-1, 1 << 20):
        c = Calls(jpegx, on=True, device=device)
        for entry in (c.moments, c.probe, c.batch):
            assert entry() != 0, device


def _samples(table, n):
    first = table.entries["first"].astype(np.int64)
    return ((first[1:] - first[:-1]) * n * n).tolist()


@pytest.mark.parametrize("nbands, bs, n", [(3, 1, 4), (1, 1, 16), (3, 5, 24), (4, 2, 3)])
def test_workspace_is_a_strip_and_its_moments_of_the_largest_group(nbands, bs, n):
    import jpegx
    sizes = [(17, 23), (40, 41), (9, 131), (300, 280), (33, 7), (64, 64), (5, 5)]      # the fourth is the lone largest
    table = jpegx.picture_set_table(sizes, nbands, bs, n)
    samples = _samples(table, n)
    total, lone = sum(samples), max(samples)
    assert jpegx.batch_probe_distortion_picture_set_workspace_bytes_n(table) == 2 * _up256(8 * total)
    assert jpegx.batch_probe_distortion_picture_set_workspace_bytes_n(table, lone - 1) == 2 * _up256(8 * lone)
    gs = lone + min(samples)
    assert jpegx.batch_probe_distortion_picture_set_workspace_bytes_n(table, gs) == 2 * _up256(8 * min(gs, total))
    # twice the size probe's: one strip more, nothing else
    for gs in (0, lone - 1, lone + min(samples)):
        assert jpegx.batch_probe_distortion_picture_set_workspace_bytes_n(table, gs) == 2 * jpegx.batch_probe_picture_set_workspace_bytes_n(table, gs)


def test_workspace_is_zero_for_what_the_entry_refuses():
    import jpegx
    c = Calls(jpegx)
    assert jpegx.batch_probe_distortion_picture_set_workspace_bytes_n(c.table) > 0
    assert jpegx.batch_probe_distortion_picture_set_workspace_bytes_n(c.table, -1) == 0
    L = jpegx.lib()
    for fields in (dict(magic=0), dict(nbands=0), dict(nbands=5), dict(N=1), dict(N=33), dict(npictures=0)):
        forged = _forged(jpegx, c.table, **fields)
        assert L.jpegx_batch_probe_distortion_picture_set_workspace_bytes_n(forged.ctypes.data, 0) == 0, fields
        assert c.batch(h_table=forged.ctypes.data) == INVALID, fields
    assert L.jpegx_batch_probe_distortion_picture_set_workspace_bytes_n(None, 0) == 0


def test_host_convenience_refuses_before_it_asks_for_a_device():
    import jpegx
    pics = [np.zeros((12, 20, 3), np.uint8), np.zeros((7, 33, 3), np.uint8)]
    with pytest.raises(jpegx.JpegxError, match="K must be 1 .. JPEGX_PROBE_MAX_CANDIDATES"):
        jpegx.batch_probe_distortion_picture_set_n(pics, 3, 4, "divide", [2.0] * 33)
    with pytest.raises(jpegx.JpegxError, match="group_samples"):
        jpegx.batch_probe_distortion_picture_set_n(pics, 3, 4, "divide", [2.0], group_samples=-1)
    with pytest.raises(jpegx.JpegxError, match="colour"):
        jpegx.batch_probe_distortion_picture_set_n([p[..., :1] for p in pics], 3, 4, "divide", [2.0], colour="rgb")
    with pytest.raises(jpegx.JpegxError, match="uint8"):
        jpegx.batch_probe_distortion_picture_set_n([p.astype(np.int32) for p in pics], 3, 4, "divide", [2.0])
    with pytest.raises(jpegx.JpegxError, match="2 .. 32"):
        jpegx.batch_probe_distortion_picture_set_n(pics, 3, 33, "divide", [2.0])
