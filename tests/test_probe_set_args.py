"""The three entries of the size probe over a set of pictures of unequal sizes (jpegx_probe_sizes_set_n,
jpegx_batch_probe_picture_set_workspace_bytes_n, jpegx_batch_probe_picture_set_n): every bad argument is refused before a
device is needed, with a message that names it, and the workspace function is pinned to its documented formula.  CPU only."""
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
    """The two compute entries with one valid-looking argument list each; a call replaces arguments by name.  Nothing here may
    reach a device: every call below is refused first (a reached device would answer JPEGX_E_NODEVICE or JPEGX_E_HIP, never
    JPEGX_E_INVALID)."""

    def __init__(self, jpegx, nbands=3, on=False):
        self.L = jpegx.lib()
        self.keep, self.p = _aligned()
        self.on = on
        self.table = jpegx.picture_set_table(SIZES, nbands, 2, 4)

    def _call(self, name, order, kw):
        names = [k for k, _ in order]
        assert not set(kw) - set(names), set(kw) - set(names)
        args = [kw.get(k, d) for k, d in order]
        params = np.ascontiguousarray(args[names.index("params")], dtype=np.float64)
        args[names.index("params")] = params.ctypes.data
        if "K" not in kw:
            args[names.index("K")] = params.size
        fn = getattr(self.L, name + ("_on" if self.on else ""))
        return fn(0, *args) if self.on else fn(*args)

    def probe(self, **kw):
        return self._call("jpegx_probe_sizes_set_n", (("strip", self.p), ("h_table", self.table.ptr), ("d_table", self.p), ("p0", 1), ("k", 2),
                                                      ("mode", DIVIDE), ("params", [40.0]), ("K", 1), ("totals", self.p), ("stream", None)), kw)

    def batch(self, **kw):
        return self._call("jpegx_batch_probe_picture_set_n",
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
        # a forged head
        for fields in (dict(magic=0x12345678), dict(nbands=0), dict(nbands=5), dict(N=1), dict(N=33)):
            forged = _forged(jpegx, c.table, **fields)
            assert entry(h_table=forged.ctypes.data) == INVALID and b"is not a table of jpegx_picture_set_table" in c.err(), fields
        # null pointers
        for name in ("h_table", "d_table", "totals"):
            assert entry(**{name: None}) == INVALID and b"null" in c.err(), name
        # alignment
        assert entry(d_table=c.p + 4) == INVALID and b"d_table must be 8-byte aligned" in c.err()
        assert entry(totals=c.p + 4) == INVALID and b"8-byte aligned" in c.err()
    assert c.probe(strip=None) == INVALID and b"null" in c.err()
    assert c.probe(strip=c.p + 4) == INVALID and b"8-byte aligned" in c.err()
    for name in ("pixels", "ws"):
        assert c.batch(**{name: None}) == INVALID and b"null" in c.err(), name
    assert c.batch(ws=c.p + 8) == INVALID and b"16-byte aligned" in c.err()
    # the range of pictures
    n = len(SIZES)
    for p0, k in ((-1, 1), (0, 0), (0, -1), (n, 1), (0, n + 1), (n - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert c.probe(p0=p0, k=k) == INVALID and b"are not pictures of the table's" in c.err(), (p0, k)
    # the groups and the colour
    for gs in (-1, -2 ** 40):
        assert c.batch(group_samples=gs) == INVALID and b"group_samples must be 0 (2^26) or positive" in c.err(), gs
    assert c.batch(colour=2) == INVALID and b"colour" in c.err()
    one = Calls(jpegx, nbands=1, on=c.on)
    assert one.batch(colour=1) == INVALID and b"colour must be 0" in one.err()


def test_every_refusal_happens_without_a_device():
    import jpegx
    _refusals(jpegx, Calls(jpegx))


def test_the_explicit_device_forms_exist_and_are_bound():
    import jpegx
    for name in ("jpegx_probe_sizes_set_n", "jpegx_batch_probe_picture_set_n"):
        assert jpegx.SIGNATURES[name + "_on"] == [ctypes.c_int] + jpegx.SIGNATURES[name]
        assert hasattr(jpegx.lib(), name + "_on")
    assert jpegx.RESTYPES["jpegx_batch_probe_picture_set_workspace_bytes_n"] is ctypes.c_size_t
    if jpegx.device_count() > 0:
        _refusals(jpegx, Calls(jpegx, on=True))


def _samples(table, n):
    """Samples per picture, from the table's entries."""
    first = table.entries["first"].astype(np.int64)
    return ((first[1:] - first[:-1]) * n * n).tolist()


def _largest_group(samples, gs):
    """The compress cut: whole pictures while the group's samples stay within gs, one at least."""
    groups, at = [], 0
    while at < len(samples):
        held, end = samples[at], at + 1
        while end < len(samples) and held + samples[end] <= gs:
            held += samples[end]
            end += 1
        groups.append(held)
        at = end
    return max(groups), len(groups)


@pytest.mark.parametrize("nbands, bs, n", [(3, 1, 4), (1, 1, 16), (3, 5, 24), (4, 2, 3)])
def test_workspace_is_the_strip_of_the_largest_group(nbands, bs, n):
    import jpegx
    sizes = [(17, 23), (40, 41), (9, 131), (300, 280), (33, 7), (64, 64), (5, 5)]      # the fourth is the lone largest
    table = jpegx.picture_set_table(sizes, nbands, bs, n)
    samples = _samples(table, n)
    for (rows, cols), s in zip(sizes, samples):
        h, w = jpegx.band_shape_n(rows, cols, bs, n)
        assert s == nbands * h * w
    total, lone = sum(samples), max(samples)
    assert samples.index(lone) == 3 and samples.count(lone) == 1
    # the default: the whole set is one group
    assert jpegx.batch_probe_picture_set_workspace_bytes_n(table) == _up256(8 * total)
    # a limit below the lone largest picture, which is then a group of its own above the limit: the formula's documented bound
    gs = lone - 1
    assert all(s <= gs for i, s in enumerate(samples) if i != 3)
    assert jpegx.batch_probe_picture_set_workspace_bytes_n(table, gs) == _up256(8 * lone)
    assert _largest_group(samples, gs)[0] == lone and _largest_group(samples, gs)[1] >= 3
    # a limit that holds several pictures: never less than the largest group of the cut, never more than the limit's samples
    gs = lone + min(samples)
    got = jpegx.batch_probe_picture_set_workspace_bytes_n(table, gs)
    assert _up256(8 * _largest_group(samples, gs)[0]) <= got == _up256(8 * min(gs, total))
    # and nothing of the compress workspace's other parts
    assert got < jpegx.batch_set_workspace_bytes_n(table, gs)


def test_workspace_is_zero_for_what_the_entry_refuses():
    import jpegx
    c = Calls(jpegx)
    assert jpegx.batch_probe_picture_set_workspace_bytes_n(c.table) > 0
    assert jpegx.batch_probe_picture_set_workspace_bytes_n(c.table, -1) == 0
    L = jpegx.lib()
    for fields in (dict(magic=0), dict(nbands=0), dict(nbands=5), dict(N=1), dict(N=33), dict(npictures=0)):
        forged = _forged(jpegx, c.table, **fields)
        assert L.jpegx_batch_probe_picture_set_workspace_bytes_n(forged.ctypes.data, 0) == 0, fields
        assert c.batch(h_table=forged.ctypes.data) == INVALID, fields
    assert L.jpegx_batch_probe_picture_set_workspace_bytes_n(None, 0) == 0


def test_host_convenience_refuses_before_it_asks_for_a_device():
    import jpegx
    pics = [np.zeros((12, 20, 3), np.uint8), np.zeros((7, 33, 3), np.uint8)]
    with pytest.raises(jpegx.JpegxError, match="K must be 1 .. JPEGX_PROBE_MAX_CANDIDATES"):
        jpegx.batch_probe_picture_set_n(pics, 3, 4, "divide", [2.0] * 33)
    with pytest.raises(jpegx.JpegxError, match="group_samples"):
        jpegx.batch_probe_picture_set_n(pics, 3, 4, "divide", [2.0], group_samples=-1)
    with pytest.raises(jpegx.JpegxError, match="colour"):
        jpegx.batch_probe_picture_set_n([p[..., :1] for p in pics], 3, 4, "divide", [2.0], colour="rgb")
    with pytest.raises(jpegx.JpegxError, match="uint8"):
        jpegx.batch_probe_picture_set_n([p.astype(np.int32) for p in pics], 3, 4, "divide", [2.0])
    with pytest.raises(jpegx.JpegxError, match="2 .. 32"):
        jpegx.batch_probe_picture_set_n(pics, 3, 33, "divide", [2.0])
