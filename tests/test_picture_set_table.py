"""jpegx_picture_set_table, the host table of a set of pictures of unequal sizes, against a NumPy restatement: shapes from
pipeline._blocked_shape, first blocks as running sums, the total; and every refusal with its code.  Host arithmetic only:
nothing here touches a device.  CPU only."""
import ctypes

import numpy as np
import pytest

import jpegx
from picture_set_model import table_twin

INVALID, UNSUPPORTED = -1, -4
PIX = {1: 16, 2: 8, 3: 16, 4: 4}


def raw(desc, npictures, nbands, bs, n, room=None, total=True):
    """The C entry on a descriptor array: (rc, blob, total)."""
    blob = np.zeros(max(room if room is not None else jpegx.lib().jpegx_picture_set_table_bytes(max(npictures, 1)), 8) // 8 + 1, np.uint64)
    t = ctypes.c_longlong(-7)
    rc = jpegx.lib().jpegx_picture_set_table(desc.ctypes.data if desc is not None else None, npictures, nbands, bs, n, blob.ctypes.data,
                                             ctypes.byref(t) if total else None)
    return rc, blob, t.value


def descs(sizes, nbands, pitches=None, offsets=None):
    d = np.zeros(len(sizes), jpegx.PICTURE_DESC_DTYPE)
    for p, (r, c) in enumerate(sizes):
        d[p] = (r, c, 0 if offsets is None else offsets[p], c * nbands if pitches is None else pitches[p])
    return d


def test_the_layout_is_the_headers():
    assert jpegx.PICTURE_DESC_DTYPE.itemsize == 24 and jpegx.PICTURE_SET_HEAD_DTYPE.itemsize == 32 and jpegx.PICTURE_SET_ENTRY_DTYPE.itemsize == 64
    L = jpegx.lib()
    assert L.jpegx_picture_set_table_bytes(0) == 0 and L.jpegx_picture_set_table_bytes(-1) == 0
    for k in (1, 2, 1000):
        assert L.jpegx_picture_set_table_bytes(k) == 32 + 64 * (k + 1) + 8 * (4 * k + 1)


@pytest.mark.parametrize("nbands", [1, 2, 3, 4])
@pytest.mark.parametrize("bs,n", [(1, 2), (1, 4), (2, 3), (3, 5), (5, 24), (1, 32), (255, 2)])
def test_against_the_restatement(nbands, bs, n):
    rng = np.random.default_rng([nbands, bs, n])
    sizes = [(1, 1), (1, 300), (300, 1)] + [(int(r), int(c)) for r, c in rng.integers(1, 700, (40, 2))]
    pitches = [c * nbands + int(s) for (_, c), s in zip(sizes, rng.integers(0, 9, len(sizes)))]
    offsets = [int(o) for o in rng.integers(0, 1 << 40, len(sizes))]
    t = jpegx.picture_set_table(sizes, nbands, bs, n, offsets=offsets, pitches=pitches)
    shapes, nb, first, planes = table_twin(sizes, nbands, bs, n)
    k = len(sizes)
    assert t.npictures == k and t.nbands == nbands and t.total_blocks == first[-1]
    h = t.head
    assert (h["magic"], h["npictures"], h["nbands"], h["bs"], h["N"], h["total_blocks"]) == (0x4A505354, k, nbands, bs, n, first[-1])
    e = t.entries
    assert e.shape == (k + 1,)
    assert np.array_equal(e["rows"][:k], [r for r, _ in sizes]) and np.array_equal(e["cols"][:k], [c for _, c in sizes])
    assert np.array_equal(e["offset"][:k], np.array(offsets, np.uint64)) and np.array_equal(e["pitch"][:k], pitches)
    assert np.array_equal(e["H"][:k], [s[0] for s in shapes]) and np.array_equal(e["W"][:k], [s[1] for s in shapes])
    assert np.array_equal(e["prows"][:k], [-(-r // bs) for r, _ in sizes]) and np.array_equal(e["pcols"][:k], [-(-c // bs) for _, c in sizes])
    assert np.array_equal(e["wb"][:k], [s[1] // n for s in shapes]) and np.array_equal(e["nb"][:k], nb)
    assert np.array_equal(e["first"], first)                                  # the end included
    lanes = np.concatenate([[0], np.cumsum([r * -(-c // PIX[nbands]) for r, c in sizes])])
    assert np.array_equal(e["lanes"], lanes)
    assert np.array_equal(t.plane_first, planes)
    for p in range(k):
        assert shapes[p] == jpegx.band_shape_n(*sizes[p], bs, n)


def test_defaults_are_the_pictures_back_to_back():
    sizes = [(3, 5), (1, 1), (4, 2)]
    t = jpegx.picture_set_table(sizes, 3, 1, 4)
    assert list(t.entries["pitch"][:3]) == [15, 3, 6] and list(t.entries["offset"][:3]) == [0, 45, 48]
    rc, blob, total = raw(descs(sizes, 3, offsets=[0, 45, 48]), 3, 3, 1, 4, total=False)           # the total may be left out
    assert rc == 0 and total == -7 and np.array_equal(blob.view(np.uint8)[:t.nbytes], t.blob.view(np.uint8)[:t.nbytes])


REFUSALS = [
    ("no pictures", dict(npictures=0), INVALID, b"count"),
    ("negative pictures", dict(npictures=-1), INVALID, b"count"),
    ("no bands", dict(nbands=0), INVALID, b"bands"),
    ("five bands", dict(nbands=5), INVALID, b"bands"),
    ("bs 0", dict(bs=0), UNSUPPORTED, b"block_size"),
    ("bs 256", dict(bs=256), UNSUPPORTED, b"block_size"),
    ("N 1", dict(n=1), INVALID, b"dct_size"),
    ("N 33", dict(n=33), INVALID, b"dct_size"),
]


@pytest.mark.parametrize("what,over,code,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_of_the_settings(what, over, code, word):
    a = dict(npictures=2, nbands=3, bs=1, n=4)
    a.update(over)
    rc, blob, _ = raw(descs([(4, 4), (5, 5)], 3, pitches=[15, 15]), a["npictures"], a["nbands"], a["bs"], a["n"])
    assert rc == code and word in jpegx.lib().jpegx_last_error(), what
    assert not blob.any(), "a refused table was written"


def test_refusals_of_a_picture_name_it():
    L = jpegx.lib()
    for bad, word in (((0, 4), b"rows and cols"), ((4, 0), b"rows and cols"), ((-3, 4), b"rows and cols"), ((65536, 32768), b"2^31")):
        rc, _, _ = raw(descs([(4, 4), bad, (5, 5)], 3, pitches=[12, max(bad[1], 1) * 3, 15]), 3, 3, 1, 4)
        assert rc == INVALID and word in L.jpegx_last_error() and b"picture 1" in L.jpegx_last_error(), bad
    rc, _, _ = raw(descs([(4, 4), (4, 4)], 3, pitches=[12, 11]), 2, 3, 1, 4)
    assert rc == INVALID and b"pitch" in L.jpegx_last_error() and b"picture 1" in L.jpegx_last_error()
    assert raw(descs([(4, 4), (4, 4)], 3, pitches=[12, 12]), 2, 3, 1, 4)[0] == 0
    assert raw(None, 2, 3, 1, 4)[0] == INVALID and b"null" in L.jpegx_last_error()
    assert L.jpegx_picture_set_table(descs([(4, 4)], 3).ctypes.data, 1, 3, 1, 4, None, None) == INVALID
    with pytest.raises(jpegx.JpegxError, match="pitch"):
        jpegx.picture_set_table([(4, 4)], 3, 1, 4, pitches=[11])
    with pytest.raises(jpegx.JpegxError, match="count"):
        jpegx.picture_set_table([], 3, 1, 4)


def test_the_2_to_31_limit_of_the_sum_at_the_last_admitted_and_the_first_refused_set():
    """nbands * H * W summed over the pictures <= 2^31 - 1: 42 pictures of 4096 x 4096 at N 4 and three bands are 2^31 - 2^25
    samples; a picture of 4096 x 2728 more stays below the limit, one block column more (4096 x 2732) passes it."""
    sizes = [(4096, 4096)] * 42
    assert 3 * (42 * 4096 * 4096 + 4096 * 2728) <= 2 ** 31 - 1 < 3 * (42 * 4096 * 4096 + 4096 * 2732)
    t = jpegx.picture_set_table(sizes + [(4096, 2728)], 3, 1, 4)
    assert t.total_blocks * 16 == 3 * (42 * 4096 * 4096 + 4096 * 2728)
    with pytest.raises(jpegx.JpegxError, match="2\\^31"):
        jpegx.picture_set_table(sizes + [(4096, 2729)], 3, 1, 4)
    # one plane beyond 2^31 - 1 samples is jpegx_band_shape_n's refusal
    with pytest.raises(jpegx.JpegxError, match="2\\^31"):
        jpegx.picture_set_table([(46341, 46341)], 1, 1, 2)
