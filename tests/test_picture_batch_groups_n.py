"""jpegx_batch_groups_pictures_n, the cut of a coded batch of pictures into decoding groups ON PICTURE BOUNDARIES, against a
NumPy restatement of its rule on synthetic plane offsets.  Host arithmetic only: CPU."""
import ctypes

import numpy as np
import pytest

import jpegx

GROUP_BYTES = 64 << 20
MAX_STREAM = 2 ** 32 - 4096
MIB = 1 << 20
SHAPE = (100, 150, 1, 4)                                  # planes of 100 x 152 samples


def restated(off, npictures, nbands, group_planes):
    """From the first picture not yet taken: whole pictures while the group holds fewer than group_planes / nbands of them and
    its bytes stay within 64 MiB; one picture at least.  Pictures are counted."""
    limit = group_planes // nbands
    first, p0 = [], 0
    while p0 < npictures:
        p1 = p0 + 1
        while p1 < npictures and p1 - p0 < limit and int(off[(p1 + 1) * nbands]) - int(off[p0 * nbands]) <= GROUP_BYTES:
            p1 += 1
        first.append(p0)
        p0 = p1
    return first + [npictures]


def offsets(sizes, start=0):
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[0] = start
    off[1:] = start + np.cumsum(np.asarray(sizes, np.uint64))
    return off


@pytest.mark.parametrize("nbands,group_planes", [(3, 3), (3, 6), (3, 9), (3, 21), (3, 3000), (1, 4), (2, 6), (4, 8)])
def test_cuts_by_picture_count_with_a_short_last_group(nbands, group_planes):
    npictures = 23
    sizes = np.random.default_rng(group_planes).integers(1000, 5000, npictures * nbands)
    off = offsets(sizes, start=12345)
    got = jpegx.batch_groups_pictures_n(off, npictures, nbands, *SHAPE, group_planes)
    assert list(got) == restated(off, npictures, nbands, group_planes)
    per = min(group_planes // nbands, npictures)
    assert list(np.diff(got)) == [per] * (npictures // per) + ([npictures % per] if npictures % per else [])


def test_a_cut_never_splits_a_picture_where_the_band_cut_does():
    """Four pictures of three bands; the 64 MiB cap falls inside picture 1 (after its first band) and inside picture 3."""
    sizes = [20 * MIB, 20 * MIB, 10 * MIB,   10 * MIB, 10 * MIB, 30 * MIB,   1, 1, 1,   30 * MIB, 30 * MIB, 30 * MIB]
    off = offsets(sizes, start=7)
    bands = list(jpegx.batch_groups_n(off, 12, *SHAPE, 12))
    assert bands == [0, 4, 9, 11, 12]                     # 60 MiB, then band 0 of picture 1 fits: the band cut splits pictures 1 and 3
    assert any(b % 3 for b in bands)
    got = list(jpegx.batch_groups_pictures_n(off, 4, 3, *SHAPE, 12))
    assert got == restated(off, 4, 3, 12) == [0, 1, 3, 4]  # picture 1 would make 100 MiB; pictures 1 + 2 are 50 MiB; picture 3 is 90 MiB
    # every group's bytes are whole pictures' bytes
    assert [int(off[3 * b]) - int(off[3 * a]) for a, b in zip(got, got[1:])] == [50 * MIB, 50 * MIB + 3, 90 * MIB]


def test_64_mib_exactly_stays_one_group():
    sizes = [32 * MIB, 16 * MIB, 16 * MIB - 3,   1, 1, 1,   1, 5, 5]
    off = offsets(sizes)
    assert list(jpegx.batch_groups_pictures_n(off, 3, 3, *SHAPE, 9)) == [0, 2, 3]       # 64 MiB with picture 1, 11 bytes more with picture 2
    sizes[0] += 1
    assert list(jpegx.batch_groups_pictures_n(offsets(sizes), 3, 3, *SHAPE, 9)) == [0, 1, 3]


def test_a_lone_picture_above_64_mib_passes_and_one_at_the_decode_limit_does_not():
    big = [1 << 30, 1 << 30, 1 << 30]                    # 3 GiB in one picture
    off = offsets([10, 10, 10] + big + [10, 10, 10])
    assert list(jpegx.batch_groups_pictures_n(off, 3, 3, *SHAPE, 9)) == [0, 1, 2, 3]
    edge = [1 << 31, (1 << 31) - 4096 - 2, 1]            # 2^32 - 4096 - 1 bytes: the last admitted
    assert sum(edge) == MAX_STREAM - 1
    off = offsets([10, 10, 10] + edge + [7, 7, 7])
    assert list(jpegx.batch_groups_pictures_n(off, 3, 3, *SHAPE, 9)) == [0, 1, 2, 3]
    edge[2] += 1                                          # 2^32 - 4096 bytes: refused, and the picture is named
    with pytest.raises(jpegx.JpegxError, match="picture 1 holds %d bytes" % MAX_STREAM):
        jpegx.batch_groups_pictures_n(offsets([10, 10, 10] + edge + [7, 7, 7]), 3, 3, *SHAPE, 9)
    # every plane of it is below the limit: the band cut takes the same offsets
    assert list(jpegx.batch_groups_n(offsets([10, 10, 10] + edge + [7, 7, 7]), 9, *SHAPE, 9))[-1] == 9


def test_random_offsets_against_the_restatement():
    rng = np.random.default_rng(2)
    for trial in range(200):
        nbands = int(rng.integers(1, 5))
        npictures = int(rng.integers(1, 15))
        scale = int(rng.choice([10, 1 << 20, 20 << 20, 70 << 20]))
        sizes = rng.integers(1, scale + 1, npictures * nbands)
        gp = nbands * int(rng.choice([1, 2, 5, 100]))
        off = offsets(sizes, start=int(rng.integers(0, 1 << 40)))
        got = list(jpegx.batch_groups_pictures_n(off, npictures, nbands, *SHAPE, gp))
        assert got == restated(off, npictures, nbands, gp), trial
        assert got[0] == 0 and got[-1] == npictures and all(b > a for a, b in zip(got, got[1:]))


def test_refusals_and_the_count_alone():
    with pytest.raises(jpegx.JpegxError, match="must not decrease"):
        jpegx.batch_groups_pictures_n(np.array([0, 9, 8, 20, 30, 40, 50], np.uint64), 2, 3, *SHAPE, 3)
    with pytest.raises(jpegx.JpegxError, match="group_planes"):
        jpegx.batch_groups_pictures_n(offsets([5] * 6), 2, 3, *SHAPE, 0)
    with pytest.raises(jpegx.JpegxError, match="group_planes"):
        jpegx.batch_groups_pictures_n(offsets([5] * 6), 2, 3, *SHAPE, 4)
    with pytest.raises(jpegx.JpegxError, match="nbands"):
        jpegx.batch_groups_pictures_n(offsets([5] * 5), 2, 3, *SHAPE, 3)
    n = ctypes.c_int(-1)
    off = offsets([5] * 30)
    assert jpegx.lib().jpegx_batch_groups_pictures_n(off.ctypes.data, 10, 3, *SHAPE, 9, None, ctypes.byref(n)) == 0 and n.value == 4
