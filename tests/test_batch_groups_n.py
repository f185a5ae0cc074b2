"""jpegx_batch_groups_n, the cut of a coded batch into decoding groups, against a NumPy restatement of its rule on
synthetic plane offsets.  Host arithmetic only: CPU."""
import ctypes

import numpy as np
import pytest

import jpegx

GROUP_BYTES = 64 << 20
GROUP_SAMPLES = 1 << 26
MAX_STREAM = 2 ** 32 - 4096


def restated(off, nplanes, samples, group_planes):
    """From the first plane not yet taken: whole planes while the group holds fewer than the plane limit and its bytes
    stay within 64 MiB; one plane at least."""
    limit = group_planes if group_planes > 0 else max(1, GROUP_SAMPLES // samples)
    first, p0 = [], 0
    while p0 < nplanes:
        p1 = p0 + 1
        while p1 < nplanes and p1 - p0 < limit and int(off[p1 + 1]) - int(off[p0]) <= GROUP_BYTES:
            p1 += 1
        first.append(p0)
        p0 = p1
    return first + [nplanes]


def offsets(sizes, start=0):
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[0] = start
    off[1:] = start + np.cumsum(np.asarray(sizes, np.uint64))
    return off


SHAPE = (100, 150, 1, 4)                                  # planes of 100 x 152 = 15 200 samples
SAMPLES = 15200


@pytest.mark.parametrize("group_planes", [0, 1, 2, 3, 7, 1000])
def test_cuts_by_plane_count(group_planes):
    sizes = np.random.default_rng(group_planes).integers(1000, 5000, 23)
    off = offsets(sizes, start=12345)
    got = jpegx.batch_groups_n(off, 23, *SHAPE, group_planes)
    assert list(got) == restated(off, 23, SAMPLES, group_planes)
    if group_planes in (2, 3, 7):
        assert list(np.diff(got)) == [group_planes] * (23 // group_planes) + ([23 % group_planes] if 23 % group_planes else [])
    if group_planes in (0, 1000):
        assert list(got) == [0, 23]


def test_group_planes_0_is_the_planes_within_2_to_26_samples():
    # planes of 4096 x 4096 samples: four to a group; of 8192 x 8200: one, although 2^26 / samples is 0
    off = offsets([100] * 9)
    assert list(jpegx.batch_groups_n(off, 9, 4096, 4096, 1, 4, 0)) == [0, 4, 8, 9]
    off = offsets([100] * 3)
    assert list(jpegx.batch_groups_n(off, 3, 8192, 8200, 1, 4, 0)) == [0, 1, 2, 3]


def test_cuts_by_the_64_mib_limit():
    mib = 1 << 20
    sizes = [30 * mib, 30 * mib, 4 * mib, 1, 63 * mib, mib, 1, 64 * mib, 64 * mib + 1, 5, 5]
    off = offsets(sizes)
    got = list(jpegx.batch_groups_n(off, len(sizes), *SHAPE, 0))
    assert got == restated(off, len(sizes), SAMPLES, 0)
    assert got == [0, 3, 5, 7, 8, 9, 11]                  # 64 MiB exactly stays one group; one byte more is the next
    got = list(jpegx.batch_groups_n(off, len(sizes), *SHAPE, 2))
    assert got == restated(off, len(sizes), SAMPLES, 2) == [0, 2, 4, 6, 7, 8, 9, 11]


def test_a_lone_plane_above_64_mib():
    sizes = [10, 3 << 30, 10, MAX_STREAM - 1, 7]
    off = offsets(sizes)
    assert list(jpegx.batch_groups_n(off, 5, *SHAPE, 0)) == restated(off, 5, SAMPLES, 0) == [0, 1, 2, 3, 4, 5]
    with pytest.raises(jpegx.JpegxError, match="plane 3"):
        jpegx.batch_groups_n(offsets([10, 10, 10, MAX_STREAM, 7]), 5, *SHAPE, 0)


def test_group_starts_that_are_no_multiple_of_4():
    sizes = [5, 6, 7, 9, 10, 11, 13, 14]
    off = offsets(sizes, start=3)
    got = jpegx.batch_groups_n(off, 8, *SHAPE, 3)
    assert list(got) == [0, 3, 6, 8]
    assert [int(off[g]) % 4 for g in got[:-1]] == [3, 1, 3]


def test_random_offsets_against_the_restatement():
    rng = np.random.default_rng(1)
    for trial in range(200):
        nplanes = int(rng.integers(1, 40))
        scale = int(rng.choice([10, 1 << 20, 40 << 20, 200 << 20]))
        sizes = rng.integers(1, scale + 1, nplanes)
        gp = int(rng.choice([0, 1, 2, 5]))
        rows, cols = (int(v) for v in rng.choice([(1, 1), (100, 150), (3000, 4000), (9000, 9000)]))
        off = offsets(sizes, start=int(rng.integers(0, 1 << 40)))
        h, w = jpegx.band_shape_n(rows, cols, 1, 4)
        if nplanes * h * w > 2 ** 31 - 1:
            with pytest.raises(jpegx.JpegxError):
                jpegx.batch_groups_n(off, nplanes, rows, cols, 1, 4, gp)
            continue
        assert list(jpegx.batch_groups_n(off, nplanes, rows, cols, 1, 4, gp)) == restated(off, nplanes, h * w, gp), trial


def test_refusals_and_the_count_alone():
    with pytest.raises(jpegx.JpegxError, match="must not decrease"):
        jpegx.batch_groups_n(np.array([0, 9, 8, 20], np.uint64), 3, *SHAPE, 0)
    n = ctypes.c_int(-1)
    off = offsets([5] * 10)
    assert jpegx.lib().jpegx_batch_groups_n(off.ctypes.data, 10, *SHAPE, 3, None, ctypes.byref(n)) == 0 and n.value == 4
