"""jpegx_batch_groups_set_n, the cut of a coded set of pictures of unequal sizes into decoding groups ON PICTURE BOUNDARIES,
against a Python restatement of its rule on synthetic plane offsets.  Host arithmetic only: CPU."""
import ctypes

import numpy as np
import pytest

import jpegx

GROUP_BYTES = 64 << 20
GROUP_SAMPLES = 1 << 26
MAX_STREAM = 2 ** 32 - 4096
MIB = 1 << 20


def restated(off, samples, nbands, group_samples):
    """From the first picture not yet taken: whole pictures while the group's samples stay within group_samples (0: 2^26) and
    its bytes within 64 MiB; one picture at least.  samples[p] = nbands * H_p * W_p."""
    limit = group_samples or GROUP_SAMPLES
    n = len(samples)
    first, p0 = [], 0
    while p0 < n:
        p1 = p0 + 1
        while p1 < n and sum(samples[p0:p1 + 1]) <= limit and int(off[(p1 + 1) * nbands]) - int(off[p0 * nbands]) <= GROUP_BYTES:
            p1 += 1
        first.append(p0)
        p0 = p1
    return first + [n]


def offsets(sizes, start=0):
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[0] = start
    off[1:] = start + np.cumsum(np.asarray(sizes, np.uint64))
    return off


def samples_of(table, n):
    e = table.entries
    return [int(e["first"][p + 1] - e["first"][p]) * n * n for p in range(table.npictures)]


def test_cuts_by_samples_on_picture_boundaries_with_a_short_last_group():
    """Pictures of 40 x 56 (3 * 2240 samples at N 4) and of 100 x 152 (3 * 15200): groups of at most 60 000 samples."""
    sizes = [(40, 56)] * 5 + [(100, 150)] * 3 + [(40, 56)] * 9
    t = jpegx.picture_set_table(sizes, 3, 1, 4)
    samples = samples_of(t, 4)
    assert samples[0] == 3 * 2240 and samples[5] == 3 * 15200
    off = offsets(np.random.default_rng(1).integers(1000, 5000, 3 * len(sizes)), start=12345)
    got = list(jpegx.batch_groups_set_n(off, t, 60000))
    assert got == restated(off, samples, 3, 60000) == [0, 5, 6, 7, 10, 17]
    # a lone picture above the samples limit is a group of its own; 0 is 2^26: one group
    assert list(jpegx.batch_groups_set_n(off, t, 1)) == list(range(len(sizes) + 1))
    assert list(jpegx.batch_groups_set_n(off, t, 0)) == [0, len(sizes)] == list(jpegx.batch_groups_set_n(off, t))
    assert list(jpegx.batch_groups_set_n(off, t, 45600 + 6720)) == restated(off, samples, 3, 45600 + 6720)


def test_the_64_mib_cut_never_splits_a_picture():
    """Four pictures of three bands; the 64 MiB cap falls inside picture 1 (after its first band) and inside picture 3."""
    t = jpegx.picture_set_table([(100, 150), (64, 64), (8, 8), (300, 20)], 3, 1, 4)
    sizes = [20 * MIB, 20 * MIB, 10 * MIB,   10 * MIB, 10 * MIB, 30 * MIB,   1, 1, 1,   30 * MIB, 30 * MIB, 30 * MIB]
    off = offsets(sizes, start=7)
    got = list(jpegx.batch_groups_set_n(off, t))
    assert got == restated(off, samples_of(t, 4), 3, 0) == [0, 1, 3, 4]
    assert [int(off[3 * b]) - int(off[3 * a]) for a, b in zip(got, got[1:])] == [50 * MIB, 50 * MIB + 3, 90 * MIB]
    # 64 MiB exactly stays one group
    sizes = [32 * MIB, 16 * MIB, 16 * MIB - 3,   1, 1, 1,   1, 5, 5,   1, 1, 1]
    assert list(jpegx.batch_groups_set_n(offsets(sizes), t)) == [0, 2, 4]
    sizes[0] += 1
    assert list(jpegx.batch_groups_set_n(offsets(sizes), t)) == [0, 1, 4]


def test_a_lone_picture_above_64_mib_passes_and_one_at_the_decode_limit_does_not():
    t = jpegx.picture_set_table([(10, 10), (20, 30), (5, 70)], 3, 2, 3)
    big = [1 << 30, 1 << 30, 1 << 30]                    # 3 GiB in one picture
    assert list(jpegx.batch_groups_set_n(offsets([10, 10, 10] + big + [10, 10, 10]), t)) == [0, 1, 2, 3]
    edge = [1 << 31, (1 << 31) - 4096 - 2, 1]            # 2^32 - 4096 - 1 bytes: the last admitted
    assert sum(edge) == MAX_STREAM - 1
    assert list(jpegx.batch_groups_set_n(offsets([10, 10, 10] + edge + [7, 7, 7]), t)) == [0, 1, 2, 3]
    edge[2] += 1                                          # 2^32 - 4096 bytes: refused, and the picture is named
    with pytest.raises(jpegx.JpegxError, match="picture 1 holds %d bytes" % MAX_STREAM):
        jpegx.batch_groups_set_n(offsets([10, 10, 10] + edge + [7, 7, 7]), t)


def test_random_sets_against_the_restatement():
    rng = np.random.default_rng(2)
    for trial in range(200):
        nbands = int(rng.integers(1, 5))
        npictures = int(rng.integers(1, 15))
        n = int(rng.choice([2, 3, 4, 16]))
        sizes = [(int(r), int(c)) for r, c in rng.integers(1, 200, (npictures, 2))]
        t = jpegx.picture_set_table(sizes, nbands, int(rng.integers(1, 4)), n)
        scale = int(rng.choice([10, 1 << 20, 20 << 20, 70 << 20]))
        off = offsets(rng.integers(1, scale + 1, npictures * nbands), start=int(rng.integers(0, 1 << 40)))
        gs = int(rng.choice([0, 1, 5000, 40000, 200000]))
        got = list(jpegx.batch_groups_set_n(off, t, gs))
        assert got == restated(off, samples_of(t, n), nbands, gs), trial
        assert got[0] == 0 and got[-1] == npictures and all(b > a for a, b in zip(got, got[1:]))


def test_refusals_and_the_count_alone():
    t = jpegx.picture_set_table([(10, 10), (20, 30)], 3, 1, 4)
    with pytest.raises(jpegx.JpegxError, match="must not decrease"):
        jpegx.batch_groups_set_n(np.array([0, 9, 8, 20, 30, 40, 50], np.uint64), t)
    with pytest.raises(jpegx.JpegxError, match="group_samples"):
        jpegx.batch_groups_set_n(offsets([5] * 6), t, -1)
    with pytest.raises(jpegx.JpegxError, match="nbands"):
        jpegx.batch_groups_set_n(offsets([5] * 5), t)
    L = jpegx.lib()
    n = ctypes.c_int(-1)
    off = offsets([5] * 6)
    assert L.jpegx_batch_groups_set_n(off.ctypes.data, t.ptr, 1, None, ctypes.byref(n)) == 0 and n.value == 2
    assert L.jpegx_batch_groups_set_n(None, t.ptr, 0, None, ctypes.byref(n)) == -1
    assert L.jpegx_batch_groups_set_n(off.ctypes.data, None, 0, None, ctypes.byref(n)) == -1
    assert L.jpegx_batch_groups_set_n(off.ctypes.data, t.ptr, 0, None, None) == -1
    junk = np.zeros(64, np.uint64)
    assert L.jpegx_batch_groups_set_n(off.ctypes.data, junk.ctypes.data, 0, None, ctypes.byref(n)) == -1 and b"table" in L.jpegx_last_error()
