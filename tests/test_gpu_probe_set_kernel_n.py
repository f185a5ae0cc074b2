"""jpegx_probe_sizes_set_n against the road it stands for, run once per candidate on the same float64 block strip
(tests/probe_set_device.py: jpegx_forward_fused_n on the strip + jpegx_entropy_sizes_n + the per-block sizes summed over each
plane's blocks from the table).  Every comparison is exact, and no cell may be flagged unless the case says which.

The sets are built for the one thing the ragged kernel adds, the plane of a block from the table: single-band pictures at
block_size 1 whose planes hold 1, 1, 1, 6, 35, 1, 2, 64, 65 and 3 blocks -- at dct_size 2 one turn of 64 blocks holds the first
five planes and a part of the sixth run of blocks, turns end inside planes and planes inside turns; from dct_size 16 on a turn is
one block -- and pictures of three bands, whose planes come in threes of one block count."""
import numpy as np
import pytest

import probe_set_device as psd
from test_gpu_probe_kernel_n import _planes

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 4, 7, 9, 16, 17, 24, 32]
COUNTS = [1, 1, 1, 6, 35, 1, 2, 64, 65, 3]
COUNTS3 = [2, 1, 7, 40, 1]                               # per band; three bands a picture
MANY = [float(v) for v in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128, 160, 200, 256, 300, 400, 512, 640, 800,
                           1000, 2000, 4096, 100000)]


def _strip(gpu, n, plane_counts, seed=0):
    """The four kinds of content of tests/test_gpu_probe_kernel_n.py in turn, plane by plane, as one strip."""
    return np.concatenate([psd.strip_of(_planes(gpu, n, 1, int(c), 1, seed=p + seed)[0], n) for p, c in enumerate(plane_counts)])


def _single(gpu, n, seed=0):
    return psd.SetStrip(gpu, _strip(gpu, n, COUNTS, seed), psd.sizes_for(COUNTS, n), 1, n)


def _triple(gpu, n, seed=0):
    return psd.SetStrip(gpu, _strip(gpu, n, np.repeat(COUNTS3, 3), seed), psd.sizes_for(COUNTS3, n), 3, n)


@pytest.fixture(scope="module", params=SIZES)
def sets(request, gpu):
    n = request.param
    devs = [_single(gpu, n), _triple(gpu, n, seed=1)]
    assert devs[0].counts().tolist() == COUNTS and devs[1].counts().tolist() == np.repeat(COUNTS3, 3).tolist()
    yield n, devs
    for d in devs:
        d.free()


def test_divide_candidates(sets):
    n, devs = sets
    for d in devs:
        d.check("divide", [40.0])
        got = d.check("divide", [1.0, 2.0, 3.0, 40.0, 64.0, 1000.0])       # power-of-two and true-division paths side by side
        assert (got >= d.counts()[:, None].astype(np.uint64)).all()      # a block is one byte at least
        # the all-zero planes (every fourth): one byte per block under every candidate
        zero = [p for p in range(d.nplanes) if (p + (1 if d.nbands == 3 else 0)) % 4 == 3]
        assert zero and (got[zero] == d.counts()[zero, None].astype(np.uint64)).all()


def test_thirty_two_candidates_and_the_same_value_twice(sets):
    n, devs = sets
    assert len(MANY) == 32
    got = devs[0].check("divide", MANY)
    assert (got[:, -1] == devs[0].counts().astype(np.uint64)).all()       # everything quantised away
    got = devs[1].check("divide", [40.0, 3.0, 40.0])
    assert np.array_equal(got[:, 0], got[:, 2])


def test_discard_edges_and_none(sets):
    n, devs = sets
    for d in devs:
        got = d.check("discard", [0.0, 1.0, float(n), float(n + 1)])
        assert (got[:, 0] == d.counts().astype(np.uint64)).all() and np.array_equal(got[:, 2], got[:, 3])
    devs[0].check("none", [0.0])
    devs[1].check("none", [0.0])


def test_sub_ranges_write_their_own_rows_only(sets):
    """p0 > 0 and k < npictures: row 0 is band 0 of picture p0, k * nbands rows are written (over garbage), the canaries in front
    of and behind them stay (SetStrip.probe)."""
    n, devs = sets
    for d in devs:
        for p0, k in ((1, 1), (2, 3), (3, d.npictures - 3), (0, 2), (d.npictures - 1, 1)):
            d.check("divide", [3.0, 40.0], p0, k)
    devs[0].check("divide", MANY, 4, 5)                                 # the 35-block plane first, the 64 and 65 behind it


@pytest.mark.parametrize("n", [2, 4, 16])
def test_bit_63_for_exactly_one_plane_of_one_block(gpu, n):
    """One flat block of DC 20000.3 as the second of the three one-block planes: at dct_size 2 it shares a wave step (16 blocks)
    and a turn with clean blocks of five planes.  Bit 63 for exactly (plane 1, divisor 1); every other total exact, plane 1
    under divisor 1000 among them."""
    strip = _strip(gpu, n, COUNTS)
    strip[n:2 * n] = 20000.3 / (n * n)
    d = psd.SetStrip(gpu, strip, psd.sizes_for(COUNTS, n), 1, n)
    try:
        want, want_bad = d.yardstick("divide", [1.0, 1000.0])
        assert np.argwhere(want_bad).tolist() == [[1, 0]]
        d.check("divide", [1.0, 1000.0], expect_bad=[(1, 0)])
        d.check("divide", [1.0, 1000.0], 1, 2, expect_bad=[(1, 0)])
        d.check("divide", [1.0, 1000.0], 2, 4)
    finally:
        d.free()


def test_explicit_device_form(gpu):
    d = _triple(gpu, 4)
    try:
        got, bad = d.probe("divide", [3.0, 40.0], 1, 3, device=0)
        want, want_bad = d.yardstick("divide", [3.0, 40.0])
        assert not bad.any() and not want_bad.any() and np.array_equal(got, want[3:12])
    finally:
        d.free()


@pytest.mark.parametrize("n", [2, 7, 17])
def test_a_set_of_equal_pictures_gives_the_totals_of_the_equal_size_probe(gpu, n):
    planes = _planes(gpu, n, 2, 3, 12, seed=2)                           # 4 pictures of 3 bands, planes of 2 x 3 blocks
    strip = np.concatenate([psd.strip_of(p, n) for p in planes])
    d = psd.SetStrip(gpu, strip, [(2 * n, 3 * n)] * 4, 3, n)
    dplanes, dtot = gpu.DeviceBuffer(planes.nbytes), gpu.DeviceBuffer(12 * 3 * 8)
    try:
        dplanes.upload(np.ascontiguousarray(planes))
        gpu.probe_sizes_n_device(dplanes.ptr, 12, 2 * n, 3 * n, n, "divide", [1.0, 3.0, 40.0], dtot.ptr)
        gpu.check(gpu.lib().jpegx_stream_synchronize(None))
        equal = dtot.download((12, 3), np.uint64)
        got = d.check("divide", [1.0, 3.0, 40.0])
        assert np.array_equal(got, equal)
    finally:
        dplanes.free()
        dtot.free()
        d.free()
