"""GPU: the three kernels of the picture set for dct_size != 8 alone, against NumPy.

jpegx_picture_set_blocks_n: the float64 block strip must be tests/picture_set_model.py's strip_twin -- per picture and band the
package's Padding, SubSampling and DCTPadding, cut into blocks in strip order, with colour 1 of the picture's YCbCr as
tests/colour_model.py gives it -- whatever stands in the gaps between the pictures and behind every input row.
jpegx_picture_set_pixels_u8: every picture's pixels must be pixels_twin of the strip, exactly cols * nbands bytes per row:
the pitch slack, the gaps between the pictures and both fences keep their canaries.
jpegx_internal_entropy_plane_index_ragged: the host sum of jpegx_entropy_block_sizes over each plane's blocks.

The sets are the smallest that reach each mechanism: pictures of one block next to pictures of 5 x 13 blocks, ragged sizes
(neither axis a multiple of bs * N), a picture of 1 x 1 pixel, 67 and 130 pictures (the search passes 64 and 128 entries and
waves straddle pictures), 1100 pictures (the prefix no longer fits the workgroup's LDS and the search reads the table), odd
pitches, unaligned offsets, and a sub-range of a larger table."""
import ctypes

import numpy as np
import pytest

from batch_n_dev import CANARY, Fenced, band_shape
from picture_set_model import Layout, noise_pictures, pixels_twin, strip_twin, table_twin

pytestmark = pytest.mark.gpu

# (nbands, colour)
BANDS = [(1, 0), (3, 0), (3, 1)]


def mixed_sizes(n, bs):
    """One-block pictures next to 5 x 13-block ones, exact and ragged, and a picture of one pixel."""
    return [band_shape(1, 1, n, bs, False), band_shape(5, 13, n, bs, True), (1, 1), band_shape(1, 1, n, bs, True), band_shape(5, 13, n, bs, False),
            band_shape(2, 1, n, bs, True), band_shape(1, 3, n, bs, True)]


def many_sizes(count, n, bs, seed):
    """`count` pictures of one to four blocks a band, every size ragged in its own way."""
    rng = np.random.default_rng([seed, count, n, bs])
    return [(int(r), int(c)) for r, c in zip(rng.integers(1, 2 * n * bs + 1, count), rng.integers(1, 2 * n * bs + 1, count))]


def upload_table(gpu, table):
    d = gpu.DeviceBuffer(table.nbytes)
    d.upload(table.blob.view(np.uint8)[:table.nbytes])
    return d


def run_gather(gpu, sizes, nb, colour, bs, n, seed, p0=0, k=None):
    k = len(sizes) - p0 if k is None else k
    pictures = noise_pictures(seed, sizes, nb)
    lay = Layout(sizes, nb, seed=seed)
    table = gpu.picture_set_table(sizes, nb, bs, n, offsets=lay.offsets, pitches=lay.pitches)
    first = table.entries["first"]
    nblk = int(first[p0 + k] - first[p0])
    din = Fenced(gpu, lay.nbytes, skew=1)                 # the pixels need no alignment
    dout = Fenced(gpu, int(table.total_blocks) * n * n * 8)
    dtab = upload_table(gpu, table)
    try:
        din.upload(lay.pack(pictures, 0xEE))              # poisoned gaps and pitch slack
        gpu.picture_set_blocks_n_device(din.ptr, table, dtab.ptr, p0, k, dout.ptr, colour=colour)
        got = dout.payload(nblk * n * n * 8, "gather").view(np.float64).reshape(nblk * n, n)
        want = strip_twin(pictures[p0:p0 + k], bs, n, colour)
        assert got.shape == want.shape
        assert np.array_equal(got, want), "blocks %s differ" % np.unique(np.nonzero(got != want)[0] // n)[:8]
    finally:
        din.free()
        dout.free()
        dtab.free()


def run_scatter(gpu, sizes, nb, colour, bs, n, seed, p0=0, k=None):
    k = len(sizes) - p0 if k is None else k
    lay = Layout(sizes, nb, seed=seed, lead=5)
    table = gpu.picture_set_table(sizes, nb, bs, n, offsets=lay.offsets, pitches=lay.pitches)
    first = table.entries["first"]
    nblk = int(first[p0 + k] - first[p0])
    strip = np.random.default_rng([seed, n, bs, nb]).integers(0, 256, (nblk * n, n), dtype=np.uint8)
    din = Fenced(gpu, strip.nbytes, skew=3)
    dout = Fenced(gpu, lay.nbytes, skew=1)
    dtab = upload_table(gpu, table)
    try:
        din.upload(strip)
        gpu.picture_set_pixels_u8_device(din.ptr, table, dtab.ptr, p0, k, dout.ptr, colour=colour)
        buf = dout.payload(dout.nbytes, "scatter")
        got, mask = lay.unpack(buf)
        want = pixels_twin(strip, sizes[p0:p0 + k], nb, bs, n, colour)
        for q in range(k):
            assert np.array_equal(got[p0 + q], want[q]), "picture %d" % (p0 + q)
        # nothing but the k pictures' own bytes: the pitch slack, the gaps and the other pictures keep the canary
        part = Layout.__new__(Layout)
        part.sizes, part.nbands, part.offsets, part.pitches, part.nbytes = sizes[p0:p0 + k], nb, lay.offsets[p0:p0 + k], lay.pitches[p0:p0 + k], lay.nbytes
        _, written = part.unpack(buf)
        assert np.all(buf[~written] == CANARY), "bytes outside the pictures were written"
    finally:
        din.free()
        dout.free()
        dtab.free()


@pytest.mark.parametrize("nb,colour", BANDS, ids=["nb%d-colour%d" % b for b in BANDS])
@pytest.mark.parametrize("bs", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [2, 3, 5, 12, 24, 32])
def test_gather_on_mixed_sizes(gpu, n, bs, nb, colour):
    run_gather(gpu, mixed_sizes(n, bs), nb, colour, bs, n, seed=n * 100 + bs)


@pytest.mark.parametrize("nb,colour", BANDS, ids=["nb%d-colour%d" % b for b in BANDS])
@pytest.mark.parametrize("bs", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [2, 3, 5, 12, 24, 32])
def test_scatter_on_mixed_sizes(gpu, n, bs, nb, colour):
    run_scatter(gpu, mixed_sizes(n, bs), nb, colour, bs, n, seed=n * 100 + bs)


MANY = [(67, 2, 1, 3, 0), (67, 5, 3, 3, 1), (130, 3, 2, 3, 1), (130, 12, 1, 1, 0), (130, 2, 5, 2, 0), (67, 4, 1, 4, 0), (1100, 2, 1, 3, 1), (1100, 3, 2, 1, 0)]


@pytest.mark.parametrize("count,n,bs,nb,colour", MANY, ids=["p%d-N%d-bs%d-nb%d-colour%d" % m for m in MANY])
def test_both_on_many_small_pictures(gpu, count, n, bs, nb, colour):
    sizes = many_sizes(count, n, bs, 7)
    run_gather(gpu, sizes, nb, colour, bs, n, seed=count)
    run_scatter(gpu, sizes, nb, colour, bs, n, seed=count)


@pytest.mark.parametrize("p0,k", [(0, 1), (3, 2), (6, 1), (2, 5), (60, 70), (1, 1090)])
def test_a_sub_range_of_a_larger_table(gpu, p0, k):
    n, bs = 4, 2
    sizes = mixed_sizes(n, bs) if p0 + k <= 7 else many_sizes(130 if p0 + k <= 130 else 1100, n, bs, 9)
    for nb, colour in ((3, 1), (1, 0)):
        run_gather(gpu, sizes, nb, colour, bs, n, seed=p0, p0=p0, k=k)
        run_scatter(gpu, sizes, nb, colour, bs, n, seed=p0, p0=p0, k=k)


def ragged_index(gpu, nplanes, d_first, nblocks, dws, dindex, cap):
    L = gpu.lib()
    fn = L.jpegx_internal_entropy_plane_index_ragged
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn(nplanes, d_first, nblocks, dws, dindex, cap, None)


@pytest.mark.parametrize("n,counts", [(2, [1, 1, 62, 1, 63, 64, 65, 200, 3, 1]), (5, [7] * 40 + [130, 1, 1]), (3, [5000, 1, 4097 * 64 + 3, 17, 64, 1])],
                         ids=["N2", "N5", "N3-past-one-scan-chunk"])
def test_the_ragged_plane_index(gpu, n, counts):
    """Planes of the given block counts, so that plane starts are no multiples of 64 and waves straddle planes: every offset
    is the host's running sum of the block sizes, the last the total, and the head holds the capacity."""
    L = gpu.lib()
    nblocks, nplanes = sum(counts), len(counts)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rng = np.random.default_rng([n, nplanes])
    zz = (rng.integers(-300, 301, (nblocks, n * n)) * (rng.random((nblocks, n * n)) < 0.3)).astype(np.int32)
    dzz, dws = gpu.DeviceBuffer(zz.nbytes), gpu.DeviceBuffer(L.jpegx_entropy_workspace_bytes_n(nblocks, n * n))
    dfirst, dindex = gpu.DeviceBuffer(first.nbytes), Fenced(gpu, 16 + 8 * (nplanes + 1))
    try:
        dzz.upload(zz)
        dfirst.upload(first)
        gpu.check(L.jpegx_entropy_sizes_n(dzz.ptr, nblocks, n * n, dws.ptr, None), "jpegx_entropy_sizes_n")
        sizes = np.zeros(nblocks, np.uint32)
        gpu.check(L.jpegx_entropy_block_sizes(dws.ptr, nblocks, sizes.ctypes.data, None), "jpegx_entropy_block_sizes")
        want = np.concatenate([[0], np.cumsum(sizes.astype(np.uint64))])[first]
        assert ragged_index(gpu, nplanes, dfirst.ptr, nblocks, dws.ptr, dindex.ptr, 12345) == 0
        gpu.check(L.jpegx_device_synchronize())
        got = dindex.payload(dindex.nbytes, "ragged plane index").view(np.uint64)
        assert got[0] == 12345 and got[1] == 0
        assert np.array_equal(got[2:], want.astype(np.uint64))
        # refusals before any launch
        assert ragged_index(gpu, 0, dfirst.ptr, nblocks, dws.ptr, dindex.ptr, 0) == -1
        assert ragged_index(gpu, nplanes, None, nblocks, dws.ptr, dindex.ptr, 0) == -1
        assert ragged_index(gpu, nplanes, dfirst.ptr + 4, nblocks, dws.ptr, dindex.ptr, 0) == -1
        assert ragged_index(gpu, nplanes, dfirst.ptr, nplanes - 1, dws.ptr, dindex.ptr, 0) == -1
    finally:
        dzz.free()
        dws.free()
        dfirst.free()
        dindex.free()


def test_a_table_of_equal_sizes_is_the_stacked_gather_in_strip_order(gpu):
    """Four pictures of one size: the strip holds the blocks of jpegx_band_planes_packed_stacked_n's planes, plane after plane."""
    n, bs, nb, k = 12, 3, 3, 4
    rows, cols = band_shape(2, 3, n, bs, True)
    px = np.random.default_rng(5).integers(0, 256, (k, rows, cols, nb), dtype=np.uint8)
    h, w = gpu.band_shape_n(rows, cols, bs, n)
    table = gpu.picture_set_table([(rows, cols)] * k, nb, bs, n)
    assert table_twin([(rows, cols)] * k, nb, bs, n)[2][-1] == table.total_blocks == k * nb * 6
    din, dplanes, dstrip = gpu.DeviceBuffer(px.nbytes), gpu.DeviceBuffer(k * nb * h * w * 8), gpu.DeviceBuffer(k * nb * h * w * 8)
    dtab = upload_table(gpu, table)
    try:
        din.upload(px)
        for colour in (0, 1):
            gpu.band_planes_packed_stacked_n_device(din.ptr, k, nb, rows, cols, bs, n, dplanes.ptr, colour=colour)
            gpu.picture_set_blocks_n_device(din.ptr, table, dtab.ptr, 0, k, dstrip.ptr, colour=colour)
            planes = dplanes.download((k * nb, h // n, n, w // n, n), np.float64)
            strip = dstrip.download((k * nb, h // n, w // n, n, n), np.float64)
            assert np.array_equal(strip, planes.transpose(0, 1, 3, 2, 4))
    finally:
        for d in (din, dplanes, dstrip, dtab):
            d.free()
