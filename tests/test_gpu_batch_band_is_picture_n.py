"""GPU: a stack of one-band pictures IS a stack of bands.  jpegx_batch_compress_n and jpegx_batch_compress_pictures_n with
nbands = 1 and colour = 0 run the same group walk (csrc/jpegx_batch_n.cpp: compress_stack, decompress_stack), differing in the
gather and the scatter alone, so their total, plane offsets and bytes are equal, jpegx_batch_decompress_n and
jpegx_batch_decompress_pictures_n give the same samples, and both are compress_band_n / decompress_band_n band by band.
Every comparison is exact.

The shape: 5 bands of 10 x 13 with group_planes 2, so the groups are 2, 2 and a short last one of 1; once at block_size 2,
dct_size 4 with 'divide' 3.0 (pooling, both paddings, several blocks to a wave) and once at block_size 1, dct_size 16 with
'none' (one block to a plane, a block longer than a wave).  The transform is un-normalised and 'none' keeps every amplitude,
so a 16 x 16 block of samples up to 255 would pass 15 bits (BadRleCodeError, on every road alike): that case's samples stay
below 48, whose 256-sample sums stay below 2^14."""
import numpy as np
import pytest

from batch_n_dev import noise_bands

pytestmark = pytest.mark.gpu

NBANDS, ROWS, COLS, GROUP_PLANES = 5, 10, 13, 2
# (block_size, dct_size, quantiser, parameter, samples below)
CASES = [(2, 4, "divide", 3.0, 256), (1, 16, "none", 0.0, 48)]


def coded(gpu, dev, compress, shape, dws, gp):
    """(rc, total, offsets, bytes) of one road: sizes-only compress, status, emit into exactly the total, status."""
    compress(None, 0)
    rc, total, _ = gpu.batch_compress_status_n(dws.ptr, *shape, gp)
    assert rc == 0 and total > 0
    dout = dev(total)
    gpu.batch_emit_n_device(dws.ptr, *shape, dout.ptr, total, gp)
    rc, total2, off = gpu.batch_compress_status_n(dws.ptr, *shape, gp)
    return rc, total2, off, dout.download((total,), np.uint8)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "bs%d-N%d-%s%g" % c[:4])
def roads(gpu, request):
    """Both roads there and back and the per-band reference, made once per case."""
    bs, n, mode, param, below = request.param
    bands = (noise_bands([NBANDS, bs, n], NBANDS, ROWS, COLS, smooth_every=3).astype(np.int32) % below).astype(np.uint8)
    blobs = [gpu.compress_band_n(b, bs, n, mode, param) for b in bands]
    samples = np.stack([gpu.decompress_band_n(b, ROWS, COLS, bs, n, mode, param) for b in blobs])
    shape, pics = (NBANDS, ROWS, COLS, bs, n), (NBANDS, 1, ROWS, COLS, bs, n)
    held = []

    def dev(nbytes):
        held.append(gpu.DeviceBuffer(nbytes))
        return held[-1]
    try:
        din = dev(bands.nbytes)
        din.upload(bands)                                   # [5][10][13] bands are [5][10][13][1] pictures, byte for byte
        ws = [dev(gpu.batch_workspace_bytes_n(*shape, GROUP_PLANES)) for _ in range(2)]
        as_bands = coded(gpu, dev, lambda d_out, cap: gpu.batch_compress_n_device(din.ptr, *shape, ws[0].ptr, d_out, cap, mode, param, GROUP_PLANES),
                         shape, ws[0], GROUP_PLANES)
        as_pictures = coded(gpu, dev, lambda d_out, cap: gpu.batch_compress_pictures_n_device(din.ptr, *pics, ws[1].ptr, d_out, cap, GROUP_PLANES, mode,
                                                                                             param, 0), shape, ws[1], GROUP_PLANES)
        rc, total, off, stream = as_bands
        dbytes = dev(total)
        dbytes.upload(stream)
        back = []
        for nws, decompress in (
                (gpu.batch_decompress_workspace_bytes_n(total, *shape, GROUP_PLANES),
                 lambda w, o: gpu.batch_decompress_n_device(dbytes.ptr, off, *shape, w, o, COLS, mode, param, GROUP_PLANES)),
                (gpu.batch_decompress_pictures_workspace_bytes_n(total, *pics, GROUP_PLANES),
                 lambda w, o: gpu.batch_decompress_pictures_n_device(dbytes.ptr, off, *pics, w, o, GROUP_PLANES, COLS, mode, param, 0))):
            dws, dout = dev(nws), dev(bands.nbytes)
            decompress(dws.ptr, dout.ptr)
            back.append((nws, dout.download((NBANDS, ROWS, COLS), np.uint8)))
    finally:
        for buf in held:
            buf.free()
    return dict(bands=bands, blobs=blobs, samples=samples, as_bands=as_bands, as_pictures=as_pictures, back=back, shape=shape, pics=pics)


def test_the_groups_are_two_two_and_a_short_one(gpu, roads):
    off = roads["as_bands"][2]
    assert gpu.batch_groups_n(off, *roads["shape"], GROUP_PLANES).tolist() == [0, 2, 4, 5]
    assert gpu.batch_groups_pictures_n(off, *roads["pics"], GROUP_PLANES).tolist() == [0, 2, 4, 5]


def test_both_compress_roads_give_the_same_total_offsets_and_bytes(roads):
    (rc_b, total_b, off_b, bytes_b), (rc_p, total_p, off_p, bytes_p) = roads["as_bands"], roads["as_pictures"]
    assert rc_b == 0 and rc_p == 0
    assert total_b == total_p
    assert np.array_equal(off_b, off_p)
    assert np.array_equal(bytes_b, bytes_p)


def test_the_bytes_are_the_per_band_road_s(roads):
    for rc, total, off, stream in (roads["as_bands"], roads["as_pictures"]):
        assert total == sum(len(b) for b in roads["blobs"]) and int(off[0]) == 0 and int(off[-1]) == total
        for p, blob in enumerate(roads["blobs"]):
            assert stream[int(off[p]):int(off[p + 1])].tobytes() == blob, "band %d" % p


def test_both_decompress_roads_give_the_same_samples_and_the_per_band_road_s(roads):
    (nws_b, back_b), (nws_p, back_p) = roads["back"]
    assert nws_b == nws_p > 0
    assert np.array_equal(back_b, back_p)
    assert np.array_equal(back_b, roads["samples"])
