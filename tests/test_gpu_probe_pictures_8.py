"""jpegx.batch_probe_pictures and jpegx.batch_probe_distortion_pictures from pixels, against the roads they stand for run once
per candidate: the plane index of a sizes-only jpegx_batch_compress_pictures, and jpegx_batch_compress_pictures ->
jpegx_batch_decompress_pictures -> a comparison with the coded bands.  Every comparison is exact.  block_size 1, 2 and 4 at 64
columns put the compression on its uint8 road, block_size 3, 5 and the ragged 37 x 53 on its float64 road; the probes are on
the float64 road throughout.  Five pictures in groups of one and two (group_planes 3 and 6 of 15 planes) and in one group."""
import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu

# block_size, rows, cols, divisors
CONFIGS = [(1, 64, 64, [1, 3, 40, 64]), (2, 64, 64, [1, 7, 40]), (4, 64, 64, [1, 2, 1000]), (3, 64, 64, [1, 3, 40]), (5, 70, 61, [2, 40]),
           (1, 37, 53, [1, 2, 3, 7, 40, 1000]), (4, 37, 53, [1, 40])]


def _pixels(count, rows, cols, seed=3):
    """Pictures of unlike content: a smooth half and a noisy half, a flat one, a ramp."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    out = np.empty((count, rows, cols, 3), np.uint8)
    for p in range(count):
        smooth = ((yy * (2 + p) + xx * 3) // 2 % 256)[..., None] + np.arange(3) * 17
        noise = rng.integers(0, 256, (rows, cols, 3))
        out[p] = (np.where((xx < cols // 2)[..., None], smooth, noise) if p % 3 != 1 else np.full((rows, cols, 3), 40 + 30 * p)) % 256
    return out


def _sizes_only(gpu, pixels, bs, params, flag):
    """uint64 [k][3][K] from K sizes-only compressions: the plane index, plane by plane."""
    k, rows, cols, nb = pixels.shape
    h, w = gpu.padded_shape(rows, cols, bs)
    gp = gpu.batch_group_planes_pictures_n(nb, rows, cols, bs, 8) or nb
    sizes = np.zeros((k, nb, len(params)), np.uint64)
    din, dws = gpu.DeviceBuffer(pixels.nbytes), gpu.DeviceBuffer(gpu.batch_pictures_workspace_bytes(k, nb, rows, cols, bs, gp))
    try:
        din.upload(pixels)
        for q, param in enumerate(params):
            gpu.batch_compress_pictures_device(din.ptr, k, nb, rows, cols, bs, dws.ptr, None, 0, gp, "divide", param, flag)
            rc, total, off = gpu.batch_compress_status(dws.ptr, k * nb, h, w)
            assert rc == 0 and int(off[-1]) == total
            sizes[:, :, q] = np.diff(off).reshape(k, nb)
    finally:
        din.free()
        dws.free()
    return sizes


def _round_trip_sse(gpu, pixels, bs, params, colour):
    """int64 [k][3][K]: compress, decompress into the coded bands, compare with them."""
    k, rows, cols, nb = pixels.shape
    coded = pixels if colour is None else np.stack([np.asarray(Image.fromarray(p, mode="RGB").convert("YCbCr")) for p in pixels])
    sse = np.zeros((k, nb, len(params)), np.int64)
    for q, param in enumerate(params):
        blobs = gpu.batch_compress_pictures(pixels, bs, "divide", param, colour=colour)
        back = gpu.batch_decompress_pictures(blobs, rows, cols, bs, "divide", param)          # the coded bands as they are
        sse[:, :, q] = ((back.astype(np.int64) - coded.astype(np.int64)) ** 2).sum(axis=(1, 2))
    return sse


@pytest.fixture(scope="module")
def yardsticks(gpu):
    """The roads once per (configuration, colour), shared by the tests below and left unchanged."""
    cache = {}

    def get(config, colour):
        key = (tuple(config[:3]), colour)
        if key not in cache:
            bs, rows, cols, divisors = config
            pixels = _pixels(5, rows, cols)
            params = [float(d) for d in divisors]
            cache[key] = (pixels, _sizes_only(gpu, pixels, bs, params, 0 if colour is None else 1), _round_trip_sse(gpu, pixels, bs, params, colour))
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]
    return get


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("config", CONFIGS, ids=["bs%d-%dx%d" % c[:3] for c in CONFIGS])
def test_sizes_are_the_plane_index_of_the_sizes_only_compression(gpu, yardsticks, config, colour):
    bs, rows, cols, divisors = config
    pixels, want, _ = yardsticks(config, colour)
    for gp in (3, 6, None):
        got, bad = gpu.batch_probe_pictures(pixels, bs, "divide", divisors, colour=colour, group_planes=gp)
        assert got.shape == (5, 3, len(divisors)) and not bad.any()
        assert np.array_equal(got, want), (gp, got.tolist(), want.tolist())
    one, _ = gpu.batch_probe_pictures(pixels[1:2], bs, "divide", divisors[-1:], colour=colour)
    assert np.array_equal(one, want[1:2, :, -1:])


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("config", CONFIGS, ids=["bs%d-%dx%d" % c[:3] for c in CONFIGS])
def test_distortion_is_the_round_trip(gpu, yardsticks, config, colour):
    bs, rows, cols, divisors = config
    pixels, _, want = yardsticks(config, colour)
    for gp in (3, None):
        got, bad = gpu.batch_probe_distortion_pictures(pixels, bs, "divide", divisors, colour=colour, group_planes=gp)
        assert got.shape == (5, 3, len(divisors)) and not bad.any()
        assert np.array_equal(got.astype(np.int64), want), (gp, got.tolist(), want.tolist())
    assert want[0, :, -1].sum() > want[0, :, 0].sum()                      # content on which the divisor matters


def test_qtable_and_discard_from_pixels(gpu):
    """The entries take all four quantisers; the roads give the yardstick."""
    pixels = _pixels(2, 37, 53)
    for mode, param in (("qtable", 0.0), ("none", 0.0), ("discard", 2.0)):
        blobs = gpu.batch_compress_pictures(pixels, 2, mode, param)
        want = np.array([[len(b) for b in picture] for picture in blobs])
        back = gpu.batch_decompress_pictures(blobs, 37, 53, 2, mode, param)
        got, bad = gpu.batch_probe_pictures(pixels, 2, mode, [param])
        assert not bad.any() and np.array_equal(got[:, :, 0], want), mode
        sse, bad = gpu.batch_probe_distortion_pictures(pixels, 2, mode, [param])
        assert not bad.any() and np.array_equal(sse[:, :, 0].astype(np.int64), ((back.astype(np.int64) - pixels) ** 2).sum(axis=(1, 2))), mode


def test_a_divisor_below_the_code_range_raises_bit_63(gpu):
    """Divisor 0.5 on a white picture: 64 * 255 / 0.5 is beyond 16383 in every band; the grey picture beside it stays clean."""
    pixels = np.stack([np.full((16, 16, 3), 255, np.uint8), np.full((16, 16, 3), 100, np.uint8)])
    got, bad = gpu.batch_probe_pictures(pixels, 1, "divide", [0.5, 1.0])
    assert bad[:, :, 0].tolist() == [[True] * 3, [False] * 3] and not bad[:, :, 1].any()
    assert (got[:, :, 1] == 4 * 4).all()                                 # 16320 and 6400: one DC code and the end marker, 4 bytes a block
    sse, bad2 = gpu.batch_probe_distortion_pictures(pixels, 1, "divide", [0.5, 1.0])
    assert np.array_equal(bad2, bad) and (sse[:, :, 1] == 0).all() and (sse[1] == 0).all()
