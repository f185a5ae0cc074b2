"""jpegx.batch_probe_pictures_n against the plane offsets of the sizes-only batch compression
(batch_compress_pictures_n_device with d_out None + batch_compress_status_n), called once per candidate.  Exact equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _pixels(count, rows, cols, nb, seed=3):
    """Pictures of unlike content: a smooth half and a noisy half, a flat one, a ramp."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    out = np.empty((count, rows, cols, nb), np.uint8)
    for p in range(count):
        smooth = ((yy * (2 + p) + xx * 3) // 2 % 256)[..., None] + np.arange(nb) * 17
        noise = rng.integers(0, 256, (rows, cols, nb))
        out[p] = (np.where((xx < cols // 2)[..., None], smooth, noise) if p % 3 != 1 else np.full((rows, cols, nb), 40 + 30 * p)) % 256
    return out


def _yardstick(gpu, pixels, bs, n, mode, params, colour, group_planes):
    """sizes uint64 [k][nb][K] and a bool per candidate (the batch's BadRleCodeError verdict) from K sizes-only compressions."""
    k, rows, cols, nb = pixels.shape
    planes = (k * nb, rows, cols, bs, n)
    sizes, refused = np.zeros((k, nb, len(params)), np.uint64), np.zeros(len(params), bool)
    din, dws = gpu.DeviceBuffer(pixels.nbytes), gpu.DeviceBuffer(gpu.batch_workspace_bytes_n(*planes, group_planes))
    try:
        din.upload(pixels)
        for q, param in enumerate(params):
            gpu.batch_compress_pictures_n_device(din.ptr, k, nb, rows, cols, bs, n, dws.ptr, None, 0, group_planes, mode, param, colour)
            rc, total, off = gpu.batch_compress_status_n(dws.ptr, *planes, group_planes)
            refused[q] = rc != 0
            if rc == 0:
                assert int(off[-1]) == total
                sizes[:, :, q] = np.diff(off).reshape(k, nb)
            else:
                assert "BadRleCodeError" in gpu.lib().jpegx_last_error().decode()
    finally:
        din.free()
        dws.free()
    return sizes, refused


CONFIGS = [(1, 4, 40, 48, [1, 3, 40, 64]), (2, 3, 40, 48, [1, 3, 40, 64]), (1, 16, 40, 48, [8, 24, 64, 1000]), (5, 24, 130, 125, [8, 40, 1000]),
           (1, 4, 37, 45, [1, 3, 40, 64]), (2, 3, 37, 45, [2, 1000]), (1, 16, 37, 45, [8, 40])]


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, n, rows, cols, divisors", CONFIGS)
def test_pictures_against_the_sizes_only_compression(gpu, bs, n, rows, cols, divisors, colour):
    flag = 0 if colour is None else 1
    for count in (1, 2, 5):
        pixels = _pixels(count, rows, cols, 3)
        recommended = gpu.batch_group_planes_pictures_n(3, rows, cols, bs, n)
        want, refused = _yardstick(gpu, pixels, bs, n, "divide", divisors, flag, recommended)
        assert not refused.any()
        got, bad = gpu.batch_probe_pictures_n(pixels, bs, n, "divide", divisors, colour=colour)
        assert got.dtype == np.uint64 and got.shape == (count, 3, len(divisors)) and bad.dtype == bool and not bad.any()
        assert np.array_equal(got, want), (count, got, want)
        one, bad_one = gpu.batch_probe_pictures_n(pixels, bs, n, "divide", divisors, colour=colour, group_planes=3)      # a picture per group
        assert np.array_equal(one, got) and not bad_one.any()
        if count == 5:
            two, _ = gpu.batch_probe_pictures_n(pixels, bs, n, "divide", divisors, colour=colour, group_planes=6)        # 2 + 2 + 1
            assert np.array_equal(two, got)


def test_discard_and_none(gpu):
    pixels = _pixels(3, 40, 48, 3)
    for mode, params in (("discard", [0, 1, 2, 4]), ("none", [0])):
        want, refused = _yardstick(gpu, pixels, 1, 4, mode, params, 0, 3)
        got, bad = gpu.batch_probe_pictures_n(pixels, 1, 4, mode, params)
        assert not refused.any() and not bad.any() and np.array_equal(got, want)


def test_a_stack_of_bands(gpu):
    """nbands = 1 with colour 0: the planes are the bands."""
    pixels = _pixels(4, 37, 45, 1)
    for bs, n, divisors in ((1, 4, [1, 40]), (2, 9, [3, 64, 500])):
        want, refused = _yardstick(gpu, pixels, bs, n, "divide", divisors, 0, 1)
        assert not refused.any()
        for gp in (1, 3, None):
            got, bad = gpu.batch_probe_pictures_n(pixels, bs, n, "divide", divisors, group_planes=gp)
            assert got.shape == (4, 1, len(divisors)) and not bad.any() and np.array_equal(got, want)


def test_bad_amplitude_flags_the_candidate_that_the_batch_refuses(gpu):
    """dct_size 16, divisor 1: a bright flat picture's DC is 256 * 112 > 16383.  The batch refuses that candidate as a whole; the
    probe flags exactly the bright picture's bands under it and keeps the other candidate's totals right."""
    pixels = _pixels(3, 40, 48, 3)
    pixels[1] = 240
    want, refused = _yardstick(gpu, pixels, 1, 16, "divide", [1, 40], 0, 3)
    assert refused.tolist() == [True, False]
    got, bad = gpu.batch_probe_pictures_n(pixels, 1, 16, "divide", [1, 40])
    assert bad[1, :, 0].all() and not bad[:, :, 1].any()
    assert np.array_equal(got[:, :, 1], want[:, :, 1])
    # the flagged picture taken out, candidate 1 is sized like the rest
    rest = pixels[[0, 2]]
    want_rest, refused_rest = _yardstick(gpu, rest, 1, 16, "divide", [1], 0, 3)
    if not refused_rest.any():
        assert not bad[[0, 2], :, 0].any() and np.array_equal(got[[0, 2], :, :1], want_rest)


def test_explicit_device_form_on_device_0(gpu):
    pixels = _pixels(2, 40, 48, 3)
    k, rows, cols, nb = pixels.shape
    divisors = [3.0, 40.0]
    want, _ = gpu.batch_probe_pictures_n(pixels, 2, 3, "divide", divisors)
    din = gpu.DeviceBuffer(pixels.nbytes)
    dws = gpu.DeviceBuffer(gpu.batch_probe_pictures_workspace_bytes_n(k, nb, rows, cols, 2, 3, 3))
    dtot = gpu.DeviceBuffer(k * nb * 2 * 8)
    try:
        din.upload(pixels)
        gpu.batch_probe_pictures_n_device(din.ptr, k, nb, rows, cols, 2, 3, "divide", divisors, 3, dws.ptr, dtot.ptr, device=0)
        gpu.check(gpu.lib().jpegx_stream_synchronize(None))
        assert np.array_equal(dtot.download((k, nb, 2), np.uint64), want)
        assert np.array_equal(din.download(pixels.shape, np.uint8), pixels)          # the pixels are never written
    finally:
        for b in (din, dws, dtot):
            b.free()
