"""pipeline.probe_picture_sizes away from the device road: the sizes are those of the literal loop over Jpeg.compress /
compress_rgb, header and length prefixes included; BadRleCodeError becomes -1; bad arguments are ValueError; more than 32
divisors come back in order.  The pictures are 24 x 32 (planes below DCTN_MIN_SAMPLES; the checkerboard's road ends in -1 on the
device as on the host), so this holds with and without a GPU."""
import numpy as np
import pytest
from PIL import Image

import pipeline
import util


def _config(rows, cols, bs, n, divisor=40):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def _pictures(count, rows, cols, mode, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for p in range(count):
        yy, xx = np.mgrid[0:rows, 0:cols]
        smooth = (yy * (3 + p) + xx * 2) % 256
        noise = rng.integers(0, 256, (rows, cols, 3))
        px = np.where((xx < cols // 2)[..., None], smooth[..., None] + np.arange(3) * 20, noise) % 256
        out.append(Image.fromarray(px.astype(np.uint8), mode=mode))
    return out


def _loop(images, config, divisors, colour):
    out = np.empty((len(images), len(divisors)), np.int64)
    for j, d in enumerate(divisors):
        cfg = _config(config.height, config.width, config.block_size, config.dct_size, d)
        codec = pipeline.Jpeg(cfg)
        for i, im in enumerate(images):
            try:
                out[i, j] = len(codec.compress(im) if colour is None else codec.compress_rgb(im))
            except util.BadRleCodeError:
                out[i, j] = -1
    return out


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, n", [(1, 4), (2, 3)])
def test_sizes_equal_the_loop(bs, n, colour):
    images = _pictures(2, 24, 32, "YCbCr" if colour is None else "RGB")
    config = _config(24, 32, bs, n)
    divisors = [1, 8, 40, 1000]
    got = pipeline.probe_picture_sizes(images, config, divisors, colour=colour)
    want = _loop(images, config, divisors, colour)
    assert got.dtype == np.int64 and got.shape == (2, 4)
    assert np.array_equal(got, want)
    assert (want > 0).all() and (np.diff(want, axis=1) < 0).all()          # content on which the divisor matters
    # the header is counted: its JSON grows with the divisor's digits
    heads = [len(pipeline.file_format.create_header(_config(24, 32, bs, n, d))) for d in divisors]
    assert heads[3] - heads[0] == 3


def test_an_array_of_pictures_is_taken_like_compress_pictures_takes_it():
    images = _pictures(2, 24, 32, "YCbCr")
    stack = np.stack([np.asarray(im) for im in images])
    config = _config(24, 32, 1, 4)
    assert np.array_equal(pipeline.probe_picture_sizes(stack, config, [3, 50]), _loop(images, config, [3, 50], None))


def test_bad_rle_is_minus_one():
    """A 0/255 checkerboard at dct_size 30 and divisor 1: the unnormalised 30 x 30 transform puts tens of thousands into the
    highest frequency, far beyond the 15 bits of a code, and the host coder raises BadRleCodeError.  (Not dct_size 32: the host
    quantiser hands blocks whose sides are multiples of 8 to the device, so that road cannot run on a machine without one.)"""
    yy, xx = np.mgrid[0:60, 0:60]
    board = Image.fromarray(np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2), mode="YCbCr")
    config = _config(60, 60, 1, 30)
    with pytest.raises(util.BadRleCodeError):
        pipeline.Jpeg(_config(60, 60, 1, 30, 1)).compress(board)
    want = len(pipeline.Jpeg(_config(60, 60, 1, 30, 64)).compress(board))
    got = pipeline.probe_picture_sizes([board], config, [1, 64])
    assert got.tolist() == [[-1, want]]


def test_value_errors():
    images = _pictures(1, 24, 32, "YCbCr")
    for name, kw in (("none", {}), ("discard", {"keep": 2})):
        config = pipeline.Configuration(width=32, height=24, block_size=1, dct_size=4, quantization=pipeline.QuantizationMethod(name, **kw))
        with pytest.raises(ValueError, match="must be 'divide'"):
            pipeline.probe_picture_sizes(images, config, [2])
    config = _config(24, 32, 1, 4)
    for bad in (2.5, 0, -3, float("nan"), float("inf"), "7", True, None):
        with pytest.raises(ValueError, match="whole positive number"):
            pipeline.probe_picture_sizes(images, config, [4, bad])
    with pytest.raises(ValueError, match="colour"):
        pipeline.probe_picture_sizes(images, config, [4], colour="bgr")


def test_thirty_three_divisors_come_back_in_order():
    images = _pictures(2, 24, 32, "YCbCr")
    config = _config(24, 32, 1, 4)
    divisors = [3 * k + 1 for k in range(33)]
    got = pipeline.probe_picture_sizes(images, config, divisors)
    assert got.shape == (2, 33)
    assert np.array_equal(got, _loop(images, config, divisors, None))
    assert np.array_equal(got[:, [0, 32]], pipeline.probe_picture_sizes(images, config, [1, 97]))


def test_empty_inputs():
    config = _config(24, 32, 1, 4)
    assert pipeline.probe_picture_sizes([], config, [2, 3]).shape == (0, 2)
    assert pipeline.probe_picture_sizes(_pictures(1, 24, 32, "YCbCr"), config, []).shape == (1, 0)
