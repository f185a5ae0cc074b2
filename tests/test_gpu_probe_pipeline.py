"""pipeline.probe_picture_sizes, compress_to_size and compress_pictures_to_size on the device road: the sizes are those of the
literal loop over Jpeg.compress / compress_rgb, the road is taken exactly where the documentation says, and the byte-budget
functions return what the same search gives when it is driven by the loop."""
import numpy as np
import pytest
from PIL import Image

import pipeline
import util

pytestmark = pytest.mark.gpu


def _config(rows, cols, bs, n, divisor=40):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def _picture(kind, rows, cols, mode):
    rng = np.random.default_rng(kind)
    yy, xx = np.mgrid[0:rows, 0:cols]
    if kind % 4 == 0:
        px = np.full((rows, cols, 3), 60 + kind)
    elif kind % 4 == 1:
        px = np.repeat(((yy * 5 + xx * 3 + kind) % 256)[..., None], 3, axis=2)
    elif kind % 4 == 2:
        px = rng.integers(0, 256, (rows, cols, 3))
    else:
        px = np.where((xx < cols // 2)[..., None], rng.integers(0, 256, (rows, cols, 3)), 128 + kind)
    return Image.fromarray((px % 256).astype(np.uint8), mode=mode)


def _loop(images, config, divisors, colour):
    out = np.empty((len(images), len(divisors)), np.int64)
    for j, d in enumerate(divisors):
        codec = pipeline.Jpeg(_config(config.height, config.width, config.block_size, config.dct_size, d))
        for i, im in enumerate(images):
            try:
                out[i, j] = len(codec.compress(im) if colour is None else codec.compress_rgb(im))
            except util.BadRleCodeError:
                out[i, j] = -1
    return out


@pytest.fixture
def probe_calls(gpu, monkeypatch):
    """Counts the calls of jpegx.batch_probe_pictures_n that the pipeline makes."""
    calls = []
    real = gpu.batch_probe_pictures_n

    def counted(*args, **kwargs):
        calls.append((args[0].shape, list(args[4])))
        return real(*args, **kwargs)

    monkeypatch.setattr(gpu, "batch_probe_pictures_n", counted)
    return calls


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("rows, cols, bs, n, divisors", [(64, 64, 1, 4, [1, 8, 40, 1000]), (60, 52, 1, 4, [1, 7, 300]),
                                                         (64, 64, 1, 16, [1, 8, 40, 1000]), (60, 52, 1, 3, [2, 9])])
def test_device_road_equals_the_loop(probe_calls, rows, cols, bs, n, divisors, colour):
    images = [_picture(k, rows, cols, "YCbCr" if colour is None else "RGB") for k in range(3)]
    config = _config(rows, cols, bs, n)
    h, w = pipeline._blocked_shape(rows, cols, bs, n)
    assert h * w >= pipeline.DCTN_MIN_SAMPLES
    got = pipeline.probe_picture_sizes(images, config, divisors, colour=colour)
    assert probe_calls == [((3, rows, cols, 3), [float(d) for d in divisors])]
    assert np.array_equal(got, _loop(images, config, divisors, colour))


def test_bad_rle_on_the_device_road(probe_calls):
    """dct_size 16, divisor 1: the bright flat picture's DC passes 16383 -- the loop raises BadRleCodeError, the probe says -1."""
    images = [_picture(2, 64, 64, "YCbCr"), Image.fromarray(np.full((64, 64, 3), 250, np.uint8), mode="YCbCr")]
    config = _config(64, 64, 1, 16)
    got = pipeline.probe_picture_sizes(images, config, [1, 64])
    want = _loop(images, config, [1, 64], None)
    assert len(probe_calls) == 1 and want[1, 0] == -1 and want[1, 1] > 0
    assert np.array_equal(got, want)


def test_the_road_is_not_taken_where_the_documentation_says(probe_calls, monkeypatch):
    config = _config(24, 24, 1, 4)
    small = [_picture(3, 24, 24, "YCbCr")]
    assert np.array_equal(pipeline.probe_picture_sizes(small, config, [2, 40]), _loop(small, config, [2, 40], None))
    assert probe_calls == []                            # 576 samples: below DCTN_MIN_SAMPLES
    images = [_picture(3, 64, 64, "YCbCr")]
    config = _config(64, 64, 1, 4)
    assert np.array_equal(pipeline.probe_picture_sizes(images, config, [40]), _loop(images, config, [40], None))
    assert probe_calls == []                            # one divisor: below DCTN_PROBE_MIN_CANDIDATES
    eight = _config(64, 64, 1, 8)
    assert np.array_equal(pipeline.probe_picture_sizes(images, eight, [2, 40]), _loop(images, eight, [2, 40], None))
    assert probe_calls == []                            # dct_size 8 has kernels of its own
    monkeypatch.setattr(pipeline, "DCTN_PROBE_MIN_CANDIDATES", None)
    pipeline.probe_picture_sizes(images, config, [2, 40])
    assert probe_calls == []                            # the road is off
    monkeypatch.setattr(pipeline, "DCTN_PROBE_MIN_CANDIDATES", 1)
    pipeline.probe_picture_sizes(images, config, [40])
    assert len(probe_calls) == 1
    many = list(range(1, 41))
    got = pipeline.probe_picture_sizes(images, config, many)
    assert [len(c[1]) for c in probe_calls[1:]] == [32, 8]      # slices of 32
    assert np.array_equal(got[:, [0, 39]], _loop(images, config, [1, 40], None))


@pytest.mark.parametrize("colour", [None, "rgb"])
def test_compress_to_size_equals_the_search_over_the_loop(probe_calls, monkeypatch, colour):
    image = _picture(3, 64, 64, "YCbCr" if colour is None else "RGB")
    config = _config(64, 64, 1, 4)
    kw = dict(colour=colour, lo=1, hi=512, probes=6, rounds=2)
    got = pipeline.compress_to_size(image, config, 6000, **kw)
    assert 1 <= len(probe_calls) <= 3 and len(got[0]) <= 6000
    probe_calls.clear()
    monkeypatch.setattr(pipeline, "DCTN_PROBE_MIN_CANDIDATES", None)        # the same search, driven by the loop
    want = pipeline.compress_to_size(image, config, 6000, **kw)
    assert probe_calls == [] and got == want
    assert pipeline.Jpeg.decompress(got[0]).size == (64, 64)


def test_compress_pictures_to_size_picks_rungs_per_picture(probe_calls):
    images = [_picture(k, 64, 64, "YCbCr") for k in (2, 0, 3, 1, 6, 5)]
    config = _config(64, 64, 1, 4)
    ladder = [2, 10, 50, 400]
    sizes = _loop(images, config, ladder, None)
    max_bytes = int(sizes[0][2])                           # the first noise picture fits from the third rung on
    containers, chosen = pipeline.compress_pictures_to_size(images, config, max_bytes, ladder)
    assert len(probe_calls) == 1
    assert chosen == [next(d for d, s in zip(ladder, row) if s <= max_bytes) for row in sizes]
    assert len(set(chosen)) >= 2 and chosen[0] == 50
    for im, d, c in zip(images, chosen, containers):
        assert c == pipeline.Jpeg(_config(64, 64, 1, 4, d)).compress(im) and len(c) <= max_bytes
