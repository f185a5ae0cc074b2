"""pipeline.probe_picture_distortion, probe_picture_psnr, compress_to_quality and compress_pictures_to_quality on the device road
against the literal loop over Jpeg.compress and Jpeg.decompress (the same functions with DCTN_DISTORTION_MIN_CANDIDATES = None).
Exact: at these sizes every decoding road of the loop ends in k_inverse_n's clamped bytes, whose arithmetic the
probe repeats.  Pictures of 64 x 64, 67 x 93 and 128 x 96; block_size 1 at dct_size 4 and 16, block_size 2 at dct_size 12."""
import numpy as np
import pytest
from PIL import Image

import pipeline

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (67, 93), (128, 96)]
CONFIGS = [(1, 4), (1, 16), (2, 12)]
FEW = [5, 40, 1000]
MANY = [4 + 3 * k for k in range(33)]                # 255 * 16^2 / 4 still codes in 15 bits
FLOORS = {1: (30.0, 22.0), 2: (14.0, 12.0)}          # dB, by block_size: half of every picture is noise, which pooling 2 x 2 loses


def _config(rows, cols, bs, n, divisor=40):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def _pictures(count, rows, cols, mode, seed=11):
    rng = np.random.default_rng([seed, rows, cols])
    yy, xx = np.mgrid[0:rows, 0:cols]
    out = []
    for p in range(count):
        smooth = ((yy * (2 + p) + xx * 3) % 256)[..., None] + np.arange(3) * 30
        px = np.where((xx < cols // 2)[..., None], smooth, rng.integers(0, 256, (rows, cols, 3))) % 256
        out.append(Image.fromarray(px.astype(np.uint8), mode=mode))
    return out


class Recorder:
    """Counts the calls of the device road without changing it."""

    def __init__(self, monkeypatch):
        import jpegx
        self.calls = 0
        inner = jpegx.batch_probe_distortion_pictures_n

        def counted(*args, **kw):
            self.calls += 1
            return inner(*args, **kw)
        monkeypatch.setattr(jpegx, "batch_probe_distortion_pictures_n", counted)


def _by_loop(monkeypatch, fn, *args, **kw):
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", None)
        return fn(*args, **kw)


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, n", CONFIGS)
@pytest.mark.parametrize("rows, cols", SHAPES)
def test_three_and_thirty_three_divisors_equal_the_loop(gpu, monkeypatch, rows, cols, bs, n, colour):
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", 1)     # the road itself is asked, whatever the gate says
    images = _pictures(2, rows, cols, "YCbCr" if colour is None else "RGB")
    config = _config(rows, cols, bs, n)
    for divisors, calls in ((FEW, 1), (MANY, 2)):
        r = Recorder(monkeypatch)
        got = pipeline.probe_picture_distortion(images, config, divisors, colour=colour)
        assert r.calls == calls
        want = _by_loop(monkeypatch, pipeline.probe_picture_distortion, images, config, divisors, colour=colour)
        assert r.calls == calls
        assert got.dtype == np.int64 and got.shape == (2, 3, len(divisors)) and np.array_equal(got, want), (got - want).tolist()
        assert (want >= 0).all()
    psnr = pipeline.probe_picture_psnr(images, config, FEW, colour=colour)
    assert np.array_equal(psnr, _by_loop(monkeypatch, pipeline.probe_picture_psnr, images, config, FEW, colour=colour))
    assert (np.diff(psnr, axis=1) < 0).all()


def test_a_picture_that_cannot_be_coded_is_minus_one(gpu, monkeypatch):
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", 1)
    images = _pictures(2, 64, 64, "YCbCr")
    white = np.asarray(images[1]).copy()
    white[:16, :16, 1] = 255                               # one block of band 1: DC 65280 under divisor 1 and 3
    images[1] = Image.fromarray(white, mode="YCbCr")
    config = _config(64, 64, 1, 16)
    r = Recorder(monkeypatch)
    got = pipeline.probe_picture_distortion(images, config, [1, 3, 64])
    want = _by_loop(monkeypatch, pipeline.probe_picture_distortion, images, config, [1, 3, 64])
    assert r.calls == 1 and np.array_equal(got, want)
    assert (got[1, :, :2] == -1).all() and (got[1, :, 2] >= 0).all()


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("rows, cols, bs, n", [(64, 64, 1, 4), (67, 93, 2, 12), (128, 96, 1, 16)])
def test_compress_to_quality_returns_the_loop_driven_search(gpu, monkeypatch, rows, cols, bs, n, colour):
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", 1)
    image = _pictures(1, rows, cols, "YCbCr" if colour is None else "RGB")[0]
    config = _config(rows, cols, bs, n)
    for floor in FLOORS[bs]:
        r = Recorder(monkeypatch)
        container, divisor, psnr = pipeline.compress_to_quality(image, config, floor, colour=colour, hi=512, probes=8, rounds=2)
        assert 1 <= r.calls <= 3
        want = _by_loop(monkeypatch, pipeline.compress_to_quality, image, config, floor, colour=colour, hi=512, probes=8, rounds=2)
        assert (container, divisor, psnr) == want and psnr >= floor
        print("%d x %d bs %d N %d %s: %.1f dB floor -> divisor %d at %.2f dB, %d bytes" % (rows, cols, bs, n, colour, floor, divisor, psnr, len(container)))
        codec = pipeline.Jpeg(_config(rows, cols, bs, n, divisor))
        assert container == (codec.compress(image) if colour is None else codec.compress_rgb(image))
    with pytest.raises(pipeline.TargetQualityError):
        pipeline.compress_to_quality(image, config, 90.0, colour=colour, lo=8, hi=512, probes=8)


def test_compress_pictures_to_quality_equals_the_loop(gpu, monkeypatch):
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", 1)
    images = _pictures(4, 67, 93, "RGB")
    images[2] = Image.fromarray(np.full((67, 93, 3), 90, np.uint8), mode="RGB")      # a flat picture keeps its quality far up the ladder
    config = _config(67, 93, 1, 16)
    ladder = [4, 8, 16, 32, 64, 128, 256]
    containers, chosen = pipeline.compress_pictures_to_quality(images, config, 40.0, ladder, colour="rgb")
    assert (containers, chosen) == _by_loop(monkeypatch, pipeline.compress_pictures_to_quality, images, config, 40.0, ladder, colour="rgb")
    assert chosen[2] == 256 and min(chosen) < 256, chosen            # the noisy pictures need a finer rung than the flat one
    for im, c, d in zip(images, containers, chosen):
        assert c == pipeline.Jpeg(_config(67, 93, 1, 16, d)).compress_rgb(im)
