"""pipeline.probe_picture_set_distortion, probe_picture_set_psnr and compress_picture_set_to_quality on the device road against
the literal loop over Jpeg.compress and Jpeg.decompress under a configuration of each picture's own size (the same functions
with DCTN_DISTORTION_SET_MIN_PICTURES = None).  Exact: every admitted plane holds at least DCTN_MIN_SAMPLES samples, so every
road of the loop ends in k_forward_n's integers and k_inverse_n's clamped bytes, whose arithmetic the probe
repeats.  Pictures of 64 x 64, 67 x 93, 128 x 96 and 40 x 200 with a grey picture and a 20 x 20 picture among them, which go
through the loop in place."""
import numpy as np
import pytest
from PIL import Image

import pipeline

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (67, 93), (128, 96), (40, 200)]
CONFIGS = [(1, 4), (1, 16), (2, 12)]
FEW = [5, 40, 1000]
MANY = [4 + 3 * k for k in range(33)]                # 255 * 16^2 / 4 still codes in 15 bits


def _config(bs, n, divisor=40, rows=1, cols=1):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def _picture(p, rows, cols, mode, seed=11):
    rng = np.random.default_rng([seed, rows, cols])
    yy, xx = np.mgrid[0:rows, 0:cols]
    smooth = ((yy * (2 + p) + xx * 3) % 256)[..., None] + np.arange(3) * 30
    px = np.where((xx < cols // 2)[..., None], smooth, rng.integers(0, 256, (rows, cols, 3))) % 256
    return Image.fromarray(px.astype(np.uint8), mode=mode)


def _mixed(mode):
    ims = [_picture(p, r, c, mode) for p, (r, c) in enumerate(SHAPES)]
    ims.insert(1, Image.fromarray(np.asarray(_picture(7, 50, 50, mode))[..., 0], mode="L"))      # a grey picture
    ims.insert(3, _picture(8, 20, 20, mode))                                                      # below DCTN_MIN_SAMPLES at dct_size 4 and 12
    ims.append(_picture(9, 10, 10, mode))                                                         # and at every dct_size here
    return ims


def _admitted(images, bs, n):
    """How many of the pictures the set road admits: three bands and planes of at least DCTN_MIN_SAMPLES samples."""
    return sum(1 for im in images if im.mode != "L" and np.prod(pipeline._blocked_shape(im.height, im.width, bs, n)) >= pipeline.DCTN_MIN_SAMPLES)


class Recorder:
    """Counts the calls of the device road and the pictures they take, without changing it."""

    def __init__(self, monkeypatch):
        import jpegx
        self.calls = []
        inner = jpegx.batch_probe_distortion_picture_set_n

        def counted(pictures, *args, **kw):
            self.calls.append(len(pictures))
            return inner(pictures, *args, **kw)
        monkeypatch.setattr(jpegx, "batch_probe_distortion_picture_set_n", counted)


def _by_loop(monkeypatch, fn, *args, **kw):
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_DISTORTION_SET_MIN_PICTURES", None)
        return fn(*args, **kw)


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, n", CONFIGS)
def test_three_and_thirty_three_divisors_equal_the_loop(gpu, monkeypatch, bs, n, colour):
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", 1)     # the road itself is asked, whatever the gates say
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_SET_MIN_PICTURES", 1)
    images = _mixed("YCbCr" if colour is None else "RGB")
    if colour is None:
        images = [im for im in images if im.mode != "L"]
    config = _config(bs, n)
    admitted = _admitted(images, bs, n)
    assert len(SHAPES) <= admitted < len(images)          # some pictures go through the loop in place
    for divisors, calls in ((FEW, 1), (MANY, 2)):
        r = Recorder(monkeypatch)
        got = pipeline.probe_picture_set_distortion(images, config, divisors, colour=colour)
        assert r.calls == [admitted] * calls
        want = _by_loop(monkeypatch, pipeline.probe_picture_set_distortion, images, config, divisors, colour=colour)
        assert r.calls == [admitted] * calls
        assert got.dtype == np.int64 and got.shape == (len(images), 3, len(divisors))
        assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
        assert (want >= 0).all()
    psnr = pipeline.probe_picture_set_psnr(images, config, FEW, colour=colour)
    assert np.array_equal(psnr, _by_loop(monkeypatch, pipeline.probe_picture_set_psnr, images, config, FEW, colour=colour))
    for at, im in enumerate(images):
        one = pipeline.probe_picture_psnr([im], _config(bs, n, rows=im.height, cols=im.width), FEW, colour=colour)
        assert np.array_equal(psnr[at], one[0]), at


def test_a_picture_that_cannot_be_coded_is_minus_one(gpu, monkeypatch):
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", 1)
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_SET_MIN_PICTURES", 1)
    images = [_picture(0, 64, 64, "YCbCr"), _picture(1, 67, 93, "YCbCr")]
    images[0] = Image.fromarray(np.asarray(images[0]) // 2, mode="YCbCr")      # no pixel above 127: codes under divisor 2
    white = np.asarray(images[1]).copy()
    white[:16, :16, 1] = 255                               # one block of band 1: DC 65280 under divisor 2 and 3
    images[1] = Image.fromarray(white, mode="YCbCr")
    r = Recorder(monkeypatch)
    got = pipeline.probe_picture_set_distortion(images, _config(1, 16), [2, 3, 64])
    want = _by_loop(monkeypatch, pipeline.probe_picture_set_distortion, images, _config(1, 16), [2, 3, 64])
    assert r.calls == [2] and np.array_equal(got, want)
    assert (got[1, :, :2] == -1).all() and (got[1, :, 2] >= 0).all() and (got[0] >= 0).all()


@pytest.mark.parametrize("colour, bs, n", [(None, 1, 4), ("rgb", 1, 16), ("rgb", 2, 12)])
def test_compress_picture_set_to_quality_equals_choosing_by_the_loop(gpu, monkeypatch, colour, bs, n):
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", 1)
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_SET_MIN_PICTURES", 1)
    mode = "YCbCr" if colour is None else "RGB"
    images = [_picture(p, r, c, mode) for p, (r, c) in enumerate(SHAPES)]
    images.insert(2, Image.fromarray(np.full((70, 90, 3), 90, np.uint8), mode=mode))      # a flat picture keeps its quality up the ladder
    images.insert(4, _picture(8, 10, 10, mode))
    ladder = [4, 8, 16, 32, 64, 128, 256]
    floor = 30.0 if bs == 1 else 13.0                      # half of every picture is noise, which pooling 2 x 2 loses
    r = Recorder(monkeypatch)
    containers, chosen = pipeline.compress_picture_set_to_quality(images, _config(bs, n), floor, ladder, colour=colour)
    assert r.calls == [5]                                  # ONE probe of the admitted pictures
    assert (containers, chosen) == _by_loop(monkeypatch, pipeline.compress_picture_set_to_quality, images, _config(bs, n), floor, ladder, colour=colour)
    # choosing per picture by the loop, compressing with Jpeg(config_i)
    loop = _by_loop(monkeypatch, pipeline.probe_picture_set_psnr, images, _config(bs, n), ladder, colour=colour)
    for at, (im, box, d) in enumerate(zip(images, containers, chosen)):
        meeting = [j for j, p in enumerate(loop[at]) if not np.isnan(p) and p >= floor]
        assert d == ladder[meeting[-1]], (at, d, loop[at].tolist())
        codec = pipeline.Jpeg(_config(bs, n, d, im.height, im.width))
        assert box == (codec.compress(im) if colour is None else codec.compress_rgb(im)), at
    print(bs, n, colour, chosen)
    if bs == 1:                                            # pooling 2 x 2 loses the noise on every rung alike
        assert chosen[2] > min(chosen), chosen             # the noisy pictures need a finer rung than the flat one
    with pytest.raises(pipeline.TargetQualityError, match="picture 0 meets 90.00 dB on no rung"):
        pipeline.compress_picture_set_to_quality(images, _config(bs, n), 90.0, ladder, colour=colour)
