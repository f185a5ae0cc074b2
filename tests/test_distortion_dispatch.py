"""pipeline.probe_picture_distortion's dispatch, probe_picture_psnr's arithmetic, and the literal loop.  The device road is a stub
(jpegx.batch_probe_distortion_pictures_n replaced, the device declared usable), the loop a second stub where only the choice of
road is asked; the loop itself is held against a loop written here on pictures of 24 x 32, whose planes stay below
DCTN_MIN_SAMPLES, so everything holds with and without a GPU."""
import numpy as np
import pytest
from PIL import Image

import pipeline
import util
from pipeline.base import AlgorithmStep, step_classes


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
    out = np.empty((len(images), 3, len(divisors)), np.int64)
    for i, im in enumerate(images):
        x = im if colour is None else im.convert("YCbCr")
        ref = np.asarray(x).astype(np.int64)
        for j, d in enumerate(divisors):
            codec = pipeline.Jpeg(_config(config.height, config.width, config.block_size, config.dct_size, d))
            try:
                back = np.asarray(pipeline.Jpeg.decompress(codec.compress(x))).astype(np.int64)
                out[i, :, j] = [((back[:, :, b] - ref[:, :, b]) ** 2).sum() for b in range(3)]
            except util.BadRleCodeError:
                out[i, :, j] = -1
    return out


class Roads:
    """Both roads stubbed: the device road answers sse[p][b][q] = 1000 p + 100 b + divisor, flagged where ``flag`` says so; the loop
    answers -7 everywhere."""

    def __init__(self, monkeypatch, gate=2, flag=None, refuse=False):
        import jpegx
        self.calls, self.loops, self.flag = [], 0, flag
        monkeypatch.setattr(pipeline, "_device_usable", lambda: True)
        monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", gate)
        monkeypatch.setattr(pipeline, "_distortion_loop", self._loop)

        def device(pixels, bs, n, mode, params, **kw):
            self.calls.append((pixels.shape, bs, n, mode, list(params), kw))
            if refuse:
                raise jpegx.JpegxError("refused")
            k = pixels.shape[0]
            sse = (1000 * np.arange(k)[:, None, None] + 100 * np.arange(3)[None, :, None] + np.asarray(params)[None, None, :]).astype(np.uint64)
            bad = np.zeros(sse.shape, bool)
            if flag is not None:
                bad[flag[0], flag[1], [params.index(float(d)) for d in flag[2] if float(d) in params]] = True
            return sse, bad
        monkeypatch.setattr(jpegx, "batch_probe_distortion_pictures_n", device)

    def _loop(self, images, config, divisors, colour):
        self.loops += 1
        return np.full((len(images), 3, len(divisors)), -7, np.int64)


BIG = (64, 64)


def test_the_gate(monkeypatch):
    images = _pictures(2, *BIG, "YCbCr")
    config = _config(*BIG, 1, 4)
    for gate, count, device in ((3, 2, False), (3, 3, True), (3, 5, True), (1, 1, True), (0, 1, True), (None, 32, False)):
        r = Roads(monkeypatch, gate=gate)
        got = pipeline.probe_picture_distortion(images, config, list(range(1, count + 1)))
        assert (len(r.calls), r.loops) == ((1, 0) if device else (0, 1)), (gate, count)
        assert got.shape == (2, 3, count) and got.dtype == np.int64
        if device:
            assert r.calls[0][:4] == ((2, 64, 64, 3), 1, 4, "divide") and r.calls[0][4] == [float(d) for d in range(1, count + 1)]
            assert got[1, 2].tolist() == [1200 + d for d in range(1, count + 1)]


def test_the_gate_constant_is_a_count_or_none():
    gate = pipeline.DCTN_DISTORTION_MIN_CANDIDATES
    assert gate is None or (isinstance(gate, int) and gate >= 1)


def test_what_keeps_the_loop(monkeypatch):
    images = _pictures(2, *BIG, "YCbCr")
    # dct_size 8, another transform, a plane below DCTN_MIN_SAMPLES, pictures of another size than the configuration's
    small = _pictures(2, 24, 32, "YCbCr")
    for imgs, config in ((images, _config(*BIG, 1, 8)), (small, _config(24, 32, 1, 4)), (images, _config(64, 60, 1, 4))):
        r = Roads(monkeypatch)
        pipeline.probe_picture_distortion(imgs, config, [2, 3, 4])
        assert (len(r.calls), r.loops) == (0, 1), (config.dct_size, config.block_size)
    # planes of 32 x 32 samples are at the limit: taken at DCTN_MIN_SAMPLES 1024, not at 1025
    assert pipeline._blocked_shape(*BIG, 3, 16) == (32, 32) and pipeline.DCTN_MIN_SAMPLES == 1024
    r = Roads(monkeypatch)
    pipeline.probe_picture_distortion(images, _config(*BIG, 3, 16), [2, 3, 4])
    assert (len(r.calls), r.loops) == (1, 0)
    r = Roads(monkeypatch)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1025)
    pipeline.probe_picture_distortion(images, _config(*BIG, 3, 16), [2, 3, 4])
    assert (len(r.calls), r.loops) == (0, 1)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1024)
    # RGB pictures without colour='rgb' are taken as they are; with it, pictures of another mode keep the loop
    r = Roads(monkeypatch)
    pipeline.probe_picture_distortion(images, _config(*BIG, 1, 4), [2, 3, 4], colour="rgb")
    assert (len(r.calls), r.loops) == (0, 1)
    r = Roads(monkeypatch)
    pipeline.probe_picture_distortion(_pictures(2, *BIG, "RGB"), _config(*BIG, 1, 4), [2, 3, 4], colour="rgb")
    assert (len(r.calls), r.loops) == (1, 0) and r.calls[0][5] == {"colour": "rgb"}
    # a refusal of the library
    r = Roads(monkeypatch, refuse=True)
    got = pipeline.probe_picture_distortion(images, _config(*BIG, 1, 4), [2, 3, 4])
    assert (len(r.calls), r.loops) == (1, 1) and (got == -7).all()
    # no device
    r = Roads(monkeypatch)
    monkeypatch.setattr(pipeline, "_device_usable", lambda: False)
    pipeline.probe_picture_distortion(images, _config(*BIG, 1, 4), [2, 3, 4])
    assert (len(r.calls), r.loops) == (0, 1)


def test_a_non_stock_registry_keeps_the_loop(monkeypatch):
    stock = list(step_classes)
    try:
        class PassThrough(AlgorithmStep):
            step_index = 9.5

            def execute(self, array):
                return array

            def invert(self, array):
                return array
        assert not pipeline._stock_registry()
        r = Roads(monkeypatch)
        pipeline.probe_picture_distortion(_pictures(1, *BIG, "YCbCr"), _config(*BIG, 1, 4), [2, 3, 4])
        assert (len(r.calls), r.loops) == (0, 1)
    finally:
        step_classes[:] = stock
    assert pipeline._stock_registry()


def test_slices_of_thirty_two_and_minus_one_from_the_flag(monkeypatch):
    images = _pictures(3, *BIG, "YCbCr")
    divisors = [3 * k + 1 for k in range(70)]
    r = Roads(monkeypatch, flag=(1, 2, [4, 100]))                          # band 2 of picture 1 under divisors 4 and 100
    got = pipeline.probe_picture_distortion(images, _config(*BIG, 1, 4), divisors)
    assert [len(c[4]) for c in r.calls] == [32, 32, 6] and sum((c[4] for c in r.calls), []) == [float(d) for d in divisors]
    want = 1000 * np.arange(3)[:, None, None] + 100 * np.arange(3)[None, :, None] + np.asarray(divisors)[None, None, :]
    want[1, :, [divisors.index(4), divisors.index(100)]] = -1              # the whole picture: Jpeg.compress raises for it
    assert np.array_equal(got, want)
    psnr = pipeline.probe_picture_psnr(images, _config(*BIG, 1, 4), divisors)
    assert np.isnan(psnr[1, [1, 33]]).all() and np.isnan(psnr).sum() == 2


def test_an_array_of_pictures_goes_up_as_it_is(monkeypatch):
    stack = np.stack([np.asarray(im) for im in _pictures(2, *BIG, "YCbCr")])
    r = Roads(monkeypatch)
    pipeline.probe_picture_distortion(stack, _config(*BIG, 1, 4), [2, 3])
    assert len(r.calls) == 1 and r.calls[0][0] == (2, 64, 64, 3)


def test_value_errors_and_empty_inputs(monkeypatch):
    images = _pictures(1, 24, 32, "YCbCr")
    for name, kw in (("none", {}), ("discard", {"keep": 2})):
        config = pipeline.Configuration(width=32, height=24, block_size=1, dct_size=4, quantization=pipeline.QuantizationMethod(name, **kw))
        with pytest.raises(ValueError, match="must be 'divide'"):
            pipeline.probe_picture_distortion(images, config, [2])
    config = _config(24, 32, 1, 4)
    for bad in (2.5, 0, -3, float("nan"), float("inf"), "7", True, None):
        with pytest.raises(ValueError, match="whole positive number"):
            pipeline.probe_picture_distortion(images, config, [4, bad])
    with pytest.raises(ValueError, match="colour"):
        pipeline.probe_picture_psnr(images, config, [4], colour="bgr")
    assert pipeline.probe_picture_distortion([], config, [2, 3]).shape == (0, 3, 2)
    assert pipeline.probe_picture_distortion(images, config, []).shape == (1, 3, 0)
    assert pipeline.probe_picture_psnr(images, config, []).shape == (1, 0)


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, n", [(1, 4), (2, 3)])
def test_the_loop_is_the_literal_loop(bs, n, colour):
    images = _pictures(2, 24, 32, "YCbCr" if colour is None else "RGB")
    config = _config(24, 32, bs, n)
    divisors = [1, 8, 40, 1000]
    got = pipeline.probe_picture_distortion(images, config, divisors, colour=colour)
    want = _loop(images, config, divisors, colour)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert (want >= 0).all() and (want[:, :, 3] > want[:, :, 1]).all()     # content on which the divisor matters
    psnr = pipeline.probe_picture_psnr(images, config, divisors, colour=colour)
    with np.errstate(divide="ignore"):
        assert np.allclose(psnr, 10 * np.log10(255.0 ** 2 * 3 * 24 * 32 / want.sum(axis=1)), rtol=1e-12, atol=0)


def test_bad_rle_is_minus_one_in_every_band():
    """The checkerboard of tests/test_probe_dispatch.py: dct_size 30 under divisor 1 cannot be coded."""
    yy, xx = np.mgrid[0:60, 0:60]
    px = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    px[:, :, 1:] = 128                                                     # only the first band is the checkerboard
    board = Image.fromarray(px, mode="YCbCr")
    got = pipeline.probe_picture_distortion([board], _config(60, 60, 1, 30), [1, 64])
    assert got[0, :, 0].tolist() == [-1, -1, -1] and (got[0, :, 1] >= 0).all()
    psnr = pipeline.probe_picture_psnr([board], _config(60, 60, 1, 30), [1, 64])
    assert np.isnan(psnr[0, 0]) and np.isfinite(psnr[0, 1])


def test_psnr_on_a_hand_made_table(monkeypatch):
    sse = np.array([[[0, 100, 3, -1], [0, 200, 0, -1], [0, 300, 0, -1]],
                    [[1, 0, 10 ** 12, 5], [1, 0, 10 ** 12, -1], [1, 0, 10 ** 12, 5]]], np.int64)
    monkeypatch.setattr(pipeline, "probe_picture_distortion", lambda images, config, divisors, colour=None: sse)
    got = pipeline.probe_picture_psnr([None, None], _config(10, 20, 1, 4), [1, 2, 3, 4])
    peak = 255.0 ** 2 * 3 * 10 * 20
    assert got.shape == (2, 4) and got.dtype == np.float64
    assert got[0, 0] == np.inf and got[1, 1] == np.inf and np.isnan(got[0, 3]) and np.isnan(got[1, 3])
    assert got[0, 1] == pytest.approx(10 * np.log10(peak / 600.0), rel=1e-14)
    assert got[0, 2] == pytest.approx(10 * np.log10(peak / 3.0), rel=1e-14)
    assert got[1, 0] == pytest.approx(10 * np.log10(peak / 3.0), rel=1e-14)
    assert got[1, 2] == pytest.approx(10 * np.log10(peak / 3e12), rel=1e-14) and got[1, 2] < 0
