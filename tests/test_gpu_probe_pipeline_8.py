"""pipeline's probes at dct_size 8 on the device road (DCT8_PROBE_MIN_CANDIDATES and DCT8_DISTORTION_MIN_CANDIDATES set by
monkeypatch; they ship as None) against the loop they replace: probe_picture_sizes, probe_picture_distortion and
probe_picture_psnr entry for entry, compress_to_size and compress_to_quality container for container.  Pictures of 64 x 64
and of 37 x 53 at block_size 4 and 1, with colour 'rgb' and without.  Every comparison is exact."""
import numpy as np
import pytest
from PIL import Image

import pipeline

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 4), (64, 64, 1), (37, 53, 4), (37, 53, 1)]
DIVISORS = [1, 2, 3, 7, 40, 1000]


def _config(rows, cols, bs, divisor=40):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=8, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def _pictures(count, rows, cols, mode, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for p in range(count):
        yy, xx = np.mgrid[0:rows, 0:cols]
        smooth = (yy * (3 + p) + xx * 2) % 256
        noise = rng.integers(0, 256, (rows, cols, 3))
        px = np.where((xx < cols // 2)[..., None], smooth[..., None] + np.arange(3) * 20, noise) % 256
        out.append(Image.fromarray(px.astype(np.uint8), mode=mode))
    return out


class Counted:
    """The gates set, and the device entries counted on their way through."""

    def __init__(self, monkeypatch):
        import jpegx
        self.sizes = self.sse = 0
        monkeypatch.setattr(pipeline, "DCT8_PROBE_MIN_CANDIDATES", 1)
        monkeypatch.setattr(pipeline, "DCT8_DISTORTION_MIN_CANDIDATES", 1)
        real_sizes, real_sse = jpegx.batch_probe_pictures, jpegx.batch_probe_distortion_pictures

        def sizes(*a, **kw):
            self.sizes += 1
            return real_sizes(*a, **kw)

        def sse(*a, **kw):
            self.sse += 1
            return real_sse(*a, **kw)
        monkeypatch.setattr(jpegx, "batch_probe_pictures", sizes)
        monkeypatch.setattr(jpegx, "batch_probe_distortion_pictures", sse)


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("rows, cols, bs", SHAPES)
def test_the_probes_equal_the_loop(monkeypatch, gpu, rows, cols, bs, colour):
    images = _pictures(3, rows, cols, "YCbCr" if colour is None else "RGB")
    config = _config(rows, cols, bs)
    assert pipeline.DCT8_PROBE_MIN_CANDIDATES is None and pipeline.DCT8_DISTORTION_MIN_CANDIDATES is None
    want_sizes = pipeline.probe_picture_sizes(images, config, DIVISORS, colour=colour)          # the gates are None: the loop
    want_sse = pipeline.probe_picture_distortion(images, config, DIVISORS, colour=colour)
    want_psnr = pipeline.probe_picture_psnr(images, config, DIVISORS, colour=colour)
    c = Counted(monkeypatch)
    assert np.array_equal(pipeline.probe_picture_sizes(images, config, DIVISORS, colour=colour), want_sizes)
    assert np.array_equal(pipeline.probe_picture_distortion(images, config, DIVISORS, colour=colour), want_sse)
    assert np.array_equal(pipeline.probe_picture_psnr(images, config, DIVISORS, colour=colour), want_psnr)
    assert (c.sizes, c.sse) == (1, 2)
    assert (want_sizes > 0).all() and (np.diff(want_sizes, axis=1) < 0).all() and (want_sse >= 0).all()


@pytest.mark.parametrize("rows, cols, bs", SHAPES)
def test_to_size_and_to_quality_return_the_loops_container(monkeypatch, gpu, rows, cols, bs):
    image = _pictures(1, rows, cols, "YCbCr")[0]
    config = _config(rows, cols, bs)
    sizes = pipeline.probe_picture_sizes([image], config, [2, 40])[0]
    budget = int(sizes.sum() // 2)                                       # between the sizes under 2 and under 40
    want = pipeline.compress_to_size(image, config, budget)
    psnr = pipeline.probe_picture_psnr([image], config, [2, 40])[0]
    floor = float(psnr[1] + 0.25 * (psnr[0] - psnr[1])) if np.isfinite(psnr).all() and psnr[0] > psnr[1] else float(psnr.min())
    want_q = pipeline.compress_to_quality(image, config, floor)
    c = Counted(monkeypatch)
    got = pipeline.compress_to_size(image, config, budget)
    assert got == want and len(got[0]) <= budget and 2 <= got[1] <= 40 and c.sizes >= 1
    got_q = pipeline.compress_to_quality(image, config, floor)
    assert got_q[0] == want_q[0] and got_q[1] == want_q[1] and got_q[2] == want_q[2] and c.sse >= 1


def test_sets_of_pictures_to_a_budget_and_to_a_floor(monkeypatch, gpu):
    images = _pictures(3, 37, 53, "RGB")
    config = _config(37, 53, 2)
    ladder = [1, 4, 16, 64, 256]
    table = pipeline.probe_picture_sizes(images, config, ladder, colour="rgb")
    budget = int(table[:, 2].max())
    want = pipeline.compress_pictures_to_size(images, config, budget, ladder, colour="rgb")
    psnr = pipeline.probe_picture_psnr(images, config, ladder, colour="rgb")
    floor = float(psnr[:, 2].min())
    want_q = pipeline.compress_pictures_to_quality(images, config, floor, ladder, colour="rgb")
    c = Counted(monkeypatch)
    assert pipeline.compress_pictures_to_size(images, config, budget, ladder, colour="rgb") == want
    assert pipeline.compress_pictures_to_quality(images, config, floor, ladder, colour="rgb") == want_q
    assert (c.sizes, c.sse) == (1, 1)
