"""GPU: pipeline.compress_picture_set / decompress_picture_set_u8 / decompress_picture_set on the set road against the loop over
Jpeg.compress / compress_rgb / decompress / decompress_rgb with a Configuration of each picture's own size, byte for byte and
sample for sample.  The gates are set by the test; a recording wrapper around the jpegx conveniences proves that the road ran
and with how many pictures."""
import numpy as np
import pytest
from PIL import Image

from test_codec_oracle_n import config_of

pytestmark = pytest.mark.gpu

# 7 pictures of 5 different sizes; every plane holds at least DCTN_MIN_SAMPLES samples at block_size 1
SIZES = [(40, 56), (33, 70), (40, 57), (120, 32), (40, 56), (64, 17), (33, 70)]
# the README example pools 5 x 5: larger pictures, so that the pooled planes still hold 1024 samples
SIZES_BS5 = [(150, 210), (161, 333), (150, 211), (400, 160), (150, 210), (320, 85), (161, 333)]
CONFIGS = [(4, 1, "divide", 40.0, SIZES), (16, 1, "divide", 40.0, SIZES), (3, 1, "discard", 4.0, SIZES), (24, 5, "divide", 1000.0, SIZES_BS5)]


def images_of(seed, sizes, mode):
    rng = np.random.default_rng(seed)
    out = []
    for p, (r, c) in enumerate(sizes):
        px = rng.integers(0, 256, (r, c, 3), dtype=np.uint8)
        if p == 1:
            y, x = np.mgrid[0:r, 0:c]
            for k in range(3):
                px[:, :, k] = ((5 * y + 3 * x + 60 * k) // 2 % 256).astype(np.uint8)
        out.append(Image.fromarray(px, mode=mode))
    return out


@pytest.fixture
def road(gpu, monkeypatch):
    """The gates open from 2 admitted pictures on, no plane limit; the calls of the two conveniences are recorded with the
    number of pictures they were handed."""
    import pipeline
    monkeypatch.setattr(pipeline, "DCTN_PICTURE_SET_MIN_PICTURES", 2)
    monkeypatch.setattr(pipeline, "DCTN_PICTURE_SET_COMPRESS_MAX_SAMPLES", None)
    monkeypatch.setattr(pipeline, "DCTN_PICTURE_SET_DECOMPRESS_MAX_SAMPLES", None)
    calls = []
    real_c, real_d = gpu.batch_compress_picture_set_n, gpu.batch_decompress_picture_set_n
    monkeypatch.setattr(gpu, "batch_compress_picture_set_n", lambda px, *a, **k: calls.append(("c", len(px))) or real_c(px, *a, **k))
    monkeypatch.setattr(gpu, "batch_decompress_picture_set_n", lambda b, *a, **k: calls.append(("d", len(b))) or real_d(b, *a, **k))
    return calls


def loop_compress(pipeline, images, cfg, colour):
    """The loop: every picture under ``cfg`` with its own width and height."""
    out = []
    for im in images:
        codec = pipeline.Jpeg(pipeline.Configuration(width=im.width, height=im.height, block_size=cfg.block_size, dct_size=cfg.dct_size,
                                                     transform=cfg.transform, quantization=cfg.quantization))
        out.append(codec.compress_rgb(im) if colour else codec.compress(im))
    return out


@pytest.mark.parametrize("n,bs,mode,param,sizes", CONFIGS, ids=["N%d-bs%d-%s%g" % c[:4] for c in CONFIGS])
@pytest.mark.parametrize("colour", [None, "rgb"])
def test_both_ways_equal_the_loop(gpu, road, monkeypatch, colour, n, bs, mode, param, sizes):
    import pipeline
    cfg = config_of(n, bs, mode, param, 1, 1)             # its own width and height are not read
    mode_name = "RGB" if colour else "YCbCr"
    images = images_of([n, bs], sizes, mode_name)
    want = loop_compress(pipeline, images, cfg, colour)
    assert road == []
    assert pipeline.compress_picture_set(images, cfg, colour=colour) == want
    assert road == [("c", 7)], "the set road did not run"
    del road[:]
    loop = [np.asarray(pipeline.Jpeg.decompress_rgb(c) if colour else pipeline.Jpeg.decompress(c)) for c in want]
    back = pipeline.decompress_picture_set_u8(want, colour=colour)
    assert road == [("d", 7)], "the set road did not run"
    assert len(back) == 7
    for got, ref, (r, c) in zip(back, loop, sizes):
        assert got.dtype == ref.dtype == np.uint8 and got.shape == ref.shape == (r, c, 3) and np.array_equal(got, ref)
    ims = pipeline.decompress_picture_set(want, colour=colour)
    assert [im.mode for im in ims] == [mode_name] * 7
    for im, ref in zip(ims, loop):
        assert np.array_equal(np.asarray(im), ref)
    # with the gate at None the road is off, and the results are the same
    del road[:]
    monkeypatch.setattr(pipeline, "DCTN_PICTURE_SET_MIN_PICTURES", None)
    assert pipeline.compress_picture_set(images, cfg, colour=colour) == want
    assert all(np.array_equal(a, b) for a, b in zip(pipeline.decompress_picture_set_u8(want, colour=colour), loop))
    assert road == []


@pytest.mark.parametrize("colour", [None, "rgb"])
def test_a_small_and_a_grey_picture_in_the_middle_come_back_in_place(gpu, road, colour):
    """A picture whose planes hold fewer than DCTN_MIN_SAMPLES samples and a grey one stay on the loop; the other five go as
    one set; the results are the loop's, in input order."""
    import pipeline
    n, bs, mode, param = 4, 1, "divide", 40.0
    cfg = config_of(n, bs, mode, param, 1, 1)
    mode_name = "RGB" if colour else "YCbCr"
    images = images_of(11, SIZES[:5], mode_name)
    images.insert(2, images_of(12, [(20, 24)], mode_name)[0])             # 480 samples a plane
    images.insert(4, Image.fromarray(np.random.default_rng(13).integers(0, 256, (40, 56), dtype=np.uint8), mode="L"))
    outcomes = []
    for call in (lambda: loop_compress(pipeline, images, cfg, colour), lambda: pipeline.compress_picture_set(images, cfg, colour=colour)):
        del road[:]
        try:
            outcomes.append(call())
        except Exception as exc:                          # whatever the loop makes of the grey picture, the function makes of it
            outcomes.append((type(exc), str(exc)))
    assert outcomes[0] == outcomes[1]
    if isinstance(outcomes[0], list):
        assert road == [("c", 5)]
    # the way back with the small picture's container in the middle
    boxes = loop_compress(pipeline, images[:4] + images[5:], cfg, colour)
    del road[:]
    back = pipeline.decompress_picture_set_u8(boxes, colour=colour)
    assert road == [("d", 5)]
    for got, c in zip(back, boxes):
        assert np.array_equal(got, np.asarray(pipeline.Jpeg.decompress_rgb(c) if colour else pipeline.Jpeg.decompress(c)))
