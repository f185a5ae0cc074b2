"""GPU: pipeline.compress_pictures / decompress_pictures_u8 / decompress_pictures at dct_size 8 on the batch road, with
DCT8_PICTURE_BATCH_MIN_PICTURES set to 2, against the loop over Jpeg.compress / compress_rgb / decompress / decompress_rgb, byte
for byte and sample for sample: at the command line's default (block_size 4, qtable; the uint8 road) and at block_size 3 with
divide 7 (the float64 road), the pictures as PIL images and as one array, both colours.  A recording wrapper around the
jpegx conveniences proves that the road ran."""
import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu

ROWS, COLS, COUNT = 45, 70, 4
CONFIGS = [(4, "qtable", {}), (3, "divide", {"divisor": 7})]


def pixels_of(seed):
    px = np.random.default_rng(seed).integers(0, 256, (COUNT, ROWS, COLS, 3), dtype=np.uint8)
    y, x = np.mgrid[0:ROWS, 0:COLS]
    for k in range(3):
        px[1, :, :, k] = ((5 * y + 3 * x + 60 * k) // 2 % 256).astype(np.uint8)
    return px


@pytest.fixture
def road(gpu, monkeypatch):
    """The gate at 2 pictures, no plane limit; the calls of the two conveniences are recorded."""
    import pipeline
    monkeypatch.setattr(pipeline, "DCT8_PICTURE_BATCH_MIN_PICTURES", 2)
    monkeypatch.setattr(pipeline, "DCT8_PICTURE_BATCH_COMPRESS_MAX_SAMPLES", None)
    monkeypatch.setattr(pipeline, "DCT8_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES", None)
    calls = []
    real_c, real_d = gpu.batch_compress_pictures, gpu.batch_decompress_pictures
    monkeypatch.setattr(gpu, "batch_compress_pictures", lambda *a, **k: calls.append("c") or real_c(*a, **k))
    monkeypatch.setattr(gpu, "batch_decompress_pictures", lambda *a, **k: calls.append("d") or real_d(*a, **k))
    return calls


@pytest.mark.parametrize("bs,mode,kw", CONFIGS, ids=["bs4-qtable", "bs3-divide7"])
@pytest.mark.parametrize("colour", [None, "rgb"])
def test_both_ways_equal_the_loop(gpu, road, monkeypatch, colour, bs, mode, kw):
    import pipeline
    cfg = pipeline.Configuration(width=COLS, height=ROWS, block_size=bs, dct_size=8, quantization=pipeline.QuantizationMethod(mode, **kw))
    px = pixels_of([bs, len(mode)])
    mode_name = "RGB" if colour else "YCbCr"
    images = [Image.fromarray(a, mode=mode_name) for a in px]
    codec = pipeline.Jpeg(cfg)
    want = [codec.compress_rgb(im) if colour else codec.compress(im) for im in images]
    assert road == []
    assert pipeline.compress_pictures(images, cfg, colour=colour) == want            # PIL images
    assert pipeline.compress_pictures(px, cfg, colour=colour) == want                # the array form
    assert road == ["c", "c"], "the batch road did not run"
    del road[:]
    loop = [np.asarray(pipeline.Jpeg.decompress_rgb(c) if colour else pipeline.Jpeg.decompress(c)) for c in want]
    back = pipeline.decompress_pictures_u8(want, colour=colour)
    assert road == ["d"], "the batch road did not run"
    assert len(back) == COUNT
    for got, ref in zip(back, loop):
        assert got.dtype == ref.dtype == np.uint8 and got.shape == ref.shape == (ROWS, COLS, 3) and np.array_equal(got, ref)
    ims = pipeline.decompress_pictures(want, colour=colour)
    assert [im.mode for im in ims] == [mode_name] * COUNT
    for im, ref in zip(ims, loop):
        assert np.array_equal(np.asarray(im), ref)
    # at the shipped gate the road is off, and the results are the same
    del road[:]
    monkeypatch.setattr(pipeline, "DCT8_PICTURE_BATCH_MIN_PICTURES", None)
    assert pipeline.compress_pictures(images, cfg, colour=colour) == want
    assert all(np.array_equal(a, b) for a, b in zip(pipeline.decompress_pictures_u8(want, colour=colour), loop))
    assert road == []
