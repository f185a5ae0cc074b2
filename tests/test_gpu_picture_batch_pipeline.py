"""GPU: pipeline.compress_pictures / decompress_pictures_u8 / decompress_pictures on the batch road against the loop over
Jpeg.compress / compress_rgb / decompress / decompress_rgb, byte for byte and sample for sample.  The three gates are set so
that 4 pictures of 40 x 56 take the road; a recording wrapper around the jpegx conveniences proves that it ran."""
import numpy as np
import pytest
from PIL import Image

from test_codec_oracle_n import config_of

pytestmark = pytest.mark.gpu

ROWS, COLS, COUNT = 40, 56, 4
# block_size 1 throughout: at 40 x 56 any pooling leaves planes below DCTN_MIN_SAMPLES, which are the loop's
CONFIGS = [(4, 1, "divide", 40.0), (16, 1, "divide", 40.0), (3, 1, "discard", 4.0), (24, 1, "divide", 1000.0)]


def pixels_of(seed):
    px = np.random.default_rng(seed).integers(0, 256, (COUNT, ROWS, COLS, 3), dtype=np.uint8)
    y, x = np.mgrid[0:ROWS, 0:COLS]
    for k in range(3):
        px[1, :, :, k] = ((5 * y + 3 * x + 60 * k) // 2 % 256).astype(np.uint8)
    return px


@pytest.fixture
def road(gpu, monkeypatch):
    """The gates open for 4 pictures of 40 x 56; the calls of the two conveniences are recorded."""
    import pipeline
    monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_MIN_PICTURES", 4)
    monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES", 48 * 72)        # 40 x 56 after both paddings at N 24
    monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES", 48 * 72)
    calls = []
    real_c, real_d = gpu.batch_compress_pictures_n, gpu.batch_decompress_pictures_n
    monkeypatch.setattr(gpu, "batch_compress_pictures_n", lambda *a, **k: calls.append("c") or real_c(*a, **k))
    monkeypatch.setattr(gpu, "batch_decompress_pictures_n", lambda *a, **k: calls.append("d") or real_d(*a, **k))
    return calls


@pytest.mark.parametrize("n,bs,mode,param", CONFIGS)
@pytest.mark.parametrize("colour", [None, "rgb"])
def test_both_ways_equal_the_loop(gpu, road, monkeypatch, colour, n, bs, mode, param):
    import pipeline
    cfg = config_of(n, bs, mode, param, ROWS, COLS)
    px = pixels_of([n, bs])
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
    # with the gate at None the road is off, and the results are the same
    del road[:]
    monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_MIN_PICTURES", None)
    assert pipeline.compress_pictures(images, cfg, colour=colour) == want
    assert all(np.array_equal(a, b) for a, b in zip(pipeline.decompress_pictures_u8(want, colour=colour), loop))
    assert road == []


def test_mixed_sizes_give_the_loops_result(gpu, road):
    import pipeline
    cfg = config_of(4, 1, "divide", 40.0, ROWS, COLS)
    px = pixels_of(9)
    images = [Image.fromarray(a, mode="RGB") for a in px]
    images[2] = images[2].crop((0, 0, COLS - 1, ROWS))
    codec = pipeline.Jpeg(cfg)
    outcomes = []
    for call in (lambda: [codec.compress_rgb(im) for im in images], lambda: pipeline.compress_pictures(images, cfg, colour="rgb")):
        try:
            outcomes.append(call())
        except Exception as exc:                          # whatever the loop makes of the odd picture, the function makes of it
            outcomes.append((type(exc), str(exc)))
    assert outcomes[0] == outcomes[1]
    assert road == []
    # containers of two configurations
    other = config_of(4, 1, "divide", 40.0, ROWS, COLS - 1)
    a = codec.compress_rgb(images[0])
    b = pipeline.Jpeg(other).compress_rgb(images[2])
    boxes = [a, a, b, a]
    back = pipeline.decompress_pictures_u8(boxes, colour="rgb")
    assert road == []
    for got, c in zip(back, boxes):
        assert np.array_equal(got, np.asarray(pipeline.Jpeg.decompress_rgb(c)))
