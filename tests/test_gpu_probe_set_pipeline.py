"""pipeline.probe_picture_set_sizes and compress_picture_set_to_size on the device road: the sizes are those of the literal loop
over Jpeg.compress / compress_rgb under a configuration of each picture's own size, the admitted pictures go to the device as
one set, and the byte-budget function returns the loop's choice of rungs and the loop's containers."""
import numpy as np
import pytest
from PIL import Image

import pipeline
import util
from test_gpu_probe_pipeline import _picture

pytestmark = pytest.mark.gpu

# a dozen pictures with sides up to 160; 16 x 16 lies below DCTN_MIN_SAMPLES at every configuration used here
SIZES = [(64, 64), (40, 99), (40, 100), (16, 16), (160, 33), (57, 131), (64, 64), (100, 100), (35, 47), (128, 96), (33, 160), (71, 52)]


def _config(bs, n, divisor=40, rows=1, cols=1):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def _mixed(colour):
    mode = "YCbCr" if colour is None else "RGB"
    ims = [_picture(k, rows, cols, mode) for k, (rows, cols) in enumerate(SIZES)]
    if colour is not None:
        ims[8] = Image.fromarray(np.asarray(ims[8])[..., 0], mode="L")       # a grey picture: compress_rgb converts it, the set does not take it
        ims[10] = ims[10].convert("YCbCr")                                    # not RGB under colour='rgb'
    return ims


def _loop(images, bs, n, divisors, colour):
    out = np.empty((len(images), len(divisors)), np.int64)
    for i, im in enumerate(images):
        for j, d in enumerate(divisors):
            codec = pipeline.Jpeg(_config(bs, n, d, im.height, im.width))
            try:
                out[i, j] = len(codec.compress(im) if colour is None else codec.compress_rgb(im))
            except util.BadRleCodeError:
                out[i, j] = -1
    return out


@pytest.fixture
def set_calls(gpu, monkeypatch):
    """Counts the calls of jpegx.batch_probe_picture_set_n that the pipeline makes."""
    calls = []
    real = gpu.batch_probe_picture_set_n

    def counted(pictures, *args, **kwargs):
        calls.append(([p.shape[:2] for p in pictures], list(args[3])))
        return real(pictures, *args, **kwargs)

    monkeypatch.setattr(gpu, "batch_probe_picture_set_n", counted)
    monkeypatch.setattr(pipeline, "DCTN_PROBE_SET_MIN_PICTURES", 1)
    return calls


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, n, divisors", [(1, 4, [1, 8, 40, 1000]), (1, 16, [2, 8, 300]), (2, 3, [2, 9])])
def test_device_road_equals_the_loop_on_a_mixed_set(set_calls, bs, n, divisors, colour):
    images = _mixed(colour)
    got = pipeline.probe_picture_set_sizes(images, _config(bs, n), divisors, colour=colour)
    out = [at for at, im in enumerate(images) if im.mode == "L" or (colour is not None and im.mode != "RGB")
           or np.prod(pipeline._blocked_shape(im.height, im.width, bs, n)) < pipeline.DCTN_MIN_SAMPLES]
    assert 3 in out and (colour is None or {8, 10} <= set(out)) and len(out) <= 5
    admitted = [SIZES[at] for at in range(len(SIZES)) if at not in out]
    assert set_calls == [(admitted, [float(d) for d in divisors])]
    assert np.array_equal(got, _loop(images, bs, n, divisors, colour))


def test_a_minus_one_cell_and_thirty_three_divisors(set_calls):
    """dct_size 16: a block's DC is 256 times its mean, so the bright flat picture passes 16383 under the divisors 1 and 2 and
    codes from 5 on -- the loop raises BadRleCodeError, the probe says -1, in the same cells.  33 divisors are two passes of
    the set."""
    images = [_picture(2, 64, 48, "YCbCr"), Image.fromarray(np.full((40, 70, 3), 250, np.uint8), mode="YCbCr"), _picture(1, 16, 16, "YCbCr"),
              _picture(3, 50, 64, "YCbCr")]
    divisors = [1] + [3 * k + 2 for k in range(32)]
    got = pipeline.probe_picture_set_sizes(images, _config(1, 16), divisors)
    assert [len(c[1]) for c in set_calls] == [32, 1] and all(c[0] == [(64, 48), (40, 70), (50, 64)] for c in set_calls)
    check = [0, 1, 2, 31, 32]                               # the loop on five of the columns, every row
    want = _loop(images, 1, 16, [divisors[j] for j in check], None)
    assert want[1, :2].tolist() == [-1, -1] and (want[:, 2:] > 0).all()
    assert np.array_equal(got[:, check], want)
    assert (got[:, 2:] > 0).all()


@pytest.mark.parametrize("colour", [None, "rgb"])
def test_compress_picture_set_to_size_equals_the_loops_choice(set_calls, colour):
    images = _mixed(colour)
    ladder = [2, 8, 40, 200]
    sizes = _loop(images, 1, 4, ladder, colour)
    budget = int(sizes[:, -1].max())                         # what the heaviest picture weighs on the last rung: every picture fits one
    want = [next(j for j, s in enumerate(row) if s != -1 and s <= budget) for row in sizes]
    assert len(set(want)) >= 2
    containers, chosen = pipeline.compress_picture_set_to_size(images, _config(1, 4), budget, ladder, colour=colour)
    assert len(set_calls) == 1 and chosen == [ladder[j] for j in want]
    for im, box, d in zip(images, containers, chosen):
        codec = pipeline.Jpeg(_config(1, 4, d, im.height, im.width))
        assert box == (codec.compress(im) if colour is None else codec.compress_rgb(im)) and len(box) <= budget
    with pytest.raises(pipeline.TargetSizeError, match="picture %d fits no rung" % int(np.argmax(sizes[:, -1] > sizes[:, -1].min()))):
        pipeline.compress_picture_set_to_size(images, _config(1, 4), int(sizes[:, -1].min()), ladder, colour=colour)
