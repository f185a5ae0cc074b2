"""What pipeline.probe_picture_set_sizes and compress_picture_set_to_size decide: which pictures they send to libjpegx's set
probe and with which arguments, what they make of its answer, and which pictures go through the literal loop over
Jpeg.compress / compress_rgb under a configuration of the picture's own size.  The set probe is a recording fake that answers
from the loop's own containers, so no device is needed.  CPU only."""
import numpy as np
import pytest
from PIL import Image

import file_format
import jpegx
import pipeline
import util


def _config(n=4, bs=1, divisor=40, rows=1, cols=1):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def _picture(rows, cols, mode="RGB", seed=0):
    rng = np.random.default_rng([rows, cols, seed])
    yy, xx = np.mgrid[0:rows, 0:cols]
    smooth = (yy * 3 + xx * 2) % 256
    noise = rng.integers(0, 256, (rows, cols, 3))
    px = np.where((xx < cols // 2)[..., None], smooth[..., None] + np.arange(3) * 20, noise) % 256
    return Image.fromarray(px.astype(np.uint8), mode=mode)


def _one(im, config, d, colour):
    """len(Jpeg(config_ij).compress(im)), -1 for BadRleCodeError: the literal loop's cell, spelled out here."""
    codec = pipeline.Jpeg(_config(config.dct_size, config.block_size, d, im.height, im.width))
    try:
        return len(codec.compress(im) if colour is None else codec.compress_rgb(im))
    except util.BadRleCodeError:
        return -1


def _loop(images, config, divisors, colour):
    return np.array([[_one(im, config, d, colour) for d in divisors] for im in images], dtype=np.int64).reshape(len(images), len(divisors))


# 40 x 99 and 40 x 100: the same planes of blocks, widths of two and three digits; 20 x 24 lies below DCTN_MIN_SAMPLES
SIZES = [(40, 99), (40, 100), (20, 24), (64, 48), (33, 70)]


def _mixed(colour):
    mode = "YCbCr" if colour is None else "RGB"
    ims = [_picture(r, c, mode) for r, c in SIZES]
    ims.insert(3, Image.fromarray(np.asarray(_picture(30, 30))[..., 0], mode="L"))      # a grey picture
    return ims


def _synthetic(config, im):
    assert (config.height, config.width) == (im.height, im.width), "the loop must size the configuration to the picture"
    divisor = config.quantization.gpu_mode()[1]
    body = 3 + (int(np.asarray(im).astype(np.int64).sum()) % 1000 + im.height * im.width * len(im.getbands())) // int(divisor)
    return file_format.generate_data(config, pipeline.CompressedData(b"y" * body, b"cb", b"r"))


class Fake:
    """jpegx.batch_probe_picture_set_n: records its arguments and answers with the band sizes that make the loop's containers
    -- the container's length less the header length its first two bytes state and the 12 bytes of prefixes, all in band 0."""

    def __init__(self, monkeypatch, colour, fail=None, bad=()):
        self.calls, self.colour, self.fail, self.bad = [], colour, fail, set(bad)
        monkeypatch.setattr(pipeline, "_device_usable", lambda: True)
        monkeypatch.setattr(pipeline, "DCTN_PROBE_MIN_CANDIDATES", 2)
        monkeypatch.setattr(pipeline, "DCTN_PROBE_SET_MIN_PICTURES", 1)
        monkeypatch.setattr(jpegx, "batch_probe_picture_set_n", self)
        # the loop's two methods, so that no road of theirs asks for the device the test pretends to have: a container of the
        # configuration's own header and a first band whose length falls with the divisor and depends on the pixels
        monkeypatch.setattr(pipeline.Jpeg, "compress", lambda codec, im: _synthetic(codec.config, im))
        monkeypatch.setattr(pipeline.Jpeg, "compress_rgb", lambda codec, im: _synthetic(codec.config, im))

    def __call__(self, pictures, bs, n, mode, params, **kw):
        self.calls.append((pictures, bs, n, mode, list(params), kw))
        if self.fail:
            raise jpegx.JpegxError(self.fail)
        sizes = np.zeros((len(pictures), 3, len(params)), np.uint64)
        bad = np.zeros(sizes.shape, bool)
        for p, px in enumerate(pictures):
            im = Image.fromarray(px, mode="YCbCr" if self.colour is None else "RGB")
            for q, d in enumerate(params):
                codec = pipeline.Jpeg(_config(n, bs, int(d), im.height, im.width))
                box = codec.compress(im) if self.colour is None else codec.compress_rgb(im)
                sizes[p, 0, q] = len(box) - file_format.unpack_integer(box[:2]) - 12
                bad[p, 1, q] = (p, d) in self.bad
        return sizes, bad


def test_without_a_device_it_is_the_loop(monkeypatch):
    monkeypatch.setattr(pipeline, "_device_usable", lambda: False)
    monkeypatch.setattr(jpegx, "batch_probe_picture_set_n", lambda *a, **k: pytest.fail("no device: the set probe must not be called"))
    ims = _mixed("rgb")
    divisors = [1, 8, 1000]
    got = pipeline.probe_picture_set_sizes(ims, _config(), divisors, colour="rgb")
    assert got.dtype == np.int64 and got.shape == (6, 3)
    assert np.array_equal(got, _loop(ims, _config(), divisors, "rgb"))
    assert (got > 0).all() and (np.diff(got, axis=1) < 0).all()
    # config's own width and height are not read
    assert np.array_equal(got, pipeline.probe_picture_set_sizes(iter(ims), _config(rows=7, cols=9), divisors, colour="rgb"))
    assert pipeline.probe_picture_set_sizes([], _config(), [2, 3]).shape == (0, 2)
    assert pipeline.probe_picture_set_sizes(ims[:1], _config(), [], colour="rgb").shape == (1, 0)


def test_bad_rle_is_minus_one_in_the_loop(monkeypatch):
    monkeypatch.setattr(pipeline, "_device_usable", lambda: False)
    yy, xx = np.mgrid[0:60, 0:60]
    board = Image.fromarray(np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2), mode="YCbCr")
    ims = [board, _picture(30, 60, "YCbCr")]
    got = pipeline.probe_picture_set_sizes(ims, _config(30), [1, 64])
    assert got[0, 0] == -1 and (got[:, 1] > 0).all()
    assert np.array_equal(got, _loop(ims, _config(30), [1, 64], None))


@pytest.mark.parametrize("colour", [None, "rgb"])
def test_only_admitted_pictures_go_and_rows_come_back_in_place(monkeypatch, colour):
    f = Fake(monkeypatch, colour)
    ims = _mixed(colour) if colour else [im for im in _mixed(colour) if im.mode != "L"]
    divisors = [2, 40]
    got = pipeline.probe_picture_set_sizes(ims, _config(), divisors, colour=colour)
    admitted = [at for at, im in enumerate(ims) if im.mode != "L" and im.height * im.width >= 1024]
    assert len(admitted) == 4 and len(f.calls) == 1
    pictures, bs, n, mode, params, kw = f.calls[0]
    assert (bs, n, mode, params) == (1, 4, "divide", [2.0, 40.0]) and kw == ({} if colour is None else {"colour": "rgb"})
    assert len(pictures) == 4 and all(np.array_equal(px, np.asarray(ims[at])) and px.dtype == np.uint8 for px, at in zip(pictures, admitted))
    assert np.array_equal(got, _loop(ims, _config(), divisors, colour))
    # headers are counted per picture: the two pictures of one plane shape and unlike widths differ by their content alone
    for at in admitted:
        im = ims[at]
        head = len(file_format.create_header(_config(4, 1, 40, im.height, im.width)))
        assert got[at, 1] == int(f(pictures[admitted.index(at):admitted.index(at) + 1], 1, 4, "divide", [40.0])[0][0, 0, 0]) + head + 12


def test_thirty_three_divisors_arrive_as_32_and_1_in_order(monkeypatch):
    f = Fake(monkeypatch, None)
    ims = [_picture(40, 99, "YCbCr"), _picture(40, 100, "YCbCr")]
    divisors = [3 * k + 1 for k in range(33)]
    got = pipeline.probe_picture_set_sizes(ims, _config(), divisors)
    assert [c[4] for c in f.calls] == [[float(d) for d in divisors[:32]], [float(divisors[32])]]
    assert got.shape == (2, 33) and np.array_equal(got[:, [0, 32]], _loop(ims, _config(), [1, 97], None))
    assert np.array_equal(got, _loop(ims, _config(), divisors, None)) and got[0, 0] > got[0, 32]


def test_minus_one_lands_where_bad_is_set(monkeypatch):
    f = Fake(monkeypatch, None, bad={(1, 8.0)})
    ims = [_picture(40, 99, "YCbCr"), _picture(40, 100, "YCbCr"), _picture(64, 48, "YCbCr")]
    got = pipeline.probe_picture_set_sizes(ims, _config(), [2, 8, 40])
    want = _loop(ims, _config(), [2, 8, 40], None)
    want[1, 1] = -1
    assert np.array_equal(got, want)


@pytest.mark.parametrize("text", ["jpegx_batch_probe_picture_set_n failed: hipErrorOutOfMemory", "the set was refused"])
def test_a_refusal_is_the_loop(monkeypatch, text):
    f = Fake(monkeypatch, None, fail=text)
    ims = [_picture(40, 99, "YCbCr"), _picture(64, 48, "YCbCr")]
    got = pipeline.probe_picture_set_sizes(ims, _config(), [2, 40])
    assert len(f.calls) == 1 and np.array_equal(got, _loop(ims, _config(), [2, 40], None))


def test_the_gates_are_read_when_the_function_is_called(monkeypatch):
    ims = [_picture(40, 99, "YCbCr"), _picture(64, 48, "YCbCr")]
    Fake(monkeypatch, None)                                 # the loop's methods are the synthetic ones from here on
    want = _loop(ims, _config(), [2, 40], None)
    for name, value, divisors in (("DCTN_PROBE_SET_MIN_PICTURES", None, [2, 40]), ("DCTN_PROBE_SET_MIN_PICTURES", 3, [2, 40]),
                                  ("DCTN_PROBE_MIN_CANDIDATES", None, [2, 40]), ("DCTN_PROBE_MIN_CANDIDATES", 3, [2, 40]),
                                  ("DCTN_PROBE_MIN_CANDIDATES", 2, [40])):
        f = Fake(monkeypatch, None)
        monkeypatch.setattr(pipeline, name, value)
        got = pipeline.probe_picture_set_sizes(ims, _config(), divisors)
        assert not f.calls, (name, value, divisors)
        assert np.array_equal(got, want[:, -len(divisors):])
    f = Fake(monkeypatch, None)
    monkeypatch.setattr(pipeline, "DCTN_PROBE_SET_MIN_PICTURES", 2)
    pipeline.probe_picture_set_sizes(ims, _config(), [2, 40])
    pipeline.probe_picture_set_sizes(ims + [_picture(20, 24, "YCbCr")], _config(), [2, 40])      # still two admitted
    pipeline.probe_picture_set_sizes(ims[:1] + [_picture(20, 24, "YCbCr")], _config(), [2, 40])  # one admitted: the loop
    assert [len(c[0]) for c in f.calls] == [2, 2]
    # dct_size 8 and quantisers other than 'divide'
    f = Fake(monkeypatch, None)
    pipeline.probe_picture_set_sizes(ims[:1], _config(8), [2, 40])
    assert not f.calls


def test_value_errors():
    ims = [_picture(20, 24, "YCbCr")]
    for name, kw in (("none", {}), ("discard", {"keep": 2})):
        config = pipeline.Configuration(width=1, height=1, block_size=1, dct_size=4, quantization=pipeline.QuantizationMethod(name, **kw))
        with pytest.raises(ValueError, match="must be 'divide'"):
            pipeline.probe_picture_set_sizes(ims, config, [2])
        with pytest.raises(ValueError, match="must be 'divide'"):
            pipeline.compress_picture_set_to_size(ims, config, 1000, [2])
    for bad in (2.5, 0, -3, float("nan"), float("inf"), "7", True, None):
        with pytest.raises(ValueError, match="whole positive number"):
            pipeline.probe_picture_set_sizes(ims, _config(), [4, bad])
    with pytest.raises(ValueError, match="colour"):
        pipeline.probe_picture_set_sizes(ims, _config(), [4], colour="bgr")
    for ladder in ([8, 4], [4, 4], [], list(range(1, 34))):
        with pytest.raises(ValueError, match="1..32 ascending rungs"):
            pipeline.compress_picture_set_to_size(ims, _config(), 10 ** 6, ladder)


# ---- compress_picture_set_to_size ---------------------------------------------------------------------------------------------
LADDER = [2, 8, 40, 200]


@pytest.mark.parametrize("colour", [None, "rgb"])
def test_every_picture_gets_its_smallest_fitting_rung(monkeypatch, colour):
    monkeypatch.setattr(pipeline, "_device_usable", lambda: False)
    ims = _mixed(colour) if colour else [im for im in _mixed(colour) if im.mode != "L"]
    sizes = _loop(ims, _config(), LADDER, colour)
    budget = int(np.sort(sizes[:, 1])[len(ims) // 2])       # the median size under the second rung: some fit it, some do not
    want = [next(j for j, s in enumerate(row) if s <= budget) for row in sizes]
    assert len(set(want)) >= 2
    calls = []
    real = pipeline.probe_picture_set_sizes
    monkeypatch.setattr(pipeline, "probe_picture_set_sizes", lambda *a, **k: calls.append(1) or real(*a, **k))
    containers, chosen = pipeline.compress_picture_set_to_size(ims, _config(), budget, LADDER, colour=colour)
    assert len(calls) == 1 and chosen == [LADDER[j] for j in want]
    for im, box, d in zip(ims, containers, chosen):
        codec = pipeline.Jpeg(_config(4, 1, d, im.height, im.width))
        assert box == (codec.compress(im) if colour is None else codec.compress_rgb(im)) and len(box) <= budget


def test_target_size_error_names_the_first_picture_that_fits_no_rung(monkeypatch):
    monkeypatch.setattr(pipeline, "_device_usable", lambda: False)
    ims = [_picture(20, 24, "YCbCr"), _picture(64, 48, "YCbCr"), _picture(40, 99, "YCbCr")]
    sizes = _loop(ims, _config(), LADDER, None)
    budget = int(sizes[0, -1])                              # the small picture's last rung: the other two fit none
    assert (sizes[1:, -1] > budget).all()
    with pytest.raises(pipeline.TargetSizeError, match="picture 1 fits no rung within %d bytes: its smallest size is %d bytes, at divisor 200"
                       % (budget, sizes[1, -1])):
        pipeline.compress_picture_set_to_size(ims, _config(), budget, LADDER)


def test_a_container_that_is_not_the_probed_size_is_a_runtime_error(monkeypatch):
    monkeypatch.setattr(pipeline, "_device_usable", lambda: False)
    ims = [_picture(20, 24, "YCbCr"), _picture(64, 48, "YCbCr")]
    real = pipeline.probe_picture_set_sizes
    monkeypatch.setattr(pipeline, "probe_picture_set_sizes", lambda *a, **k: real(*a, **k) - 1)
    with pytest.raises(RuntimeError, match="picture 0 was probed at"):
        pipeline.compress_picture_set_to_size(ims, _config(), 10 ** 6, LADDER)
