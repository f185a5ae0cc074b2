"""What pipeline.probe_picture_set_distortion and probe_picture_set_psnr decide: which pictures they send to libjpegx's set
distortion probe and with which arguments, what they make of its answer, and which pictures go through the literal loop over
Jpeg.compress / Jpeg.decompress under a configuration of the picture's own size.  The set probe is a recording fake that
answers from the same synthetic codec the loop is given, so no device is needed.  CPU only."""
import numpy as np
import pytest
from PIL import Image

import jpegx
import pipeline
import util


def _config(n=4, bs=1, divisor=40, rows=1, cols=1):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def _picture(rows, cols, mode="RGB", seed=0):
    rng = np.random.default_rng([rows, cols, seed])
    return Image.fromarray(rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8), mode=mode)


# 40 x 99 and 40 x 100: the same planes of blocks; 20 x 24 lies below DCTN_MIN_SAMPLES
SIZES = [(40, 99), (40, 100), (20, 24), (64, 48), (33, 70)]
BOARD = 251                                              # the synthetic codec cannot code a picture whose first byte is this under divisor 1


def _mixed(colour):
    mode = "YCbCr" if colour is None else "RGB"
    ims = [_picture(r, c, mode) for r, c in SIZES]
    ims.insert(3, Image.fromarray(np.asarray(_picture(30, 30))[..., 0], mode="L"))      # a grey picture
    return ims


def _decoded(px, d):
    """The synthetic codec's loss: every byte rounded down to a multiple of the divisor (none at divisor 1)."""
    return (np.asarray(px).astype(np.int64) // int(d)) * int(d)


def _sse(px, d):
    px = np.asarray(px).astype(np.int64)
    return ((px - _decoded(px, d)) ** 2).reshape(-1, px.shape[-1] if px.ndim == 3 else 1).sum(axis=0)


def _compress(codec, im):
    assert (codec.config.height, codec.config.width) == (im.height, im.width), "the loop must size the configuration to the picture"
    px = np.asarray(im)
    if px.reshape(-1)[0] == BOARD and codec.config.quantization.gpu_mode()[1] == 1:
        raise util.BadRleCodeError("synthetic")
    return (im.mode, px)


def _decompress(codec, box):
    mode, px = box
    return Image.fromarray(_decoded(px, codec.config.quantization.gpu_mode()[1]).astype(np.uint8), mode=mode)


def _cell(im, d, colour):
    x = im if colour is None else im.convert("YCbCr")
    px = np.asarray(x)
    if px.reshape(-1)[0] == BOARD and d == 1:
        return np.full(3, -1, np.int64)
    return np.broadcast_to(_sse(px, d), (3,))


def _loop(images, divisors, colour):
    return np.array([[_cell(im, d, colour) for d in divisors] for im in images], np.int64).reshape(len(images), len(divisors), 3).transpose(0, 2, 1)


class Fake:
    """jpegx.batch_probe_distortion_picture_set_n: records its arguments and answers with the synthetic codec's sums."""

    def __init__(self, monkeypatch, colour, fail=None, bad=()):
        self.calls, self.colour, self.fail, self.bad = [], colour, fail, set(bad)
        monkeypatch.setattr(pipeline, "_device_usable", lambda: True)
        monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", 1)
        monkeypatch.setattr(pipeline, "DCTN_DISTORTION_SET_MIN_PICTURES", 1)
        monkeypatch.setattr(jpegx, "batch_probe_distortion_picture_set_n", self)
        monkeypatch.setattr(jpegx, "batch_probe_picture_set_n", lambda *a, **k: pytest.fail("the size probe is another road"))
        # the loop's two methods, so that no road of theirs asks for the device the test pretends to have
        monkeypatch.setattr(pipeline.Jpeg, "compress", _compress)
        monkeypatch.setattr(pipeline.Jpeg, "decompress", _decompress)

    def __call__(self, pictures, bs, n, mode, params, **kw):
        self.calls.append((pictures, bs, n, mode, list(params), kw))
        if self.fail:
            raise jpegx.JpegxError(self.fail)
        sse = np.zeros((len(pictures), 3, len(params)), np.uint64)
        bad = np.zeros(sse.shape, bool)
        for p, px in enumerate(pictures):
            x = px if self.colour is None else np.asarray(Image.fromarray(px, mode="RGB").convert("YCbCr"))
            for q, d in enumerate(params):
                sse[p, :, q] = _sse(x, d)
                bad[p, 1, q] = (p, d) in self.bad
        return sse, bad


def test_without_a_device_it_is_the_loop(monkeypatch):
    Fake(monkeypatch, "rgb")
    monkeypatch.setattr(pipeline, "_device_usable", lambda: False)
    monkeypatch.setattr(jpegx, "batch_probe_distortion_picture_set_n", lambda *a, **k: pytest.fail("no device: the set probe must not be called"))
    ims = _mixed("rgb")
    divisors = [1, 7, 100]                               # a grey picture's chroma is 128: no multiple of 7 or 100
    got = pipeline.probe_picture_set_distortion(ims, _config(), divisors, colour="rgb")
    assert got.dtype == np.int64 and got.shape == (6, 3, 3)
    assert np.array_equal(got, _loop(ims, divisors, "rgb"))
    assert (got[:, :, 0] == 0).all() and (got[:, :, 1:] > 0).all()
    # config's own width and height are not read
    assert np.array_equal(got, pipeline.probe_picture_set_distortion(iter(ims), _config(rows=7, cols=9), divisors, colour="rgb"))
    assert pipeline.probe_picture_set_distortion([], _config(), [2, 3]).shape == (0, 3, 2)
    assert pipeline.probe_picture_set_distortion(ims[:1], _config(), [], colour="rgb").shape == (1, 3, 0)


@pytest.mark.parametrize("colour", [None, "rgb"])
def test_only_admitted_pictures_go_and_rows_come_back_in_place(monkeypatch, colour):
    f = Fake(monkeypatch, colour)
    ims = _mixed(colour) if colour else [im for im in _mixed(colour) if im.mode != "L"]
    divisors = [2, 40]
    got = pipeline.probe_picture_set_distortion(ims, _config(), divisors, colour=colour)
    admitted = [at for at, im in enumerate(ims) if im.mode != "L" and im.height * im.width >= 1024]
    assert len(admitted) == 4 and len(f.calls) == 1
    pictures, bs, n, mode, params, kw = f.calls[0]
    assert (bs, n, mode, params) == (1, 4, "divide", [2.0, 40.0]) and kw == ({} if colour is None else {"colour": "rgb"})
    assert len(pictures) == 4 and all(np.array_equal(px, np.asarray(ims[at])) and px.dtype == np.uint8 for px, at in zip(pictures, admitted))
    assert np.array_equal(got, _loop(ims, divisors, colour))


def test_thirty_three_divisors_arrive_as_32_and_1_in_order(monkeypatch):
    f = Fake(monkeypatch, None)
    ims = [_picture(40, 99, "YCbCr"), _picture(40, 100, "YCbCr")]
    divisors = [3 * k + 1 for k in range(33)]
    got = pipeline.probe_picture_set_distortion(ims, _config(), divisors)
    assert [c[4] for c in f.calls] == [[float(d) for d in divisors[:32]], [float(divisors[32])]]
    assert got.shape == (2, 3, 33) and np.array_equal(got, _loop(ims, divisors, None))


def test_bad_in_one_band_is_minus_one_in_all_three(monkeypatch):
    Fake(monkeypatch, None, bad={(1, 8.0)})
    ims = [_picture(40, 99, "YCbCr"), _picture(40, 100, "YCbCr"), _picture(64, 48, "YCbCr")]
    got = pipeline.probe_picture_set_distortion(ims, _config(), [2, 8, 40])
    want = _loop(ims, [2, 8, 40], None)
    want[1, :, 1] = -1
    assert np.array_equal(got, want)
    psnr = pipeline.probe_picture_set_psnr(ims, _config(), [2, 8, 40])
    assert np.isnan(psnr[1, 1]) and np.isnan(psnr).sum() == 1


def test_bad_rle_is_minus_one_in_the_loop(monkeypatch):
    f = Fake(monkeypatch, None)
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_SET_MIN_PICTURES", None)
    px = np.asarray(_picture(40, 50, "YCbCr")).copy()
    px[0, 0, 0] = BOARD
    ims = [Image.fromarray(px, mode="YCbCr"), _picture(30, 60, "YCbCr")]
    got = pipeline.probe_picture_set_distortion(ims, _config(), [1, 64])
    assert not f.calls and (got[0, :, 0] == -1).all() and (got[1, :, 0] == 0).all() and (got[:, :, 1] > 0).all()


@pytest.mark.parametrize("text", ["jpegx_batch_probe_distortion_picture_set_n failed: hipErrorOutOfMemory", "the set was refused"])
def test_a_refusal_is_the_loop_for_every_row(monkeypatch, text):
    f = Fake(monkeypatch, None, fail=text)
    ims = [_picture(40, 99, "YCbCr"), _picture(20, 24, "YCbCr"), _picture(64, 48, "YCbCr")]
    got = pipeline.probe_picture_set_distortion(ims, _config(), [2, 40])
    assert len(f.calls) == 1 and np.array_equal(got, _loop(ims, [2, 40], None))


def test_the_gates_are_read_when_the_function_is_called(monkeypatch):
    ims = [_picture(40, 99, "YCbCr"), _picture(64, 48, "YCbCr")]
    want = _loop(ims, [2, 40], None)
    for name, value, divisors in (("DCTN_DISTORTION_SET_MIN_PICTURES", None, [2, 40]), ("DCTN_DISTORTION_SET_MIN_PICTURES", 3, [2, 40]),
                                  ("DCTN_DISTORTION_MIN_CANDIDATES", None, [2, 40]), ("DCTN_DISTORTION_MIN_CANDIDATES", 3, [2, 40]),
                                  ("DCTN_DISTORTION_MIN_CANDIDATES", 2, [40])):
        f = Fake(monkeypatch, None)
        monkeypatch.setattr(pipeline, name, value)
        got = pipeline.probe_picture_set_distortion(ims, _config(), divisors)
        assert not f.calls, (name, value, divisors)
        assert np.array_equal(got, want[:, :, -len(divisors):])
    # at their values
    f = Fake(monkeypatch, None)
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", 2)
    monkeypatch.setattr(pipeline, "DCTN_DISTORTION_SET_MIN_PICTURES", 2)
    assert np.array_equal(pipeline.probe_picture_set_distortion(ims, _config(), [2, 40]), want)
    pipeline.probe_picture_set_distortion(ims + [_picture(20, 24, "YCbCr")], _config(), [2, 40])      # still two admitted
    pipeline.probe_picture_set_distortion(ims[:1] + [_picture(20, 24, "YCbCr")], _config(), [2, 40])  # one admitted: the loop
    assert [len(c[0]) for c in f.calls] == [2, 2]
    # the size probe's gates are not this road's
    f = Fake(monkeypatch, None)
    monkeypatch.setattr(pipeline, "DCTN_PROBE_SET_MIN_PICTURES", None)
    monkeypatch.setattr(pipeline, "DCTN_PROBE_MIN_CANDIDATES", None)
    pipeline.probe_picture_set_distortion(ims, _config(), [2])
    assert len(f.calls) == 1
    # dct_size 8
    f = Fake(monkeypatch, None)
    pipeline.probe_picture_set_distortion(ims[:1], _config(8), [2, 40])
    assert not f.calls


def test_the_shipped_gate_is_none_or_a_positive_count():
    gate = pipeline.DCTN_DISTORTION_SET_MIN_PICTURES
    assert gate is None or (isinstance(gate, int) and gate >= 1)


def test_psnr_uses_each_pictures_own_size(monkeypatch):
    ims = [_picture(40, 99, "YCbCr"), _picture(64, 48, "YCbCr"), _picture(20, 24, "YCbCr")]
    sse = np.array([[[0, 100], [0, 200], [0, 300]], [[7, -1], [8, -1], [9, -1]], [[600, 0], [0, 0], [0, 0]]], np.int64)
    monkeypatch.setattr(pipeline, "probe_picture_set_distortion", lambda images, config, divisors, colour=None: sse)
    got = pipeline.probe_picture_set_psnr(iter(ims), _config(rows=3, cols=3), [2, 40])
    assert got.dtype == np.float64 and got.shape == (3, 2)
    assert got[0, 0] == np.inf and got[2, 1] == np.inf and np.isnan(got[1, 1])
    assert got[0, 1] == pytest.approx(10 * np.log10(255.0 ** 2 * 3 * 40 * 99 / 600))
    assert got[1, 0] == pytest.approx(10 * np.log10(255.0 ** 2 * 3 * 64 * 48 / 24))
    assert got[2, 0] == pytest.approx(10 * np.log10(255.0 ** 2 * 3 * 20 * 24 / 600))
    assert got[0, 1] != got[2, 0]                         # the same sum, unlike sizes


def test_value_errors():
    ims = [_picture(20, 24, "YCbCr")]
    for name, kw in (("none", {}), ("discard", {"keep": 2})):
        config = pipeline.Configuration(width=1, height=1, block_size=1, dct_size=4, quantization=pipeline.QuantizationMethod(name, **kw))
        with pytest.raises(ValueError, match="must be 'divide'"):
            pipeline.probe_picture_set_distortion(ims, config, [2])
    for bad in (2.5, 0, -3, float("nan"), "7", True, None):
        with pytest.raises(ValueError, match="whole positive number"):
            pipeline.probe_picture_set_distortion(ims, _config(), [4, bad])
    with pytest.raises(ValueError, match="colour"):
        pipeline.probe_picture_set_distortion(ims, _config(), [4], colour="bgr")
