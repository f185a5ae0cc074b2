"""What pipeline.compress_pictures / decompress_pictures_u8 decide: when they call libjpegx's picture batch and with which
arguments, and when they are the loop over Jpeg.compress / compress_rgb / decompress / decompress_rgb instead.  Every entry
they can reach is a recording fake, as in tests/test_batch_dispatch_n.py, so no device is needed and nothing of libjpegx
runs.  CPU only."""
import numpy as np
import pytest
from PIL import Image

import file_format
import jpegx
import pipeline
from pipeline.base import AlgorithmStep, step_classes


def config(n=4, bs=1, quant=None, height=40, width=56, **kw):
    return pipeline.Configuration(width=width, height=height, block_size=bs, dct_size=n,
                                  quantization=quant or pipeline.QuantizationMethod("none"), **kw)


def container(cfg, bands=(b"y", b"cb", b"cr")):
    return file_format.generate_data(cfg, pipeline.CompressedData(*bands))


class Fakes:
    """The gates at 2 pictures and no plane limit unless a test sets them; the loop's four methods and the two batch
    conveniences record their calls."""

    def __init__(self, monkeypatch, usable=True, fail=None):
        self.log, self.fail, self.seen = [], fail, []
        monkeypatch.setattr(pipeline, "_device_usable", lambda: usable)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_MIN_PICTURES", 2)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES", None)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES", None)
        log = self.log
        monkeypatch.setattr(pipeline.Jpeg, "compress", lambda self, im: log.append(("compress", im.mode)) or b"loop")
        monkeypatch.setattr(pipeline.Jpeg, "compress_rgb", lambda self, im: log.append(("compress_rgb", im.mode)) or b"loop-rgb")
        monkeypatch.setattr(pipeline.Jpeg, "decompress", staticmethod(lambda c: log.append(("decompress",)) or Image.new("YCbCr", (3, 2))))
        monkeypatch.setattr(pipeline.Jpeg, "decompress_rgb", staticmethod(lambda c: log.append(("decompress_rgb",)) or Image.new("RGB", (3, 2))))
        monkeypatch.setattr(jpegx, "batch_compress_pictures_n", self._batch(
            "batch_compress_pictures_n", lambda px, *a, **k: [[b"Y%d" % p, b"", b"cr" * p] for p in range(len(px))]))
        monkeypatch.setattr(jpegx, "batch_decompress_pictures_n", self._batch(
            "batch_decompress_pictures_n", lambda blobs, rows, cols, *a, **k: np.ones((len(blobs), rows, cols, 3), np.uint8)))

    def _batch(self, name, result):
        def call(first, *args, **kwargs):
            self.seen.append(first)
            self.log.append((name, len(first)) + args + tuple(sorted(kwargs.items())))
            if self.fail:
                raise jpegx.JpegxError(self.fail)
            return result(first, *args, **kwargs)
        return call


def pictures(k=4, rows=40, cols=56, mode="RGB"):
    rng = np.random.default_rng(k)
    return [Image.fromarray(rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8), mode=mode) for _ in range(k)]


# ---- compress_pictures --------------------------------------------------------------------------------------------------------
def test_admitted_and_the_containers_are_generate_data_s(monkeypatch):
    f = Fakes(monkeypatch)
    cfg = config()
    ims = pictures(4)
    got = pipeline.compress_pictures(ims, cfg, colour="rgb")
    assert f.log == [("batch_compress_pictures_n", 4, 1, 4, "none", 0.0, ("colour", "rgb"))]
    assert f.seen[0].dtype == np.uint8 and np.array_equal(f.seen[0], np.stack([np.asarray(im) for im in ims]))
    assert got == [container(cfg, (b"Y%d" % p, b"", b"cr" * p)) for p in range(4)]
    assert got[2] == file_format.create_header(cfg) + b"\x02\x00\x00\x00Y2" + b"\x00\x00\x00\x00" + b"\x04\x00\x00\x00crcr"
    f.log.clear()
    # without colour the pictures go as they are, whatever their three-band mode; no colour keyword is handed on
    q = pipeline.QuantizationMethod("divide", divisor=1000)
    pipeline.compress_pictures(iter(pictures(3, 300, 400, "YCbCr")), config(24, 5, q, 300, 400))
    pipeline.compress_pictures(pictures(2, mode="RGB") + pictures(1, mode="HSV"), config(16, 1, pipeline.QuantizationMethod("discard", keep=2)))
    assert f.log == [("batch_compress_pictures_n", 3, 5, 24, "divide", 1000.0), ("batch_compress_pictures_n", 3, 1, 16, "discard", 2.0)]


def test_an_array_is_n_pictures(monkeypatch):
    f = Fakes(monkeypatch)
    px = np.random.default_rng(0).integers(0, 256, (3, 40, 56, 3), dtype=np.uint8)
    assert len(pipeline.compress_pictures(px, config())) == 3
    assert len(pipeline.compress_pictures(px[:, ::1], config(), colour="rgb")) == 3
    assert [e[0] for e in f.log] == ["batch_compress_pictures_n"] * 2 and f.seen[0] is not None and np.array_equal(f.seen[0], px)
    f.log.clear()
    # the loop takes its slices as pictures of mode YCbCr, or RGB with colour='rgb'
    monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_MIN_PICTURES", None)
    assert pipeline.compress_pictures(px, config()) == [b"loop"] * 3
    assert pipeline.compress_pictures(px, config(), colour="rgb") == [b"loop-rgb"] * 3
    assert f.log == [("compress", "YCbCr")] * 3 + [("compress_rgb", "RGB")] * 3
    f.log.clear()
    for bad in (px[:, :39], px[..., :2], px.astype(np.int32)):          # another size, two bands, no bytes: the loop
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_MIN_PICTURES", 2)
        try:
            pipeline.compress_pictures(bad, config())
        except Exception:
            pass
    assert "batch_compress_pictures_n" not in [e[0] for e in f.log]


LOOPS = {
    "one picture": lambda: (pictures(1), config(), "rgb"),
    "mixed sizes": lambda: (pictures(3) + pictures(1, 40, 57), config(), "rgb"),
    "a picture that is not RGB with colour rgb": lambda: (pictures(3) + pictures(1, mode="YCbCr"), config(), "rgb"),
    "a grey picture": lambda: (pictures(3) + [Image.new("L", (56, 40))], config(), None),
    "a four-band picture": lambda: (pictures(3) + [Image.new("CMYK", (56, 40))], config(), None),
    "dct_size 8": lambda: (pictures(4), config(8, 1, pipeline.QuantizationMethod("qtable")), "rgb"),
    "dct_size 8, divide": lambda: (pictures(4), config(8, 2, pipeline.QuantizationMethod("divide", divisor=7)), None),
    "planes below DCTN_MIN_SAMPLES": lambda: (pictures(4, 8, 8), config(height=8, width=8), "rgb"),
    "block_size 256": lambda: (pictures(4), config(bs=256), "rgb"),
    "block_size 2.0": lambda: (pictures(4), config(bs=2.0), "rgb"),
    "dct_size 33": lambda: (pictures(4), config(n=33), None),
    "transform DFT": lambda: (pictures(4), config(transform="DFT"), None),
    "a divisor that reaches 2^31": lambda: (pictures(4), config(quant=pipeline.QuantizationMethod("divide", divisor=1e-9)), "rgb"),
}


@pytest.mark.parametrize("what", sorted(LOOPS))
def test_everything_else_is_the_loop(monkeypatch, what):
    f = Fakes(monkeypatch)
    ims, cfg, colour = LOOPS[what]()
    got = pipeline.compress_pictures(ims, cfg, colour=colour)
    assert got == [b"loop-rgb" if colour else b"loop"] * len(ims)
    assert f.log == [("compress_rgb" if colour else "compress", im.mode) for im in ims]


def test_no_gpu_a_non_stock_registry_and_the_gates(monkeypatch):
    cfg = config()
    boxes = [container(cfg)] * 4
    f = Fakes(monkeypatch, usable=False)
    pipeline.compress_pictures(pictures(4), cfg, colour="rgb")
    pipeline.decompress_pictures_u8(boxes)
    assert f.log == [("compress_rgb", "RGB")] * 4 + [("decompress",)] * 4
    f = Fakes(monkeypatch)
    stock = list(step_classes)
    try:
        class PassThrough(AlgorithmStep):
            step_index = 9.5

            def execute(self, array):
                return array

            def invert(self, array):
                return array
        assert not pipeline._stock_registry()
        pipeline.compress_pictures(pictures(4), cfg)
        pipeline.decompress_pictures_u8(boxes, colour="rgb")
    finally:
        step_classes[:] = stock
    assert f.log == [("compress", "RGB")] * 4 + [("decompress_rgb",)] * 4
    # the gate is read when the functions are called; never below 2
    for gate, count, batch in [(None, 5, False), (6, 5, False), (5, 5, True), (0, 2, True), (0, 1, False), (4, 3, False), (4, 4, True)]:
        f = Fakes(monkeypatch)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_MIN_PICTURES", gate)
        pipeline.compress_pictures(pictures(count), cfg)
        pipeline.decompress_pictures_u8([container(cfg)] * count)
        names = [e[0] for e in f.log]
        assert names == (["batch_compress_pictures_n", "batch_decompress_pictures_n"] if batch else ["compress"] * count + ["decompress"] * count), gate
    assert pipeline.compress_pictures([], cfg) == [] and pipeline.decompress_pictures_u8([]) == []
    with pytest.raises(ValueError):
        pipeline.compress_pictures(pictures(2), cfg, colour="bgr")
    with pytest.raises(ValueError):
        pipeline.decompress_pictures_u8(boxes, colour="bgr")


def test_the_plane_size_gates(monkeypatch):
    """Planes of more samples than DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES / _DECOMPRESS_MAX_SAMPLES are the loop, each
    direction by its own constant, read at call time.  The sizes are those after both paddings: 118 x 120 pads to 120 x 120 at
    N 4, one row more to 124 x 120."""
    for rows, batch in ((118, True), (121, False)):
        f = Fakes(monkeypatch)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES", 14400)
        cfg = config(height=rows, width=120)
        pipeline.compress_pictures(pictures(2, rows, 120), cfg)
        pipeline.decompress_pictures_u8([container(cfg)] * 2)
        assert [e[0] for e in f.log] == (["batch_compress_pictures_n"] if batch else ["compress"] * 2) + ["batch_decompress_pictures_n"]
        f = Fakes(monkeypatch)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES", 14400)
        pipeline.compress_pictures(pictures(2, rows, 120), cfg)
        pipeline.decompress_pictures_u8([container(cfg)] * 2)
        assert [e[0] for e in f.log] == ["batch_compress_pictures_n"] + (["batch_decompress_pictures_n"] if batch else ["decompress"] * 2)


@pytest.mark.parametrize("text", ["fake failed (-1): BadRleCodeError (0, 16, 40000)", "fake failed (-2): hipErrorUnknown"])
def test_a_refusal_of_the_batch_is_the_loop(monkeypatch, text):
    f = Fakes(monkeypatch, fail=text)
    cfg = config()
    assert pipeline.compress_pictures(pictures(3), cfg, colour="rgb") == [b"loop-rgb"] * 3
    assert [e[0] for e in f.log] == ["batch_compress_pictures_n"] + ["compress_rgb"] * 3
    f.log.clear()
    back = pipeline.decompress_pictures_u8([container(cfg)] * 3)
    assert [e[0] for e in f.log] == ["batch_decompress_pictures_n"] + ["decompress"] * 3 and len(back) == 3


# ---- decompress_pictures_u8 / decompress_pictures -------------------------------------------------------------------------------
def test_decompress_admitted(monkeypatch):
    f = Fakes(monkeypatch)
    cfg = config(4, 3, None, 150, 210)
    boxes = [container(cfg, (b"a%d" % p, bytearray(b"bb"), b"ccc")) for p in range(4)]
    back = pipeline.decompress_pictures_u8(boxes, colour="rgb")
    assert f.log == [("batch_decompress_pictures_n", 4, 150, 210, 3, 4, "none", 0.0, ("colour", "rgb"))]
    assert f.seen[0] == [[b"a%d" % p, b"bb", b"ccc"] for p in range(4)]
    assert isinstance(back, list) and len(back) == 4 and all(b.shape == (150, 210, 3) and b.dtype == np.uint8 and b.all() for b in back)
    f.log.clear()
    ims = pipeline.decompress_pictures([bytearray(b) for b in boxes])
    assert f.log == [("batch_decompress_pictures_n", 4, 150, 210, 3, 4, "none", 0.0)]
    assert [im.mode for im in ims] == ["YCbCr"] * 4 and ims[0].size == (210, 150)
    assert [im.mode for im in pipeline.decompress_pictures(boxes, colour="rgb")] == ["RGB"] * 4


@pytest.mark.parametrize("what", ["a container with another header", "an empty band", "a truncated container", "a divisor that is no integer",
                                  "one container", "dct_size 8", "planes below DCTN_MIN_SAMPLES", "an array among the containers"])
def test_decompress_loops(monkeypatch, what):
    f = Fakes(monkeypatch)
    cfg = config()
    boxes = [container(cfg)] * 4
    if what == "a container with another header":
        boxes = boxes[:3] + [container(config(height=41))]
    elif what == "an empty band":
        boxes = boxes[:3] + [container(cfg, (b"y", b"", b"cr"))]
    elif what == "a truncated container":
        boxes = boxes[:3] + [boxes[0][:-1]]
    elif what == "a divisor that is no integer":
        boxes = [container(config(quant=pipeline.QuantizationMethod("divide", divisor=2.5)))] * 4
    elif what == "one container":
        boxes = boxes[:1]
    elif what == "dct_size 8":
        boxes = [container(config(8, 1, pipeline.QuantizationMethod("qtable")))] * 4
    elif what == "planes below DCTN_MIN_SAMPLES":
        boxes = [container(config(height=8, width=8))] * 4
    else:
        boxes = boxes[:3] + [np.zeros(40, np.uint8)]
    back = pipeline.decompress_pictures_u8(boxes)
    assert f.log == [("decompress",)] * len(boxes) and len(back) == len(boxes)
    assert all(b.shape == (2, 3, 3) and b.dtype == np.uint8 for b in back)
