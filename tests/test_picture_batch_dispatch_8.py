"""What pipeline.compress_pictures / decompress_pictures_u8 decide at dct_size 8: the loop at the shipped gate
(DCT8_PICTURE_BATCH_MIN_PICTURES = None), and with the gate set libjpegx's dct_size-8 picture batch with exactly the
arguments of _job_config_8 / _decode_job_8.  Every entry they can reach is a recording fake, as in
tests/test_picture_batch_dispatch.py, so no device is needed and nothing of libjpegx runs but jpegx.padded_shape (host
arithmetic).  CPU only."""
import numpy as np
import pytest
from PIL import Image

import file_format
import jpegx
import pipeline
from pipeline.base import AlgorithmStep, step_classes

QTABLE = pipeline.QuantizationMethod("qtable")


def config(bs=4, quant=None, height=40, width=56, n=8, **kw):
    return pipeline.Configuration(width=width, height=height, block_size=bs, dct_size=n, quantization=quant or QTABLE, **kw)


def container(cfg, bands=(b"y", b"cb", b"cr")):
    return file_format.generate_data(cfg, pipeline.CompressedData(*bands))


class Fakes:
    """The dct_size-8 gate as given (None: as shipped) and no plane limit unless a test sets one; the DCTN_* gates open, so
    that only the DCT8_* ones can keep dct_size 8 from the batch.  The loop's four methods and the four batch conveniences
    record their calls."""

    def __init__(self, monkeypatch, gate=2, usable=True, fail=None):
        self.log, self.fail, self.seen = [], fail, []
        monkeypatch.setattr(pipeline, "_device_usable", lambda: usable)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_MIN_PICTURES", 2)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES", None)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES", None)
        if gate is not None:
            monkeypatch.setattr(pipeline, "DCT8_PICTURE_BATCH_MIN_PICTURES", gate)
            monkeypatch.setattr(pipeline, "DCT8_PICTURE_BATCH_COMPRESS_MAX_SAMPLES", None)
            monkeypatch.setattr(pipeline, "DCT8_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES", None)
        log = self.log
        monkeypatch.setattr(pipeline.Jpeg, "compress", lambda self, im: log.append(("compress", im.mode)) or b"loop")
        monkeypatch.setattr(pipeline.Jpeg, "compress_rgb", lambda self, im: log.append(("compress_rgb", im.mode)) or b"loop-rgb")
        monkeypatch.setattr(pipeline.Jpeg, "decompress", staticmethod(lambda c: log.append(("decompress",)) or Image.new("YCbCr", (3, 2))))
        monkeypatch.setattr(pipeline.Jpeg, "decompress_rgb", staticmethod(lambda c: log.append(("decompress_rgb",)) or Image.new("RGB", (3, 2))))
        made = lambda px, *a, **k: [[b"Y%d" % p, b"cb", b"cr" * p] for p in range(len(px))]                  # noqa: E731
        back = lambda blobs, rows, cols, *a, **k: np.ones((len(blobs), rows, cols, 3), np.uint8)            # noqa: E731
        monkeypatch.setattr(jpegx, "batch_compress_pictures", self._batch("batch_compress_pictures", made))
        monkeypatch.setattr(jpegx, "batch_decompress_pictures", self._batch("batch_decompress_pictures", back))
        monkeypatch.setattr(jpegx, "batch_compress_pictures_n", self._batch("batch_compress_pictures_n", made))
        monkeypatch.setattr(jpegx, "batch_decompress_pictures_n", self._batch("batch_decompress_pictures_n", back))

    def _batch(self, name, result):
        def call(first, *args, **kwargs):
            self.seen.append(first)
            self.log.append((name, len(first)) + args + tuple(sorted(kwargs.items())))
            if self.fail:
                raise jpegx.JpegxError(self.fail)
            return result(first, *args, **kwargs)
        return call

    def names(self):
        return [e[0] for e in self.log]


def pictures(k=4, rows=40, cols=56, mode="RGB"):
    rng = np.random.default_rng(k)
    return [Image.fromarray(rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8), mode=mode) for _ in range(k)]


def test_the_gate_ships_closed():
    assert pipeline.DCT8_PICTURE_BATCH_MIN_PICTURES is None


def test_at_the_shipped_gate_dct_size_8_is_the_loop(monkeypatch):
    f = Fakes(monkeypatch, gate=None)
    cfg = config()
    assert pipeline.compress_pictures(pictures(4), cfg, colour="rgb") == [b"loop-rgb"] * 4
    assert pipeline.compress_pictures(np.zeros((3, 40, 56, 3), np.uint8), cfg) == [b"loop"] * 3
    assert len(pipeline.decompress_pictures_u8([container(cfg)] * 4)) == 4
    assert len(pipeline.decompress_pictures_u8([container(cfg)] * 2, colour="rgb")) == 2
    assert f.log == [("compress_rgb", "RGB")] * 4 + [("compress", "YCbCr")] * 3 + [("decompress",)] * 4 + [("decompress_rgb",)] * 2
    # ... while every other dct_size goes by its own gates, as before
    f.log.clear()
    other = config(1, pipeline.QuantizationMethod("none"), n=4)
    pipeline.compress_pictures(pictures(2), other)
    pipeline.decompress_pictures_u8([container(other)] * 2)
    assert f.names() == ["batch_compress_pictures_n", "batch_decompress_pictures_n"]


def test_admitted_with_the_arguments_of_job_config_8(monkeypatch):
    f = Fakes(monkeypatch)
    cfg = config()
    ims = pictures(4)
    got = pipeline.compress_pictures(ims, cfg, colour="rgb")
    assert pipeline._job_config_8(cfg) == (4, "qtable", 0.0)
    assert f.log == [("batch_compress_pictures", 4, 4, "qtable", 0.0, ("colour", "rgb"))]
    assert f.seen[0].dtype == np.uint8 and np.array_equal(f.seen[0], np.stack([np.asarray(im) for im in ims]))
    assert got == [container(cfg, (b"Y%d" % p, b"cb", b"cr" * p)) for p in range(4)]
    assert got[2] == file_format.create_header(cfg) + b"\x02\x00\x00\x00Y2" + b"\x02\x00\x00\x00cb" + b"\x04\x00\x00\x00crcr"
    f.log.clear()
    # without colour the pictures go as they are, whatever their three-band mode; no colour keyword is handed on
    pipeline.compress_pictures(iter(pictures(3, 300, 400, "YCbCr")), config(3, pipeline.QuantizationMethod("divide", divisor=7), 300, 400))
    pipeline.compress_pictures(pictures(2) + pictures(1, mode="HSV"), config(1, pipeline.QuantizationMethod("discard", keep=2)))
    pipeline.compress_pictures(np.zeros((2, 40, 56, 3), np.uint8), config(255, pipeline.QuantizationMethod("none")))
    assert f.log == [("batch_compress_pictures", 3, 3, "divide", 7.0), ("batch_compress_pictures", 3, 1, "discard", 2.0),
                     ("batch_compress_pictures", 2, 255, "none", 0.0)]
    assert "batch_compress_pictures_n" not in f.names()


def test_decompress_admitted_with_the_arguments_of_decode_job_8(monkeypatch):
    f = Fakes(monkeypatch)
    cfg = config(3, pipeline.QuantizationMethod("divide", divisor=7), 150, 210)
    boxes = [container(cfg, (b"a%d" % p, bytearray(b"bb"), b"ccc")) for p in range(4)]
    back = pipeline.decompress_pictures_u8(boxes, colour="rgb")
    assert pipeline._decode_job_8(cfg)[2:] == (3, "divide", 7.0)
    assert f.log == [("batch_decompress_pictures", 4, 150, 210, 3, "divide", 7.0, ("colour", "rgb"))]
    assert f.seen[0] == [[b"a%d" % p, b"bb", b"ccc"] for p in range(4)]
    assert isinstance(back, list) and len(back) == 4 and all(b.shape == (150, 210, 3) and b.dtype == np.uint8 and b.all() for b in back)
    f.log.clear()
    ims = pipeline.decompress_pictures([bytearray(b) for b in boxes])
    assert f.log == [("batch_decompress_pictures", 4, 150, 210, 3, "divide", 7.0)]
    assert [im.mode for im in ims] == ["YCbCr"] * 4 and ims[0].size == (210, 150)
    assert [im.mode for im in pipeline.decompress_pictures(boxes, colour="rgb")] == ["RGB"] * 4


LOOPS = {
    "one picture": lambda: (pictures(1), config(), "rgb"),
    "mixed sizes": lambda: (pictures(3) + pictures(1, 40, 57), config(), "rgb"),
    "a picture that is not RGB with colour rgb": lambda: (pictures(3) + pictures(1, mode="YCbCr"), config(), "rgb"),
    "a grey picture": lambda: (pictures(3) + [Image.new("L", (56, 40))], config(), None),
    "block_size 256": lambda: (pictures(4), config(bs=256), "rgb"),
    "block_size 0": lambda: (pictures(4), config(bs=0), None),
    "transform DFT": lambda: (pictures(4), config(transform="DFT"), None),
    "an edited luminance table": lambda: (pictures(4), config(quant=_edited_table()), None),
}


def _edited_table():
    q = pipeline.QuantizationMethod("qtable")
    q.quantizer.table = (np.asarray(q.quantizer.table) + 1).tolist()
    return q


@pytest.mark.parametrize("what", sorted(LOOPS))
def test_everything_else_is_the_loop(monkeypatch, what):
    f = Fakes(monkeypatch)
    ims, cfg, colour = LOOPS[what]()
    got = pipeline.compress_pictures(ims, cfg, colour=colour)
    assert got == [b"loop-rgb" if colour else b"loop"] * len(ims)
    assert f.log == [("compress_rgb" if colour else "compress", im.mode) for im in ims]


@pytest.mark.parametrize("what", ["a container with another header", "an empty band", "a truncated container", "one container",
                                  "a divisor the fused inverse refuses", "an array among the containers"])
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
    elif what == "one container":
        boxes = boxes[:1]
    elif what == "a divisor the fused inverse refuses":
        boxes = [container(config(quant=pipeline.QuantizationMethod("divide", divisor=1000)))] * 4
    else:
        boxes = boxes[:3] + [np.zeros(40, np.uint8)]
    back = pipeline.decompress_pictures_u8(boxes)
    assert f.log == [("decompress",)] * len(boxes) and len(back) == len(boxes)


def test_no_device_a_non_stock_registry_and_the_count_gate(monkeypatch):
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
    # the gate is read when the functions are called; never below 2; the DCTN_* gate has no say at dct_size 8
    for gate, count, batch in [(6, 5, False), (5, 5, True), (0, 2, True), (0, 1, False), (4, 3, False), (4, 4, True)]:
        f = Fakes(monkeypatch, gate=gate)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_MIN_PICTURES", None)
        pipeline.compress_pictures(pictures(count), cfg)
        pipeline.decompress_pictures_u8([container(cfg)] * count)
        assert f.names() == (["batch_compress_pictures", "batch_decompress_pictures"] if batch else ["compress"] * count + ["decompress"] * count), gate


def test_the_plane_size_gates(monkeypatch):
    """Planes of more samples than DCT8_PICTURE_BATCH_COMPRESS_MAX_SAMPLES / _DECOMPRESS_MAX_SAMPLES are the loop, each
    direction by its own constant, read at call time.  The sizes are jpegx.padded_shape's, after pooling and both paddings:
    at block_size 2, 240 x 240 is 120 x 120 = 14 400 samples, one row more pads to 128 x 120."""
    assert jpegx.padded_shape(240, 240, 2) == (120, 120) and jpegx.padded_shape(241, 240, 2) == (128, 120)
    for rows, batch in ((240, True), (241, False)):
        cfg = config(2, height=rows, width=240)
        f = Fakes(monkeypatch)
        monkeypatch.setattr(pipeline, "DCT8_PICTURE_BATCH_COMPRESS_MAX_SAMPLES", 14400)
        pipeline.compress_pictures(pictures(2, rows, 240), cfg)
        pipeline.decompress_pictures_u8([container(cfg)] * 2)
        assert f.names() == (["batch_compress_pictures"] if batch else ["compress"] * 2) + ["batch_decompress_pictures"]
        f = Fakes(monkeypatch)
        monkeypatch.setattr(pipeline, "DCT8_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES", 14400)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES", 1)      # not dct_size 8's constant
        pipeline.compress_pictures(pictures(2, rows, 240), cfg)
        pipeline.decompress_pictures_u8([container(cfg)] * 2)
        assert f.names() == ["batch_compress_pictures"] + (["batch_decompress_pictures"] if batch else ["decompress"] * 2)


@pytest.mark.parametrize("text", ["fake failed (-1): BadRleCodeError (0, 16, 40000)", "fake failed (-4): forward_u8: a divisor below 0.5",
                                  "fake failed (-2): hipErrorUnknown"])
def test_a_refusal_of_the_batch_is_the_loop(monkeypatch, text):
    f = Fakes(monkeypatch, fail=text)
    cfg = config()
    assert pipeline.compress_pictures(pictures(3), cfg, colour="rgb") == [b"loop-rgb"] * 3
    assert f.names() == ["batch_compress_pictures"] + ["compress_rgb"] * 3
    f.log.clear()
    back = pipeline.decompress_pictures_u8([container(cfg)] * 3)
    assert f.names() == ["batch_decompress_pictures"] + ["decompress"] * 3 and len(back) == 3
