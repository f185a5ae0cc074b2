"""What pipeline.compress_picture_set / decompress_picture_set_u8 decide: which pictures they send to libjpegx's picture set
and with which arguments, and which go through the loop over Jpeg.compress / compress_rgb / decompress / decompress_rgb
instead.  Every entry they can reach is a recording fake, as in tests/test_picture_batch_dispatch.py, so no device is needed
and nothing of libjpegx runs.  CPU only."""
import numpy as np
import pytest
from PIL import Image

import file_format
import jpegx
import pipeline
from pipeline.base import AlgorithmStep, step_classes


def config(n=4, bs=1, quant=None, height=1, width=1, **kw):
    return pipeline.Configuration(width=width, height=height, block_size=bs, dct_size=n,
                                  quantization=quant or pipeline.QuantizationMethod("none"), **kw)


def sized(cfg, rows, cols):
    return pipeline.Configuration(width=cols, height=rows, block_size=cfg.block_size, dct_size=cfg.dct_size, transform=cfg.transform,
                                  quantization=cfg.quantization)


def container(cfg, bands=(b"y", b"cb", b"cr")):
    return file_format.generate_data(cfg, pipeline.CompressedData(*bands))


class Fakes:
    """The set's gates at 2 pictures and no plane limit unless a test sets them; the loop's four methods, the two set
    conveniences and the equal-size batch record their calls."""

    def __init__(self, monkeypatch, usable=True, fail=None):
        self.log, self.fail, self.seen = [], fail, []
        monkeypatch.setattr(pipeline, "_device_usable", lambda: usable)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_SET_MIN_PICTURES", 2)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_SET_COMPRESS_MAX_SAMPLES", None)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_SET_DECOMPRESS_MAX_SAMPLES", None)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_MIN_PICTURES", 2)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES", None)
        log = self.log
        monkeypatch.setattr(pipeline.Jpeg, "compress", lambda self, im: log.append(("compress", im.mode, self.config.height, self.config.width))
                            or b"loop%dx%d" % (im.height, im.width))
        monkeypatch.setattr(pipeline.Jpeg, "compress_rgb", lambda self, im: log.append(("compress_rgb", im.mode, self.config.height, self.config.width))
                            or b"loop-rgb%dx%d" % (im.height, im.width))
        monkeypatch.setattr(pipeline.Jpeg, "decompress", staticmethod(lambda c: log.append(("decompress",)) or Image.new("YCbCr", (3, 2))))
        monkeypatch.setattr(pipeline.Jpeg, "decompress_rgb", staticmethod(lambda c: log.append(("decompress_rgb",)) or Image.new("RGB", (3, 2))))
        monkeypatch.setattr(jpegx, "batch_compress_picture_set_n", self._batch(
            "batch_compress_picture_set_n", lambda px, *a, **k: [[b"Y%d" % p, b"", b"cr" * p] for p in range(len(px))]))
        monkeypatch.setattr(jpegx, "batch_decompress_picture_set_n", self._batch(
            "batch_decompress_picture_set_n", lambda blobs, sizes, *a, **k: [np.full((r, c, 3), 1 + p, np.uint8) for p, (r, c) in enumerate(sizes)]))
        monkeypatch.setattr(jpegx, "batch_compress_pictures_n", self._batch("batch_compress_pictures_n", lambda px, *a, **k: [[b"e"] * 3] * len(px)))

    def _batch(self, name, result):
        def call(first, *args, **kwargs):
            self.seen.append(first)
            self.log.append((name, len(first)) + args + tuple(sorted(kwargs.items())))
            if self.fail:
                raise jpegx.JpegxError(self.fail)
            return result(first, *args, **kwargs)
        return call


SIZES = [(40, 56), (33, 70), (40, 57), (120, 32), (40, 56)]


def pictures(sizes=SIZES, mode="RGB", seed=0):
    rng = np.random.default_rng(seed)
    return [Image.fromarray(rng.integers(0, 256, (r, c, 3), dtype=np.uint8), mode=mode) for r, c in sizes]


# ---- compress_picture_set ---------------------------------------------------------------------------------------------------
def test_mixed_sizes_go_once_with_each_pictures_pixels_and_own_header(monkeypatch):
    f = Fakes(monkeypatch)
    cfg = config()                                        # its own width and height (1 x 1) are not read
    ims = pictures()
    got = pipeline.compress_picture_set(ims, cfg, colour="rgb")
    assert f.log == [("batch_compress_picture_set_n", 5, 1, 4, "none", 0.0, ("colour", "rgb"))]
    assert len(f.seen[0]) == 5 and all(a.dtype == np.uint8 and np.array_equal(a, np.asarray(im)) for a, im in zip(f.seen[0], ims))
    assert got == [container(sized(cfg, r, c), (b"Y%d" % p, b"", b"cr" * p)) for p, (r, c) in enumerate(SIZES)]
    assert got[2] == file_format.create_header(sized(cfg, 40, 57)) + b"\x02\x00\x00\x00Y2" + b"\x00\x00\x00\x00" + b"\x04\x00\x00\x00crcr"
    assert len({g[:6] for g in got}) == 4                # four different sizes, four different headers
    f.log.clear()
    # without colour the pictures go as they are, whatever their three-band mode; no colour keyword is handed on
    q = pipeline.QuantizationMethod("divide", divisor=1000)
    pipeline.compress_picture_set(iter(pictures([(300, 400), (200, 410), (333, 217)], "YCbCr")), config(24, 5, q))
    pipeline.compress_picture_set(pictures(SIZES[:2], "RGB") + pictures(SIZES[2:3], "HSV"), config(16, 1, pipeline.QuantizationMethod("discard", keep=2)))
    assert f.log == [("batch_compress_picture_set_n", 3, 5, 24, "divide", 1000.0), ("batch_compress_picture_set_n", 3, 1, 16, "discard", 2.0)]


def test_pictures_the_jobs_do_not_admit_go_through_the_loop_and_come_back_in_place(monkeypatch):
    f = Fakes(monkeypatch)
    cfg = config()
    ims = pictures()
    ims.insert(1, Image.new("L", (56, 40)))              # a grey picture
    ims.insert(3, pictures([(8, 8)])[0])                  # a plane below DCTN_MIN_SAMPLES
    ims.insert(5, pictures([(40, 56)], "YCbCr")[0])      # not RGB under colour='rgb'
    got = pipeline.compress_picture_set(ims, cfg, colour="rgb")
    assert f.log[0] == ("batch_compress_picture_set_n", 5, 1, 4, "none", 0.0, ("colour", "rgb"))
    admitted = [0, 2, 4, 6, 7]
    assert all(np.array_equal(a, np.asarray(ims[at])) for a, at in zip(f.seen[0], admitted))
    # the loop takes the other three, each under a configuration of its own size, in input order
    assert f.log[1:] == [("compress_rgb", "L", 40, 56), ("compress_rgb", "RGB", 8, 8), ("compress_rgb", "YCbCr", 40, 56)]
    assert [got[at] for at in (1, 3, 5)] == [b"loop-rgb40x56", b"loop-rgb8x8", b"loop-rgb40x56"]
    for k, at in enumerate(admitted):
        im = ims[at]
        assert got[at] == container(sized(cfg, im.height, im.width), (b"Y%d" % k, b"", b"cr" * k))
    # without colour the YCbCr picture is admitted
    f.log.clear()
    pipeline.compress_picture_set(ims, cfg)
    assert f.log[0][:2] == ("batch_compress_picture_set_n", 6) and [e[0] for e in f.log[1:]] == ["compress"] * 2


LOOPS = {
    "one admitted picture": lambda: (pictures(SIZES[:1]) + pictures([(8, 8)]), config(), "rgb"),
    "dct_size 8": lambda: (pictures(), config(8, 1, pipeline.QuantizationMethod("qtable")), "rgb"),
    "dct_size 8, divide": lambda: (pictures(), config(8, 2, pipeline.QuantizationMethod("divide", divisor=7)), None),
    "planes below DCTN_MIN_SAMPLES": lambda: (pictures([(8, 8), (9, 7), (31, 31)]), config(), "rgb"),
    "block_size 256": lambda: (pictures(), config(bs=256), "rgb"),
    "block_size 2.0": lambda: (pictures(), config(bs=2.0), "rgb"),
    "dct_size 33": lambda: (pictures(), config(n=33), None),
    "transform DFT": lambda: (pictures(), config(transform="DFT"), None),
    "a divisor that reaches 2^31": lambda: (pictures(), config(quant=pipeline.QuantizationMethod("divide", divisor=1e-9)), "rgb"),
    "grey pictures": lambda: ([Image.new("L", (56, 40)), Image.new("L", (50, 44))], config(), None),
}


@pytest.mark.parametrize("what", sorted(LOOPS))
def test_everything_else_is_the_loop(monkeypatch, what):
    f = Fakes(monkeypatch)
    ims, cfg, colour = LOOPS[what]()
    got = pipeline.compress_picture_set(ims, cfg, colour=colour)
    assert got == [(b"loop-rgb%dx%d" if colour else b"loop%dx%d") % (im.height, im.width) for im in ims]
    assert f.log == [("compress_rgb" if colour else "compress", im.mode, im.height, im.width) for im in ims]


def test_no_gpu_a_non_stock_registry_and_the_gates(monkeypatch):
    cfg = config()
    boxes = [container(sized(cfg, r, c)) for r, c in SIZES]
    f = Fakes(monkeypatch, usable=False)
    pipeline.compress_picture_set(pictures(), cfg, colour="rgb")
    pipeline.decompress_picture_set_u8(boxes)
    assert [e[0] for e in f.log] == ["compress_rgb"] * 5 + ["decompress"] * 5
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
        pipeline.compress_picture_set(pictures(), cfg)
        pipeline.decompress_picture_set_u8(boxes, colour="rgb")
    finally:
        step_classes[:] = stock
    assert [e[0] for e in f.log] == ["compress"] * 5 + ["decompress_rgb"] * 5
    # the gate counts ADMITTED pictures, is read when the functions are called, and is never below 2; None is the loop
    for gate, count, batch in [(None, 5, False), (6, 5, False), (5, 5, True), (0, 2, True), (0, 1, False), (4, 3, False), (4, 4, True)]:
        f = Fakes(monkeypatch)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_SET_MIN_PICTURES", gate)
        pipeline.compress_picture_set(pictures(SIZES[:count]) + [Image.new("L", (9, 9))], cfg)
        pipeline.decompress_picture_set_u8(boxes[:count] + [b"junk"])
        names = [e[0] for e in f.log]
        want = ["batch_compress_picture_set_n", "compress", "batch_decompress_picture_set_n", "decompress"] if batch else \
            ["compress"] * (count + 1) + ["decompress"] * (count + 1)
        assert names == want, gate
    assert pipeline.compress_picture_set([], cfg) == [] and pipeline.decompress_picture_set_u8([]) == []
    with pytest.raises(ValueError):
        pipeline.compress_picture_set(pictures(), cfg, colour="bgr")
    with pytest.raises(ValueError):
        pipeline.decompress_picture_set_u8(boxes, colour="bgr")


def test_the_plane_size_gates_look_at_the_largest_plane(monkeypatch):
    """118 x 120 pads to 120 x 120 = 14400 samples at N 4, one row more to 124 x 120; the other pictures are small."""
    for rows, batch in ((118, True), (121, False)):
        sizes = [(40, 56), (rows, 120), (33, 70)]
        cfg = config()
        boxes = [container(sized(cfg, r, c)) for r, c in sizes]
        f = Fakes(monkeypatch)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_SET_COMPRESS_MAX_SAMPLES", 14400)
        pipeline.compress_picture_set(pictures(sizes), cfg)
        pipeline.decompress_picture_set_u8(boxes)
        assert [e[0] for e in f.log] == (["batch_compress_picture_set_n"] if batch else ["compress"] * 3) + ["batch_decompress_picture_set_n"]
        f = Fakes(monkeypatch)
        monkeypatch.setattr(pipeline, "DCTN_PICTURE_SET_DECOMPRESS_MAX_SAMPLES", 14400)
        pipeline.compress_picture_set(pictures(sizes), cfg)
        pipeline.decompress_picture_set_u8(boxes)
        assert [e[0] for e in f.log] == ["batch_compress_picture_set_n"] + (["batch_decompress_picture_set_n"] if batch else ["decompress"] * 3)


@pytest.mark.parametrize("text", ["fake failed (-1): BadRleCodeError (0, 16, 40000)", "fake failed (-2): hipErrorUnknown"])
def test_a_refusal_of_the_set_is_the_loop(monkeypatch, text):
    f = Fakes(monkeypatch, fail=text)
    cfg = config()
    assert pipeline.compress_picture_set(pictures(SIZES[:3]), cfg, colour="rgb") == [b"loop-rgb%dx%d" % s for s in SIZES[:3]]
    assert [e[0] for e in f.log] == ["batch_compress_picture_set_n"] + ["compress_rgb"] * 3
    f.log.clear()
    back = pipeline.decompress_picture_set_u8([container(sized(cfg, r, c)) for r, c in SIZES[:3]])
    assert [e[0] for e in f.log] == ["batch_decompress_picture_set_n"] + ["decompress"] * 3 and len(back) == 3


def test_compress_pictures_with_mixed_sizes_is_still_the_loop(monkeypatch):
    f = Fakes(monkeypatch)
    cfg = config(height=40, width=56)
    got = pipeline.compress_pictures(pictures([(40, 56)] * 3 + [(40, 57)]), cfg, colour="rgb")
    assert [e[0] for e in f.log] == ["compress_rgb"] * 4 and len(got) == 4
    f.log.clear()
    pipeline.compress_pictures(pictures([(40, 56)] * 3), cfg, colour="rgb")
    assert [e[0] for e in f.log] == ["batch_compress_pictures_n"]


# ---- decompress_picture_set_u8 / decompress_picture_set -----------------------------------------------------------------------
def test_decompress_admitted(monkeypatch):
    f = Fakes(monkeypatch)
    cfg = config(4, 3)
    sizes = [(150, 210), (99, 211), (150, 210), (301, 96)]
    boxes = [container(sized(cfg, r, c), (b"a%d" % p, bytearray(b"bb"), b"ccc")) for p, (r, c) in enumerate(sizes)]
    back = pipeline.decompress_picture_set_u8(boxes, colour="rgb")
    assert f.log == [("batch_decompress_picture_set_n", 4, sizes, 3, 4, "none", 0.0, ("colour", "rgb"))]
    assert f.seen[0] == [[b"a%d" % p, b"bb", b"ccc"] for p in range(4)]
    assert isinstance(back, list) and [b.shape for b in back] == [(r, c, 3) for r, c in sizes]
    assert all(b.dtype == np.uint8 and np.all(b == 1 + p) for p, b in enumerate(back))
    f.log.clear()
    ims = pipeline.decompress_picture_set([bytearray(b) for b in boxes])
    assert f.log == [("batch_decompress_picture_set_n", 4, sizes, 3, 4, "none", 0.0)]
    assert [im.mode for im in ims] == ["YCbCr"] * 4 and [im.size for im in ims] == [(c, r) for r, c in sizes]
    assert [im.mode for im in pipeline.decompress_picture_set(boxes, colour="rgb")] == ["RGB"] * 4


def test_decompress_sends_what_it_can_and_loops_over_the_rest_in_place(monkeypatch):
    f = Fakes(monkeypatch)
    cfg = config()
    sizes = [(40, 56), (33, 70), (120, 32)]
    boxes = [container(sized(cfg, r, c)) for r, c in sizes]
    odd = [container(sized(config(bs=2), 40, 56)),        # another block_size: another header
           container(sized(cfg, 40, 56), (b"y", b"", b"cr")),      # an empty band
           boxes[0][:-1],                                  # truncated
           container(sized(cfg, 8, 8)),                    # a plane below DCTN_MIN_SAMPLES
           np.zeros(40, np.uint8)]                         # no bytes at all
    mixed = [boxes[0], odd[0], boxes[1], odd[1], odd[2], boxes[2], odd[3], odd[4]]
    back = pipeline.decompress_picture_set_u8(mixed)
    assert f.log[0] == ("batch_decompress_picture_set_n", 3, sizes, 1, 4, "none", 0.0)
    assert f.log[1:] == [("decompress",)] * 5
    assert [b.shape for b in back] == [(40, 56, 3), (2, 3, 3), (33, 70, 3), (2, 3, 3), (2, 3, 3), (120, 32, 3), (2, 3, 3), (2, 3, 3)]
    assert [int(back[at][0, 0, 0]) for at in (0, 2, 5)] == [1, 2, 3]


@pytest.mark.parametrize("what", ["one admitted container", "dct_size 8", "a divisor that is no integer", "planes below DCTN_MIN_SAMPLES"])
def test_decompress_loops(monkeypatch, what):
    f = Fakes(monkeypatch)
    cfg = config()
    if what == "one admitted container":
        boxes = [container(sized(cfg, 40, 56)), container(sized(cfg, 8, 8))]
    elif what == "dct_size 8":
        boxes = [container(sized(config(8, 1, pipeline.QuantizationMethod("qtable")), r, c)) for r, c in SIZES]
    elif what == "a divisor that is no integer":
        boxes = [container(sized(config(quant=pipeline.QuantizationMethod("divide", divisor=2.5)), r, c)) for r, c in SIZES]
    else:
        boxes = [container(sized(cfg, 8, 8)), container(sized(cfg, 9, 7))]
    back = pipeline.decompress_picture_set_u8(boxes)
    assert f.log == [("decompress",)] * len(boxes) and len(back) == len(boxes)
