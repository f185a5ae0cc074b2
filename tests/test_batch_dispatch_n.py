"""What pipeline.compress_bands / decompress_bands_u8 decide: which libjpegx batch entry they call and with which
arguments, and when they are the loop over compress_band / decompress_band_u8 instead.  Every entry they can reach is a
recording fake, as in tests/test_dispatch_record.py, so no device is needed and nothing of libjpegx runs.  CPU only."""
import numpy as np
import pytest

import jpegx
import pipeline
from pipeline.base import AlgorithmStep, step_classes


def config(n=4, bs=1, quant=None, height=40, width=40, **kw):
    return pipeline.Configuration(width=width, height=height, block_size=bs, dct_size=n,
                                  quantization=quant or pipeline.QuantizationMethod("none"), **kw)


class Fakes:
    def __init__(self, monkeypatch, usable=True, fail=None):
        self.log, self.fail = [], fail
        monkeypatch.setattr(pipeline, "_device_usable", lambda: usable)
        monkeypatch.setattr(pipeline, "compress_band", self._per_band("compress_band", lambda a, cfg: b"one"))
        monkeypatch.setattr(pipeline, "decompress_band_u8",
                            self._per_band("decompress_band_u8", lambda r, cfg: np.zeros((int(cfg.height), int(cfg.width)), np.uint8)))
        monkeypatch.setattr(jpegx, "batch_compress_n", self._batch("batch_compress_n", lambda bands, *a, **k: [b"n"] * len(bands)))
        monkeypatch.setattr(jpegx, "batch_compress", self._batch("batch_compress", lambda planes, *a, **k: [b"8"] * len(planes)))
        monkeypatch.setattr(jpegx, "batch_decompress_n",
                            self._batch("batch_decompress_n", lambda blobs, rows, cols, *a, **k: np.ones((len(blobs), rows, cols), np.uint8)))
        monkeypatch.setattr(jpegx, "batch_decompress",
                            self._batch("batch_decompress", lambda blobs, h, w, bs=1, *a, **k: np.ones((len(blobs), h * int(bs), w * int(bs)), np.uint8)))

    def _per_band(self, name, result):
        def call(a, cfg):
            self.log.append((name,))
            return result(a, cfg)
        return call

    def _batch(self, name, result):
        def call(first, *args, **kwargs):
            self.log.append((name, len(first)) + args + tuple(sorted(kwargs.items())))
            if self.fail:
                raise jpegx.JpegxError(self.fail)
            return result(first, *args, **kwargs)
        return call


def u8_bands(k=5, rows=40, cols=40, dtype=np.uint8):
    return [np.full((rows, cols), 10 + p, dtype) for p in range(k)]


# ---- compress_bands ---------------------------------------------------------------------------------------------------------
def test_admitted_at_dct_size_n(monkeypatch):
    f = Fakes(monkeypatch)
    assert pipeline.compress_bands(u8_bands(), config()) == [b"n"] * 5
    assert f.log == [("batch_compress_n", 5, 1, 4, "none", 0.0)]
    f.log.clear()
    q = pipeline.QuantizationMethod("divide", divisor=1000)
    assert pipeline.compress_bands(u8_bands(4, 300, 400, np.int64), config(24, 5, q, 300, 400)) == [b"n"] * 4
    assert f.log == [("batch_compress_n", 4, 5, 24, "divide", 1000.0)]
    f.log.clear()
    assert pipeline.compress_bands(iter(u8_bands(4)), config(16, 1, pipeline.QuantizationMethod("discard", keep=2))) == [b"n"] * 4
    assert f.log == [("batch_compress_n", 4, 1, 16, "discard", 2.0)]


def test_the_stack_handed_over_is_the_bands(monkeypatch):
    seen = []
    Fakes(monkeypatch)
    monkeypatch.setattr(jpegx, "batch_compress_n", lambda bands, *a: seen.append(bands) or [b"x"] * len(bands))
    bands = [np.random.default_rng(p).integers(0, 256, (40, 44)).astype(np.int32) for p in range(4)]
    pipeline.compress_bands(bands, config(width=44))
    assert seen[0].dtype == np.uint8 and np.array_equal(seen[0], np.stack(bands))


def test_admitted_at_dct_size_8(monkeypatch):
    f = Fakes(monkeypatch)
    q = pipeline.QuantizationMethod("qtable")
    assert pipeline.compress_bands(u8_bands(4, 32, 48), config(8, 2, q, 32, 48)) == [b"8"] * 4
    assert f.log == [("batch_compress", 4, 2, "qtable", 0.0)]
    f.log.clear()
    # the shape and block_size limits of jpegx.batch_compress: else the loop
    assert pipeline.compress_bands(u8_bands(4, 30, 48), config(8, 2, q, 30, 48)) == [b"one"] * 4
    assert pipeline.compress_bands(u8_bands(4, 48, 48), config(8, 3, q, 48, 48)) == [b"one"] * 4
    assert f.log == [("compress_band",)] * 8


LOOPS = {
    "one band": lambda: (u8_bands(1), config()),
    "unequal shapes": lambda: (u8_bands(4) + u8_bands(1, 40, 41), config()),
    "float bands": lambda: (u8_bands(5, dtype=np.float64), config()),
    "a sample of 300": lambda: (u8_bands(4, dtype=np.int64) + [np.full((40, 40), 300)], config()),
    "a negative sample": lambda: (u8_bands(4, dtype=np.int64) + [np.full((40, 40), -1)], config()),
    "3-D bands": lambda: ([np.zeros((4, 40, 40), np.uint8)] * 5, config()),
    "planes below DCTN_MIN_SAMPLES": lambda: (u8_bands(5, 8, 8), config(height=8, width=8)),
    "block_size 256": lambda: (u8_bands(), config(bs=256)),
    "block_size 2.0": lambda: (u8_bands(), config(bs=2.0)),
    "dct_size 33": lambda: (u8_bands(), config(n=33)),
    "transform DFT": lambda: (u8_bands(), config(transform="DFT")),
    "a subclassed quantiser": lambda: (u8_bands(), config(quant=subclassed())),
    "a divisor that reaches 2^31": lambda: (u8_bands(), config(quant=pipeline.QuantizationMethod("divide", divisor=1e-9))),
}


def subclassed():
    from quantizers import DivisionQuantizer

    class Mine(DivisionQuantizer):
        pass
    q = pipeline.QuantizationMethod("divide", divisor=10)
    q.quantizer = Mine(10)
    return q


@pytest.mark.parametrize("what", sorted(LOOPS))
def test_everything_else_is_the_loop(monkeypatch, what):
    f = Fakes(monkeypatch)
    bands, cfg = LOOPS[what]()
    assert pipeline.compress_bands(bands, cfg) == [b"one"] * len(bands)
    assert f.log == [("compress_band",)] * len(bands)


def test_no_gpu_a_non_stock_registry_and_the_gate(monkeypatch):
    f = Fakes(monkeypatch, usable=False)
    assert pipeline.compress_bands(u8_bands(), config()) == [b"one"] * 5
    assert pipeline.decompress_bands_u8([b"\x00"] * 5, config())[0].shape == (40, 40)
    assert f.log == [("compress_band",)] * 5 + [("decompress_band_u8",)] * 5
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
        pipeline.compress_bands(u8_bands(), config())
        pipeline.decompress_bands_u8([b"\x00"] * 5, config())
    finally:
        step_classes[:] = stock
    assert f.log == [("compress_band",)] * 5 + [("decompress_band_u8",)] * 5
    # the gate is read when the functions are called
    for gate, count, batch in [(None, 5, False), (6, 5, False), (5, 5, True), (0, 2, True), (0, 1, False), (4, 3, False), (4, 4, True)]:
        f = Fakes(monkeypatch)
        monkeypatch.setattr(pipeline, "DCTN_BATCH_MIN_PLANES", gate)
        pipeline.compress_bands(u8_bands(count), config())
        pipeline.decompress_bands_u8([b"\x00"] * count, config())
        names = [e[0] for e in f.log]
        assert names == (["batch_compress_n", "batch_decompress_n"] if batch else ["compress_band"] * count + ["decompress_band_u8"] * count), gate
    assert pipeline.compress_bands([], config()) == [] and pipeline.decompress_bands_u8([], config()) == []
    monkeypatch.undo()
    assert pipeline.DCTN_BATCH_MIN_PLANES == 4


def test_the_plane_size_gates(monkeypatch):
    """Planes of more samples than DCTN_BATCH_COMPRESS_MAX_SAMPLES / DCTN_BATCH_DECOMPRESS_MAX_SAMPLES are the loop, each
    direction by its own constant, read at call time; None lifts the limit.  The sizes are those after both paddings."""
    assert pipeline.DCTN_BATCH_COMPRESS_MAX_SAMPLES == 14400 and pipeline.DCTN_BATCH_DECOMPRESS_MAX_SAMPLES == 262144
    q8 = pipeline.QuantizationMethod("qtable")
    # 118 x 120 samples pad to 120 x 120 = 14 400 at N 4 and N 8; one row more to 124 x 120 / 128 x 120
    for n, quant in ((4, None), (8, q8)):
        for rows, batch in ((118 if n == 4 else 120, True), (121, False)):
            f = Fakes(monkeypatch)
            rows8 = rows if n == 4 else (120 if batch else 128)
            pipeline.compress_bands(u8_bands(4, rows8, 120), config(n, 1, quant, rows8, 120))
            assert [e[0] for e in f.log] == ([("batch_compress_n" if n == 4 else "batch_compress")] if batch else ["compress_band"] * 4), (n, rows8)
    for n, quant in ((4, None), (8, q8)):
        for rows, batch in ((512, True), (513, False)):
            f = Fakes(monkeypatch)
            pipeline.decompress_bands_u8([b"\x01"] * 4, config(n, 1, quant, rows, 512))
            assert [e[0] for e in f.log] == ([("batch_decompress_n" if n == 4 else "batch_decompress")] if batch else ["decompress_band_u8"] * 4), (n, rows)
    f = Fakes(monkeypatch)
    monkeypatch.setattr(pipeline, "DCTN_BATCH_COMPRESS_MAX_SAMPLES", None)
    monkeypatch.setattr(pipeline, "DCTN_BATCH_MIN_PLANES", 2)
    monkeypatch.setattr(pipeline, "DCTN_BATCH_DECOMPRESS_MAX_SAMPLES", 100)
    pipeline.compress_bands(u8_bands(2, 3000, 4000), config(4, 1, None, 3000, 4000))
    pipeline.decompress_bands_u8([b"\x01"] * 2, config())
    assert [e[0] for e in f.log] == ["batch_compress_n", "decompress_band_u8", "decompress_band_u8"]


@pytest.mark.parametrize("text", ["fake failed (-1): BadRleCodeError (0, 16, 40000)", "fake failed (-2): hipErrorUnknown"])
def test_a_refusal_of_the_batch_is_the_loop(monkeypatch, text):
    f = Fakes(monkeypatch, fail=text)
    assert pipeline.compress_bands(u8_bands(), config()) == [b"one"] * 5
    assert [e[0] for e in f.log] == ["batch_compress_n"] + ["compress_band"] * 5
    f.log.clear()
    back = pipeline.decompress_bands_u8([b"\x01"] * 4, config())
    assert [e[0] for e in f.log] == ["batch_decompress_n"] + ["decompress_band_u8"] * 4 and len(back) == 4


# ---- decompress_bands_u8 ------------------------------------------------------------------------------------------------------
def test_decompress_admitted(monkeypatch):
    f = Fakes(monkeypatch)
    back = pipeline.decompress_bands_u8([b"\x01", bytearray(b"\x02"), b"\x03", b"\x04"], config(4, 3, None, 150, 210))
    assert f.log == [("batch_decompress_n", 4, 150, 210, 3, 4, "none", 0.0)]
    assert isinstance(back, list) and len(back) == 4 and all(b.shape == (150, 210) and b.dtype == np.uint8 and b.all() for b in back)
    f.log.clear()
    q = pipeline.QuantizationMethod("qtable")
    back = pipeline.decompress_bands_u8([b"\x01"] * 4, config(8, 2, q, 30, 50))
    assert f.log == [("batch_decompress", 4, 16, 32, 2, "qtable", 0.0, ("out", "u8"))]     # 15 x 25 pooled samples: 2 x 4 blocks
    assert all(b.shape == (30, 50) for b in back)


@pytest.mark.parametrize("what", ["an array among the blobs", "an empty blob", "a divisor that is no integer", "one blob", "planes below DCTN_MIN_SAMPLES",
                                  "a height that is no integer"])
def test_decompress_loops(monkeypatch, what):
    f = Fakes(monkeypatch)
    blobs, cfg = [b"\x01"] * 5, config()
    if what == "an array among the blobs":
        blobs = [b"\x01", np.zeros((1, 1, 16)), b"\x01", b"\x01", b"\x01"]
    elif what == "an empty blob":
        blobs = [b"\x01", b"", b"\x01", b"\x01", b"\x01"]
    elif what == "a divisor that is no integer":
        cfg = config(quant=pipeline.QuantizationMethod("divide", divisor=2.5))
    elif what == "one blob":
        blobs = blobs[:1]
    elif what == "planes below DCTN_MIN_SAMPLES":
        cfg = config(height=8, width=8)
    else:
        cfg = config(height=40.0)
    back = pipeline.decompress_bands_u8(blobs, cfg)
    assert f.log == [("decompress_band_u8",)] * len(blobs) and len(back) == len(blobs)
