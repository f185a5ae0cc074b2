"""The dispatch of pipeline.probe_picture_sizes and probe_picture_distortion at dct_size 8: both roads are stubs (the jpegx
entries replaced, the device declared usable, the loops replaced), so only the choice of road and the arguments are asked.
DCT8_PROBE_MIN_CANDIDATES and DCT8_DISTORTION_MIN_CANDIDATES ship as None, which keeps the loop; set, they send 'divide' at
dct_size 8 to jpegx.batch_probe_pictures / batch_probe_distortion_pictures, while every other size goes on to the _n entries
under the DCTN_* gates; qtable, a registry that is not stock, a refusal and a missing device keep the loop.  CPU only."""
import numpy as np
import pytest
from PIL import Image

import pipeline
from pipeline.base import AlgorithmStep, step_classes


def _config(rows, cols, bs, n, divisor=40, quantization=None):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, transform="DCT",
                                  quantization=quantization or pipeline.QuantizationMethod("divide", divisor=divisor))


def _pictures(count, rows, cols, mode, seed=7):
    rng = np.random.default_rng(seed)
    return [Image.fromarray(rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8), mode=mode) for _ in range(count)]


class Roads:
    """Four device entries and two loops stubbed.  The size entries answer sizes[p][b][q] = 1000 p + 100 b + divisor, the
    distortion entries twice that, flagged where ``flag`` = (picture, band, divisors) says so; the loops answer -7."""

    def __init__(self, monkeypatch, gate8=2, gate_n=2, flag=None, refuse=False):
        import jpegx
        self.calls, self.loops, self.flag, self.refuse = [], 0, flag, refuse
        monkeypatch.setattr(pipeline, "_device_usable", lambda: True)
        monkeypatch.setattr(pipeline, "DCT8_PROBE_MIN_CANDIDATES", gate8)
        monkeypatch.setattr(pipeline, "DCT8_DISTORTION_MIN_CANDIDATES", gate8)
        monkeypatch.setattr(pipeline, "DCTN_PROBE_MIN_CANDIDATES", gate_n)
        monkeypatch.setattr(pipeline, "DCTN_DISTORTION_MIN_CANDIDATES", gate_n)
        monkeypatch.setattr(pipeline, "_probe_loop", self._loop)
        monkeypatch.setattr(pipeline, "_distortion_loop", self._loop3)
        monkeypatch.setattr(jpegx, "batch_probe_pictures", lambda px, bs, mode, params, **kw: self._device("sizes8", 1, px, (bs,), mode, params, kw))
        monkeypatch.setattr(jpegx, "batch_probe_distortion_pictures",
                            lambda px, bs, mode, params, **kw: self._device("sse8", 2, px, (bs,), mode, params, kw))
        monkeypatch.setattr(jpegx, "batch_probe_pictures_n",
                            lambda px, bs, n, mode, params, **kw: self._device("sizes_n", 1, px, (bs, n), mode, params, kw))
        monkeypatch.setattr(jpegx, "batch_probe_distortion_pictures_n",
                            lambda px, bs, n, mode, params, **kw: self._device("sse_n", 2, px, (bs, n), mode, params, kw))

    def _device(self, name, factor, pixels, head, mode, params, kw):
        import jpegx
        self.calls.append((name, pixels.shape, head, mode, list(params), kw))
        if self.refuse:
            raise jpegx.JpegxError("refused")
        k = pixels.shape[0]
        out = factor * (1000 * np.arange(k)[:, None, None] + 100 * np.arange(3)[None, :, None] + np.asarray(params)[None, None, :])
        bad = np.zeros(out.shape, bool)
        if self.flag is not None:
            bad[self.flag[0], self.flag[1], [params.index(float(d)) for d in self.flag[2] if float(d) in params]] = True
        return out.astype(np.uint64), bad

    def _loop(self, images, config, divisors, colour):
        self.loops += 1
        return np.full((len(images), len(divisors)), -7, np.int64)

    def _loop3(self, images, config, divisors, colour):
        self.loops += 1
        return np.full((len(images), 3, len(divisors)), -7, np.int64)


BIG = (64, 64)
PROBES = [("sizes", pipeline.probe_picture_sizes), ("sse", pipeline.probe_picture_distortion)]


def test_the_gates_ship_as_none():
    assert pipeline.DCT8_PROBE_MIN_CANDIDATES is None and pipeline.DCT8_DISTORTION_MIN_CANDIDATES is None


@pytest.mark.parametrize("what, probe", PROBES)
def test_the_gate(monkeypatch, what, probe):
    images = _pictures(2, *BIG, "YCbCr")
    config = _config(*BIG, 4, 8)
    for gate, count, device in ((None, 32, False), (3, 2, False), (3, 3, True), (3, 5, True), (1, 1, True), (0, 1, True)):
        r = Roads(monkeypatch, gate8=gate)
        got = probe(images, config, list(range(1, count + 1)))
        assert (len(r.calls), r.loops) == ((1, 0) if device else (0, 1)), (gate, count)
        if device:
            name, shape, head, mode, params, kw = r.calls[0]
            assert (name, shape, head, mode, kw) == (what + "8", (2, 64, 64, 3), (4,), "divide", {})
            assert params == [float(d) for d in range(1, count + 1)] and all(isinstance(p, float) for p in params)
        else:
            assert (got == -7).all()


def test_sizes_add_the_header_and_the_prefixes(monkeypatch):
    images = _pictures(2, *BIG, "YCbCr")
    divisors = [3, 40, 1000]
    Roads(monkeypatch)
    got = pipeline.probe_picture_sizes(images, _config(*BIG, 1, 8), divisors)
    heads = [len(pipeline.file_format.create_header(_config(*BIG, 1, 8, d))) for d in divisors]
    want = [[sum(1000 * p + 100 * b + d for b in range(3)) + heads[j] + 12 for j, d in enumerate(divisors)] for p in range(2)]
    assert got.dtype == np.int64 and got.tolist() == want and heads[2] - heads[0] == 3


def test_distortion_comes_back_band_by_band(monkeypatch):
    images = _pictures(2, *BIG, "YCbCr")
    Roads(monkeypatch)
    got = pipeline.probe_picture_distortion(images, _config(*BIG, 1, 8), [3, 40])
    assert got.dtype == np.int64 and got[1, 2].tolist() == [2 * 1203, 2 * 1240] and got.shape == (2, 3, 2)


@pytest.mark.parametrize("what, probe", PROBES)
def test_other_sizes_still_go_to_the_n_entries(monkeypatch, what, probe):
    images = _pictures(2, *BIG, "YCbCr")
    r = Roads(monkeypatch, gate8=1)
    probe(images, _config(*BIG, 1, 4), [2, 3, 4])
    assert r.loops == 0 and [c[0] for c in r.calls] == [what + "_n"] and r.calls[0][2] == (1, 4)
    r = Roads(monkeypatch, gate8=1, gate_n=None)                           # the DCT8 gate opens nothing for another size
    probe(images, _config(*BIG, 1, 4), [2, 3, 4])
    assert (len(r.calls), r.loops) == (0, 1)
    r = Roads(monkeypatch, gate8=None, gate_n=1)                           # nor the DCTN gate anything for dct_size 8
    probe(images, _config(*BIG, 1, 8), [2, 3, 4])
    assert (len(r.calls), r.loops) == (0, 1)


@pytest.mark.parametrize("what, probe", PROBES)
def test_what_keeps_the_loop(monkeypatch, what, probe):
    images = _pictures(2, *BIG, "YCbCr")
    config = _config(*BIG, 1, 8)
    # another transform; pictures of another size than the configuration's; a block_size beyond 255
    dft = pipeline.Configuration(width=64, height=64, block_size=1, dct_size=8, transform="DFT",
                                 quantization=pipeline.QuantizationMethod("divide", divisor=40))
    for imgs, cfg in ((images, dft), (images, _config(64, 56, 1, 8)), (_pictures(1, 512, 512, "YCbCr"), _config(512, 512, 256, 8))):
        r = Roads(monkeypatch)
        probe(imgs, cfg, [2, 3, 4])
        assert (len(r.calls), r.loops) == (0, 1), (cfg.transform, cfg.width, cfg.block_size)
    # with colour='rgb', pictures of another mode keep the loop; RGB pictures go up with the flag
    r = Roads(monkeypatch)
    probe(images, config, [2, 3, 4], colour="rgb")
    assert (len(r.calls), r.loops) == (0, 1)
    r = Roads(monkeypatch)
    probe(_pictures(2, *BIG, "RGB"), config, [2, 3, 4], colour="rgb")
    assert (len(r.calls), r.loops) == (1, 0) and r.calls[0][5] == {"colour": "rgb"} and r.calls[0][0] == what + "8"
    # a refusal of the library
    r = Roads(monkeypatch, refuse=True)
    got = probe(images, config, [2, 3, 4])
    assert (len(r.calls), r.loops) == (1, 1) and (got == -7).all()
    # no device
    r = Roads(monkeypatch)
    monkeypatch.setattr(pipeline, "_device_usable", lambda: False)
    probe(images, config, [2, 3, 4])
    assert (len(r.calls), r.loops) == (0, 1)


@pytest.mark.parametrize("what, probe", PROBES)
def test_qtable_is_not_a_probe_configuration(monkeypatch, what, probe):
    """The pipeline probes vary the divisor: any other quantiser is a ValueError before a road is chosen, the device entries'
    qtable notwithstanding."""
    r = Roads(monkeypatch, gate8=1)
    for q in (pipeline.QuantizationMethod("qtable"), pipeline.QuantizationMethod("none"), pipeline.QuantizationMethod("discard", keep=2)):
        with pytest.raises(ValueError, match="must be 'divide'"):
            probe(_pictures(1, *BIG, "YCbCr"), _config(*BIG, 1, 8, quantization=q), [2])
    assert (len(r.calls), r.loops) == (0, 0)
    # and _probe_job itself admits 'divide' alone
    assert pipeline._probe_job(_pictures(1, *BIG, "YCbCr"), _config(*BIG, 1, 8, quantization=pipeline.QuantizationMethod("qtable")), [2], None, 1, 1) is None
    assert pipeline._probe_job(_pictures(1, *BIG, "YCbCr"), _config(*BIG, 1, 8), [2], None, 1, 1) is not None


@pytest.mark.parametrize("what, probe", PROBES)
def test_a_non_stock_registry_keeps_the_loop(monkeypatch, what, probe):
    stock = list(step_classes)
    try:
        class PassThrough(AlgorithmStep):
            step_index = 9.5

            def execute(self, array):
                return array

            def invert(self, array):
                return array
        assert not pipeline._stock_registry()
        r = Roads(monkeypatch)
        probe(_pictures(1, *BIG, "YCbCr"), _config(*BIG, 1, 8), [2, 3, 4])
        assert (len(r.calls), r.loops) == (0, 1)
    finally:
        step_classes[:] = stock
    assert pipeline._stock_registry()


def test_slices_of_thirty_two_and_minus_one_from_the_flag(monkeypatch):
    images = _pictures(3, 37, 53, "YCbCr")
    config = _config(37, 53, 3, 8)
    divisors = [3 * k + 1 for k in range(70)]
    r = Roads(monkeypatch, flag=(1, 2, [4, 100]))                          # band 2 of picture 1 under divisors 4 and 100
    got = pipeline.probe_picture_distortion(images, config, divisors)
    assert [len(c[4]) for c in r.calls] == [32, 32, 6] and sum((c[4] for c in r.calls), []) == [float(d) for d in divisors]
    assert all(c[:3] == ("sse8", (3, 37, 53, 3), (3,)) for c in r.calls)
    want = 2 * (1000 * np.arange(3)[:, None, None] + 100 * np.arange(3)[None, :, None] + np.asarray(divisors)[None, None, :])
    want[1, :, [divisors.index(4), divisors.index(100)]] = -1              # the whole picture: Jpeg.compress raises for it
    assert np.array_equal(got, want)
    r = Roads(monkeypatch, flag=(1, 2, [4, 100]))
    sizes = pipeline.probe_picture_sizes(images, config, divisors)
    assert (sizes[1, [1, 33]] == -1).all() and (sizes == -1).sum() == 2 and [len(c[4]) for c in r.calls] == [32, 32, 6]
    r = Roads(monkeypatch, flag=(1, 2, [4, 100]))
    psnr = pipeline.probe_picture_psnr(images, config, divisors)
    assert np.isnan(psnr[1, [1, 33]]).all() and np.isnan(psnr).sum() == 2


@pytest.mark.parametrize("what, probe", PROBES)
def test_a_block_size_that_is_no_integer_keeps_the_loop(monkeypatch, what, probe):
    """_job_config_8 lets a block_size such as 2.0 through, the container's header does not: the loop raises for it, so the
    device road must not answer in its place.  An integer block_size is handed on as an int, as the N branch hands its sizes on."""
    r = Roads(monkeypatch)
    probe(_pictures(1, *BIG, "YCbCr"), _config(*BIG, 2.0, 8), [2, 3])
    assert (len(r.calls), r.loops) == (0, 1)
    r = Roads(monkeypatch)
    probe(_pictures(1, *BIG, "YCbCr"), _config(*BIG, np.int64(2), 8), [2, 3])
    assert (len(r.calls), r.loops) == (1, 0) and r.calls[0][2] == (2,) and type(r.calls[0][2][0]) is int


def test_an_array_of_pictures_goes_up_as_it_is(monkeypatch):
    stack = np.stack([np.asarray(im) for im in _pictures(2, *BIG, "YCbCr")])
    r = Roads(monkeypatch)
    pipeline.probe_picture_sizes(stack, _config(*BIG, 2, 8), [2, 3])
    assert len(r.calls) == 1 and r.calls[0][:3] == ("sizes8", (2, 64, 64, 3), (2,))
