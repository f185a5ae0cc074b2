"""pipeline.compress_to_quality and compress_pictures_to_quality on a stubbed probe: the search takes exactly the steps its
docstring names on a made-up PSNR table that is not monotone in the divisor, costs 1 + rounds probes at most and one compression,
TargetQualityError names the best PSNR seen, arguments are checked, and the batch keeps the input order.  CPU only: neither the
probe nor a codec runs."""
import numpy as np
import pytest

import pipeline


def _config(divisor=40):
    return pipeline.Configuration(width=32, height=24, block_size=1, dct_size=4, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


class Table:
    """psnr(d) = 50 - 0.2 d unless ``special`` says otherwise; records the candidate lists probed and the compressions made."""

    def __init__(self, monkeypatch, special=None):
        self.special, self.probed, self.made = special or {}, [], []
        monkeypatch.setattr(pipeline, "probe_picture_psnr", self.probe)
        monkeypatch.setattr(pipeline, "_compress_one", self.compress)

    def psnr(self, d):
        return self.special.get(d, 50.0 - 0.2 * d)

    def probe(self, images, config, divisors, colour=None):
        assert len(images) == 1
        self.probed.append(list(divisors))
        return np.array([[self.psnr(d) for d in divisors]])

    def compress(self, image, config, colour):
        self.made.append(config.quantization.gpu_mode()[1])
        return b"container-%d" % config.quantization.gpu_mode()[1]


def test_the_search_path_on_a_table_that_is_not_monotone(monkeypatch):
    # 23 dips below the floor between two numbers that meet it; 49 misses it although 50 would meet it again
    t = Table(monkeypatch, {23: 10.0, 49: 39.0, 50: 41.0})
    got = pipeline.compress_to_quality("picture", _config(), 40.0, lo=1, hi=100, probes=4, rounds=2)
    assert t.probed == [[1, 5, 22, 100],                 # geometric; 22 is the largest that meets 40 dB (45.6), 100 misses (30)
                        [23, 48, 73, 99],                # evenly between 22 and 100: 48 meets (40.4), 73 does not -> f 48, g 73
                        [49, 56, 64, 72]]                # between 48 and 73: none meets -> f stays 48, g 49
    assert got == (b"container-48", 48, pytest.approx(40.4)) and t.made == [48.0]
    # a third round has nothing left between 48 and 49
    t = Table(monkeypatch, {23: 10.0, 49: 39.0, 50: 41.0})
    assert pipeline.compress_to_quality("picture", _config(), 40.0, lo=1, hi=100, probes=4, rounds=5)[1] == 48 and len(t.probed) == 3
    # no rounds: the geometric candidate itself
    t = Table(monkeypatch)
    assert pipeline.compress_to_quality("picture", _config(), 40.0, lo=1, hi=100, probes=4, rounds=0)[1:] == (22, pytest.approx(45.6))
    assert len(t.probed) == 1 and t.made == [22.0]


def test_the_top_candidate_and_nan(monkeypatch):
    # every candidate meets the floor: f = hi, g = hi + 1, nothing lies between
    t = Table(monkeypatch)
    assert pipeline.compress_to_quality("picture", _config(), 10.0, lo=1, hi=100, probes=4)[1] == 100 and len(t.probed) == 1
    # nan (the picture cannot be coded under that divisor) never meets a floor, not even minus infinity
    t = Table(monkeypatch, {1: float("nan"), 5: float("nan"), 22: float("nan"), 100: float("nan"), 30: float("nan")})
    with pytest.raises(pipeline.TargetQualityError, match="codes the picture at all"):
        pipeline.compress_to_quality("picture", _config(), float("-inf"), lo=1, hi=100, probes=4)
    t = Table(monkeypatch, {100: float("nan"), 99: float("nan")})
    container, f, psnr = pipeline.compress_to_quality("picture", _config(), 20.0, lo=1, hi=100, probes=4, rounds=1)
    assert t.probed[1] == [23, 48, 73, 99] and (f, psnr) == (73, pytest.approx(35.4))
    # inf (nothing lost) meets every floor
    t = Table(monkeypatch, {1: float("inf")})
    assert pipeline.compress_to_quality("picture", _config(), 1000.0, lo=1, hi=100, probes=4, rounds=0)[1:] == (1, float("inf"))


def test_target_quality_error_names_the_best_psnr_seen(monkeypatch):
    Table(monkeypatch, {5: 49.9})
    with pytest.raises(pipeline.TargetQualityError) as exc:
        pipeline.compress_to_quality("picture", _config(), 60.0, lo=1, hi=100, probes=4)
    assert str(exc.value) == "no divisor in 1..100 keeps the picture at 60.00 dB or above: the best PSNR seen is 49.90 dB, at divisor 5"
    assert isinstance(exc.value, ValueError)


def test_argument_checks(monkeypatch):
    t = Table(monkeypatch)
    for kw in (dict(lo=0), dict(hi=0), dict(lo=5, hi=4), dict(probes=0), dict(rounds=-1), dict(lo=1.5), dict(probes=True)):
        with pytest.raises(ValueError, match="lo, hi, probes and rounds"):
            pipeline.compress_to_quality("picture", _config(), 40.0, **kw)
    for bad in (None, "40", float("nan"), True):
        with pytest.raises(ValueError, match="min_psnr"):
            pipeline.compress_to_quality("picture", _config(), bad)
    with pytest.raises(ValueError, match="colour"):
        pipeline.compress_to_quality("picture", _config(), 40.0, colour="bgr")
    assert t.probed == [] and t.made == []


def test_the_real_probe_refuses_a_configuration_that_is_not_divide():
    config = pipeline.Configuration(width=32, height=24, block_size=1, dct_size=4, quantization=pipeline.QuantizationMethod("none"))
    with pytest.raises(ValueError, match="must be 'divide'"):
        pipeline.compress_to_quality("picture", config, 40.0)
    with pytest.raises(ValueError, match="must be 'divide'"):
        pipeline.compress_pictures_to_quality(["picture"], config, 40.0, [2, 3])


def test_a_batch_keeps_the_input_order(monkeypatch):
    ladder = [2, 8, 20, 60]
    table = np.array([[45.0, 38.0, 41.0, 30.0],          # not monotone: the largest rung that meets 40 dB is 20
                      [50.0, 45.0, 41.0, 40.0],          # 60
                      [40.0, 39.0, 39.5, 20.0],          # 2
                      [float("inf"), 44.0, 43.0, float("nan")],      # 20
                      [48.0, 47.0, 46.0, 45.0]])         # 60
    calls = []
    monkeypatch.setattr(pipeline, "probe_picture_psnr", lambda images, config, divisors, colour=None: (calls.append(list(divisors)), table)[1])

    def compress_pictures(group, config, colour=None):
        d = config.quantization.gpu_mode()[1]
        calls.append((d, list(group), colour))
        return [("%s@%d" % (name, d)).encode() for name in group]
    monkeypatch.setattr(pipeline, "compress_pictures", compress_pictures)
    containers, chosen = pipeline.compress_pictures_to_quality(["a", "b", "c", "d", "e"], _config(), 40.0, ladder, colour="rgb")
    assert chosen == [20, 60, 2, 20, 60]
    assert containers == [b"a@20", b"b@60", b"c@2", b"d@20", b"e@60"]
    assert calls == [ladder, (2.0, ["c"], "rgb"), (20.0, ["a", "d"], "rgb"), (60.0, ["b", "e"], "rgb")]      # ONE probe, one call per rung
    with pytest.raises(pipeline.TargetQualityError, match="picture 2 meets 40.50 dB on no rung: its best PSNR is 40.00 dB, at divisor 2"):
        pipeline.compress_pictures_to_quality(["a", "b", "c", "d", "e"], _config(), 40.5, ladder)
    for bad in ([], [3, 2], [2, 2], list(range(1, 34))):
        with pytest.raises(ValueError, match="ascending rungs"):
            pipeline.compress_pictures_to_quality(["a"], _config(), 40.0, bad)
