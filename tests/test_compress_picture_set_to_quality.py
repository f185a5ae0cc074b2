"""pipeline.compress_picture_set_to_quality on a stubbed probe: every picture gets the largest rung of the ladder that meets the
floor on a made-up PSNR table that is not monotone, one probe measures the set, every rung's pictures are one
compress_picture_set call, the input order is kept, TargetQualityError has compress_pictures_to_quality's wording and the ladder
is validated.  CPU only: neither the probe nor a codec runs."""
import numpy as np
import pytest

import pipeline


def _config(divisor=40):
    return pipeline.Configuration(width=1, height=1, block_size=1, dct_size=4, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


LADDER = [2, 8, 20, 60]
TABLE = np.array([[45.0, 38.0, 41.0, 30.0],          # not monotone: the largest rung that meets 40 dB is 20
                  [50.0, 45.0, 41.0, 40.0],          # 60
                  [40.0, 39.0, 39.5, 20.0],          # 2
                  [float("inf"), 44.0, 43.0, float("nan")],      # 20
                  [48.0, 47.0, 46.0, 45.0]])         # 60


def _stub(monkeypatch, table):
    calls = []
    monkeypatch.setattr(pipeline, "probe_picture_set_psnr",
                        lambda images, config, divisors, colour=None: (calls.append((list(images), list(divisors), colour)), table)[1])
    monkeypatch.setattr(pipeline, "probe_picture_psnr", lambda *a, **k: pytest.fail("the probe of one size is another road"))

    def compress_picture_set(group, config, colour=None):
        d = config.quantization.gpu_mode()[1]
        calls.append((d, list(group), colour))
        return [("%s@%d" % (name, d)).encode() for name in group]
    monkeypatch.setattr(pipeline, "compress_picture_set", compress_picture_set)
    monkeypatch.setattr(pipeline, "compress_pictures", lambda *a, **k: pytest.fail("pictures of one size are another road"))
    return calls


def test_largest_meeting_rung_one_probe_one_call_per_rung_input_order(monkeypatch):
    calls = _stub(monkeypatch, TABLE)
    names = ["a", "b", "c", "d", "e"]
    containers, chosen = pipeline.compress_picture_set_to_quality(iter(names), _config(), 40.0, LADDER, colour="rgb")
    assert chosen == [20, 60, 2, 20, 60]
    assert containers == [b"a@20", b"b@60", b"c@2", b"d@20", b"e@60"]
    assert calls == [(names, LADDER, "rgb"), (2.0, ["c"], "rgb"), (20.0, ["a", "d"], "rgb"), (60.0, ["b", "e"], "rgb")]
    # inf meets every floor, nan none
    _stub(monkeypatch, TABLE[3:4])
    containers, chosen = pipeline.compress_picture_set_to_quality(names[3:4], _config(), 1000.0, LADDER)
    assert chosen == [2] and containers == [b"d@2"]


def test_target_quality_error_texts(monkeypatch):
    _stub(monkeypatch, TABLE)
    with pytest.raises(pipeline.TargetQualityError) as exc:
        pipeline.compress_picture_set_to_quality(["a", "b", "c", "d", "e"], _config(), 40.5, LADDER)
    assert str(exc.value) == "picture 2 meets 40.50 dB on no rung: its best PSNR is 40.00 dB, at divisor 2"
    assert isinstance(exc.value, ValueError)
    _stub(monkeypatch, np.array([[50.0] * 4, [float("nan")] * 4]))
    with pytest.raises(pipeline.TargetQualityError) as exc:
        pipeline.compress_picture_set_to_quality(["a", "b"], _config(), float("-inf"), LADDER)
    assert str(exc.value) == "picture 1 meets -inf dB on no rung (BadRleCodeError at every rung)"
    # two rungs of one best PSNR: the larger divisor is named
    _stub(monkeypatch, np.array([[30.0, 30.0, 29.0, float("nan")]]))
    with pytest.raises(pipeline.TargetQualityError, match="picture 0 meets 35.00 dB on no rung: its best PSNR is 30.00 dB, at divisor 2$"):
        pipeline.compress_picture_set_to_quality(["a"], _config(), 35.0, LADDER)


def test_ladder_and_argument_validation(monkeypatch):
    calls = _stub(monkeypatch, TABLE)
    for bad in ([], [3, 2], [2, 2], list(range(1, 34))):
        with pytest.raises(ValueError, match="compress_picture_set_to_quality: divisors must be 1..32 ascending rungs"):
            pipeline.compress_picture_set_to_quality(["a"], _config(), 40.0, bad)
    with pytest.raises(ValueError, match="whole positive number"):
        pipeline.compress_picture_set_to_quality(["a"], _config(), 40.0, [2, 2.5])
    with pytest.raises(ValueError, match="colour"):
        pipeline.compress_picture_set_to_quality(["a"], _config(), 40.0, LADDER, colour="bgr")
    config = pipeline.Configuration(width=1, height=1, block_size=1, dct_size=4, quantization=pipeline.QuantizationMethod("none"))
    with pytest.raises(ValueError, match="must be 'divide'"):
        pipeline.compress_picture_set_to_quality(["a"], config, 40.0, LADDER)
    assert calls == []
    # 32 rungs are taken
    ladder = list(range(1, 33))
    _stub(monkeypatch, np.full((1, 32), 41.0))
    assert pipeline.compress_picture_set_to_quality(["a"], _config(), 40.0, ladder)[1] == [32]
