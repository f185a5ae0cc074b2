"""pipeline.compress_to_size and compress_pictures_to_size: the divisor is the one the documented search defines (hand-worked
size tables, one of them not monotone), the container keeps the budget and decodes, nothing fitting is TargetSizeError, a
probe that disagrees with the compression is RuntimeError, and the batch form returns per-picture rungs in input order with
the containers of the per-picture compressions.  CPU only: recorded tables, and the host road on 24 x 24 pictures."""
import numpy as np
import pytest
from PIL import Image

import pipeline


def _config(rows=24, cols=24, bs=1, n=4, divisor=40):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, transform="DCT",
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


class Recorded:
    """probe_picture_sizes and Jpeg.compress replaced by a size table: size(divisor) -> bytes (-1: BadRleCodeError)."""

    def __init__(self, monkeypatch, size, lie=0):
        self.calls = []
        outer = self

        def probe(images, config, divisors, colour=None):
            outer.calls.append(list(divisors))
            return np.array([[size(d) for d in divisors] for _ in images], dtype=np.int64)

        class FakeJpeg:
            def __init__(self, config):
                self.divisor = config.quantization.params["divisor"]

            def compress(self, image):
                return b"\x00" * (size(self.divisor) + lie)

            compress_rgb = compress

        monkeypatch.setattr(pipeline, "probe_picture_sizes", probe)
        monkeypatch.setattr(pipeline, "Jpeg", FakeJpeg)


def test_monotone_table(monkeypatch):
    rec = Recorded(monkeypatch, lambda d: 1000 // d + 100)
    # 1, 2, 4, 8, 16 -> 1100, 600, 350, 225, 162: f = 8, g = 4; then 5, 6, 7 -> 300, 266, 242: f = 5, nothing left between 4 and 5
    container, divisor = pipeline.compress_to_size("picture", _config(), 300, lo=1, hi=16, probes=5)
    assert divisor == 5 and len(container) == 300
    assert rec.calls == [[1, 2, 4, 8, 16], [5, 6, 7]]


def test_table_that_is_not_monotone(monkeypatch):
    table = {1: 900, 2: 800, 4: 250, 8: 700, 16: 200, 3: 280}
    rec = Recorded(monkeypatch, table.__getitem__)
    # the smallest fitting candidate is 4 although 8 does not fit; g = 2; 3 fits -> f = 3
    container, divisor = pipeline.compress_to_size("picture", _config(), 300, lo=1, hi=16, probes=5)
    assert (divisor, len(container)) == (3, 280) and rec.calls == [[1, 2, 4, 8, 16], [3]]
    table[3] = 500                                      # ... and where 3 does not fit, f stays 4
    rec.calls.clear()
    container, divisor = pipeline.compress_to_size("picture", _config(), 300, lo=1, hi=16, probes=5)
    assert (divisor, len(container)) == (4, 250) and rec.calls == [[1, 2, 4, 8, 16], [3]]


def test_rounds_of_evenly_spaced_probes(monkeypatch):
    rec = Recorded(monkeypatch, lambda d: 2000 // d)
    # 1, 10, 100 -> 2000, 200, 20: f = 100, g = 10.  11..99 by index 0, 44, 88: 11, 55, 99 -> 181, 36, 20: f = 55, g = 11.
    # 12..54: 12, 33, 54 -> 166, 60, 37: f = 33, g = 12.  13..32: 13, 22, 32 -> 153, 90, 62: f = 22, g = 13.  Three rounds are spent.
    container, divisor = pipeline.compress_to_size("picture", _config(), 150, lo=1, hi=100, probes=3, rounds=3)
    assert (divisor, len(container)) == (22, 90)
    assert rec.calls == [[1, 10, 100], [11, 55, 99], [12, 33, 54], [13, 22, 32]]
    rec.calls.clear()
    assert pipeline.compress_to_size("picture", _config(), 150, lo=1, hi=100, probes=3, rounds=0)[1] == 100
    assert rec.calls == [[1, 10, 100]]
    assert pipeline.compress_to_size("picture", _config(), 150, lo=1, hi=100, probes=3, rounds=1)[1] == 55
    # with room for all the numbers in between, the answer is the smallest fitting divisor there is: 2000 // 14 = 142
    assert pipeline.compress_to_size("picture", _config(), 150, lo=1, hi=100, probes=16, rounds=3)[1] == 14


def test_flagged_entries_do_not_fit(monkeypatch):
    Recorded(monkeypatch, lambda d: -1 if d < 6 else 1000 // d)
    container, divisor = pipeline.compress_to_size("picture", _config(), 10 ** 6, lo=1, hi=16, probes=5)
    assert (divisor, len(container)) == (6, 166)


def test_nothing_fits(monkeypatch):
    Recorded(monkeypatch, lambda d: 1000 // d + 100)
    with pytest.raises(pipeline.TargetSizeError, match=r"smallest size seen is 162 bytes, at divisor 16") as info:
        pipeline.compress_to_size("picture", _config(), 161, lo=1, hi=16, probes=5)
    assert isinstance(info.value, ValueError)
    Recorded(monkeypatch, lambda d: -1)
    with pytest.raises(pipeline.TargetSizeError, match="BadRleCodeError"):
        pipeline.compress_to_size("picture", _config(), 10 ** 6, lo=1, hi=16, probes=5)


def test_probe_and_compression_must_agree(monkeypatch):
    Recorded(monkeypatch, lambda d: 1000 // d + 100, lie=1)
    with pytest.raises(RuntimeError, match="divisor 5 was probed at 300 bytes, its container holds 301"):
        pipeline.compress_to_size("picture", _config(), 300, lo=1, hi=16, probes=5)


def test_bad_search_arguments():
    for kw in (dict(lo=0), dict(lo=5, hi=4), dict(probes=0), dict(rounds=-1), dict(lo=1.5)):
        with pytest.raises(ValueError):
            pipeline.compress_to_size("picture", _config(), 300, **kw)


# ---- the real host road ---------------------------------------------------------------------------------------------------
def _picture(kind, mode="YCbCr", rows=24, cols=24):
    rng = np.random.default_rng(kind)
    yy, xx = np.mgrid[0:rows, 0:cols]
    if kind == 0:
        px = np.full((rows, cols, 3), 90)
    elif kind == 1:
        px = np.repeat(((yy * 5 + xx * 3) % 256)[..., None], 3, axis=2)
    elif kind == 2:
        px = rng.integers(0, 256, (rows, cols, 3))
    else:
        px = np.where((xx < cols // 2)[..., None], rng.integers(0, 256, (rows, cols, 3)), 128)
    return Image.fromarray(px.astype(np.uint8), mode=mode)


def _size(image, config, d, colour):
    codec = pipeline.Jpeg(_config(config.height, config.width, config.block_size, config.dct_size, d))
    return len(codec.compress(image) if colour is None else codec.compress_rgb(image))


def _search(size, max_bytes, lo, hi, probes, rounds):
    """The documented search, written down a second time over a size function."""
    ratio = hi / lo
    cand = sorted({lo, hi} | {min(hi, max(lo, int(round(lo * ratio ** (i / (probes - 1.0)))))) for i in range(1, probes - 1)})
    fit = [d for d in cand if size(d) <= max_bytes]
    f = fit[0]
    g = max([d for d in cand if d < f], default=lo - 1)
    for _ in range(rounds):
        m = f - g - 1
        inner = list(range(g + 1, f)) if m <= probes else sorted({g + 1 + (i * (m - 1)) // (probes - 1) for i in range(probes)})
        if not inner:
            break
        fit = [d for d in inner if size(d) <= max_bytes]
        f = fit[0] if fit else f
        g = max([d for d in inner if d < f], default=g)
    return f


@pytest.mark.parametrize("colour", [None, "rgb"])
def test_host_road_keeps_the_budget_and_decodes(colour):
    image = _picture(3, "YCbCr" if colour is None else "RGB")
    config = _config()
    for max_bytes in (1500, 700):
        container, divisor = pipeline.compress_to_size(image, config, max_bytes, colour=colour, lo=1, hi=512, probes=6, rounds=2)
        assert len(container) <= max_bytes
        assert divisor == _search(lambda d: _size(image, config, d, colour), max_bytes, 1, 512, 6, 2)
        assert container == (pipeline.Jpeg(_config(divisor=divisor)).compress(image) if colour is None
                             else pipeline.Jpeg(_config(divisor=divisor)).compress_rgb(image))
        back = pipeline.Jpeg.decompress(container)
        assert back.size == (24, 24) and back.mode == "YCbCr"
    with pytest.raises(pipeline.TargetSizeError):
        pipeline.compress_to_size(image, config, 40, colour=colour, lo=1, hi=512, probes=6)


def test_pictures_to_size_picks_rungs_per_picture_in_input_order():
    images = [_picture(k) for k in (2, 0, 3, 1, 2)]
    config = _config()
    ladder = [2, 10, 50, 400]
    sizes = pipeline.probe_picture_sizes(images, config, ladder)
    max_bytes = int(sizes[0][2])                           # the noise picture fits from the third rung on
    containers, chosen = pipeline.compress_pictures_to_size(images, config, max_bytes, ladder)
    want = [next(d for d, s in zip(ladder, row) if s <= max_bytes) for row in sizes]
    assert chosen == want and chosen[0] == chosen[4] == 50 and chosen[1] == 2 and len(set(chosen)) >= 2
    for im, d, c in zip(images, chosen, containers):
        assert c == pipeline.Jpeg(_config(divisor=d)).compress(im) and len(c) <= max_bytes
    # an array of pictures goes the same way
    stack = np.stack([np.asarray(im) for im in images])
    assert pipeline.compress_pictures_to_size(stack, config, max_bytes, ladder) == (containers, chosen)


def test_pictures_to_size_errors():
    images = [_picture(0), _picture(2), _picture(2)]
    config = _config()
    with pytest.raises(pipeline.TargetSizeError, match="picture 1 fits no rung within 600 bytes"):
        pipeline.compress_pictures_to_size(images, config, 600, [2, 10])
    for ladder in ([], [10, 2], [2, 2], list(range(1, 34)), [2.5]):
        with pytest.raises(ValueError):
            pipeline.compress_pictures_to_size(images, config, 10 ** 6, ladder)
