"""GPU: every road of compress_band / decompress_band / decompress_band_u8 for dct_size != 8 against the product-free
oracle of tests/codec_oracle_n.py (pinned to the unmodified reference by tests/test_codec_oracle_n.py), over the pairwise
matrix of codec_oracle_n.matrix_cases(): N in 2..32, block sizes 1..255, every quantiser, ragged / exact / one-row /
one-column / one-sample bands.

Forward roads, each forced through the gates of pipeline/__init__.py and shown by a spy on its jpegx entry to have run:
  F  jpegx.forward_fused_n + the host coder jpegx.entropy_encode_n
  J  jpegx.compress_plane_n (steps 4-8 as one device job)
  B  jpegx.compress_band_n (all nine steps from the 8-bit band), from uint8, int32, int64, int16 and a strided view
  X  a registry with a pass-through step appended: jpegx.forward_fused_n + the host step classes
Roads back, each through decompress_band and decompress_band_u8, on the product's bytes and on the oracle's:
  P  the host parser jpegx.entropy_decode_n + jpegx.inverse_fused_n
  D  jpegx.decompress_plane_n, out 'i32' and 'u8'
A case is 'free' (the oracle's values keep 100 tau from every rounding tie, asserted when the case is built: bytes and
bands must be equal) or 'ties' (8-bit noise: the criterion of tests/dctn_criterion.py against the oracle's unrounded
values, the mismatch capped by the tie share alone, and the stream the canonical coding of its integers).

With a divisor that is no integer the reference truncates the restored coefficients (codec_oracle_n.restore); the
decode job does not, so road D hands such a stream to road P, which restores on the host -- the spies assert that too.
"""
import contextlib

import numpy as np
import pytest

import codec_oracle_n as on
from test_codec_oracle_n import (Known, case_id, check_compressed, check_decoded, check_host_road, check_refusals, config_of,
                                 host_road_needs_a_device, known, refusal_cases)

pytestmark = pytest.mark.gpu

ENTRIES = ("forward_fused_n", "entropy_encode_n", "compress_plane_n", "compress_band_n", "entropy_decode_n", "inverse_fused_n",
           "decompress_plane_n")
# road -> (DCTN_ENTROPY_MIN_SAMPLES, DCTN_BAND_JOB_MIN_SAMPLES, the entries that run once each)
FORWARD = {"F": (None, None, {"forward_fused_n": 1, "entropy_encode_n": 1}), "J": (0, None, {"compress_plane_n": 1}),
           "B": (None, 0, {"compress_band_n": 1}), "X": (None, None, {"forward_fused_n": 1})}
# road -> (DCTN_ENTROPY_DECODE_MIN_SAMPLES, the entries that run once each)
BACK = {"P": (None, {"entropy_decode_n": 1, "inverse_fused_n": 1}), "D": (0, {"decompress_plane_n": 1})}


class Spies:
    def __init__(self, gpu, monkeypatch):
        self.calls = []
        for name in ENTRIES:
            monkeypatch.setattr(gpu, name, self._spy(name, getattr(gpu, name)))

    def _spy(self, name, real):
        def entry(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return real(*args, **kwargs)
        return entry

    def take(self):
        """{entry: calls} since the last take, and the calls themselves."""
        calls, self.calls = self.calls, []
        counts = {}
        for name, _, _ in calls:
            counts[name] = counts.get(name, 0) + 1
        return counts, calls


@pytest.fixture
def spies(gpu, monkeypatch):
    return Spies(gpu, monkeypatch)


@contextlib.contextmanager
def forward_road(monkeypatch, road):
    import pipeline
    from pipeline.base import AlgorithmStep, step_classes
    entropy, band_job, _ = FORWARD[road]
    stock = list(step_classes)
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
        m.setattr(pipeline, "DCTN_ENTROPY_MIN_SAMPLES", entropy)
        m.setattr(pipeline, "DCTN_BAND_JOB_MIN_SAMPLES", band_job)
        try:
            if road == "X":
                class PassThrough(AlgorithmStep):
                    step_index = 9.5

                    def execute(self, array):
                        return array

                    def invert(self, array):
                        return array
                assert not pipeline._stock_registry()
            yield
        finally:
            step_classes[:] = stock


@contextlib.contextmanager
def back_road(monkeypatch, road):
    import pipeline
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
        m.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", BACK[road][0])
        yield


def band_forms(band):
    """The band as every dtype and layout the band job is documented to take (int16 goes up as int64)."""
    h, w = band.shape
    wide = np.zeros((h, w + 5), np.uint8)
    wide[:, :w] = band
    return [("uint8", band.astype(np.uint8)), ("int32", band.astype(np.int32)), ("int64", band.astype(np.int64)),
            ("int16", band.astype(np.int16)), ("strided", wide[:, :w])]


def run_forward_roads(monkeypatch, spies, k):
    """Every forward road on case k: the road ran, and its bytes meet the oracle.  Returns {road: bytes}."""
    import pipeline
    cfg, blobs = k.config(), {}
    for road, (_, _, expected) in FORWARD.items():
        with forward_road(monkeypatch, road):
            spies.take()
            blob = pipeline.compress_band(k.band, cfg)
            counts, _ = spies.take()
            assert counts == expected, "road %s did not run as such for %s: %r" % (road, k.what, counts)
            check_compressed(blob, k, "%s %s" % (road, k.what))
            blobs[road] = blob
            if road == "B":
                for name, form in band_forms(k.band):
                    assert pipeline.compress_band(form, cfg) == blob, (k.what, name)
                    counts, calls = spies.take()
                    assert counts == expected, (k.what, name, counts)
                    assert calls[0][1][0].dtype == (np.int64 if name == "int16" else form.dtype)
    return blobs


def run_back_roads(monkeypatch, spies, k, blobs):
    """Every road back, through both entries, on each stream of blobs."""
    import pipeline
    cfg = k.config()
    whole = k.mode != "divide" or k.param == np.trunc(k.param)
    for road, (_, expected) in BACK.items():
        if road == "D" and not whole:
            expected = BACK["P"][1]                 # the job restores without the reference's truncation: it is not asked
        with back_road(monkeypatch, road):
            for name, blob in blobs:
                inv = k.inv if blob == k.blob else k.inverse(blob)
                for fn, dtype, out in ((pipeline.decompress_band, np.int64, "i32"), (pipeline.decompress_band_u8, np.uint8, "u8")):
                    spies.take()
                    got = fn(blob, cfg)
                    counts, calls = spies.take()
                    what = "%s %s %s %s" % (road, fn.__name__, name, k.what)
                    assert counts == expected, "road %s did not run as such: %s %r" % (road, what, counts)
                    if "decompress_plane_n" in expected:
                        assert calls[0][2]["out"] == out, what
                    elif not whole:
                        assert [c[1][2] for c in calls if c[0] == "inverse_fused_n"] == ["none"], what
                    check_decoded(got, inv, k.kind, what, dtype)


@pytest.mark.parametrize("case", on.matrix_cases(), ids=case_id)
def test_every_road_meets_the_oracle(gpu, monkeypatch, spies, case):
    k = known(case)
    blobs = run_forward_roads(monkeypatch, spies, k)
    own = sorted(set(blobs.values()) - {k.blob})
    assert len(own) <= 1, "the forward roads disagree among themselves for " + k.what
    run_back_roads(monkeypatch, spies, k, [("oracle", k.blob)] + [("own", b) for b in own])


@pytest.mark.parametrize("case", [c for c in on.matrix_cases() if host_road_needs_a_device(c[0], c[2])], ids=case_id)
def test_host_road_cells_that_need_a_device(gpu, monkeypatch, spies, case):
    """The host NumPy road at N = 16, 24, 32 under 'none' and 'divide' (tests/test_codec_oracle_n.py runs the other cells
    without a device): the quantiser objects use libjpegx's float64 quantiser kernel there, no entry of the N roads."""
    check_host_road(monkeypatch, case)
    assert spies.take()[0] == {}


def tie_free_noise(h, w, seed):
    """Multiples of 4 up to 252: off the ties under 'none' at N = 4 (codec_oracle_n.make_band); Known asserts it."""
    return np.random.default_rng(seed).integers(0, 64, (h, w)) * 4


def test_the_gates_as_shipped(gpu, spies):
    """All four constants as committed, N = 4, block_size 1, planes one block row either side of each gate: the road that the
    comments in pipeline/__init__.py promise runs, and the result is the oracle's on both sides."""
    import pipeline
    assert (pipeline.DCTN_MIN_SAMPLES, pipeline.DCTN_ENTROPY_MIN_SAMPLES, pipeline.DCTN_ENTROPY_DECODE_MIN_SAMPLES,
            pipeline.DCTN_BAND_JOB_MIN_SAMPLES) == (1024, None, 262144, 16384)
    host, f_road, b_road = {}, FORWARD["F"][2], FORWARD["B"][2]
    for h, w, forward, back in ((28, 32, host, host), (32, 32, f_road, BACK["P"][1]), (124, 128, f_road, BACK["P"][1]),
                                (128, 128, b_road, BACK["P"][1]), (508, 512, b_road, BACK["P"][1]), (512, 512, b_road, BACK["D"][1])):
        k = Known(tie_free_noise(h, w, h), 255, 4, 1, "none", 0.0, "free", "shipped gates %dx%d" % (h, w))
        assert k.f.pre.size == h * w
        spies.take()
        blob = pipeline.compress_band(k.band.astype(np.uint8), k.config())
        assert spies.take()[0] == forward, (h, w)
        check_compressed(blob, k, k.what)
        for fn, dtype in ((pipeline.decompress_band, np.int64), (pipeline.decompress_band_u8, np.uint8)):
            got = fn(k.blob, k.config())
            assert spies.take()[0] == back, (h, w, fn.__name__)
            check_decoded(got, k.inv, "free", k.what, dtype)


def test_refusals_at_15_bits(gpu, monkeypatch, spies):
    """A DC of exactly 16383 codes on every forward road, with the oracle's bytes; 16384, and a flat 255 band under
    'divide' 1e-4 at N = 32, raise the reference's error on every road (and on the host road of the N = 32 cell)."""
    import pipeline
    import util
    for band, n, mode, param, refused in refusal_cases():
        cfg = config_of(n, 1, mode, param, *band.shape)
        for road, (_, _, expected) in FORWARD.items():
            with forward_road(monkeypatch, road):
                spies.take()
                if refused:
                    with pytest.raises(on.BadRleCodeError):
                        on.compress_reference(band, 1, n, mode, param)
                    with pytest.raises(util.BadRleCodeError):
                        pipeline.compress_band(band, cfg)
                else:
                    f = on.Forward(band, 1, n, mode, param)
                    assert int(f.k.max()) == 16383 and f.distance >= 100 * f.tau
                    assert pipeline.compress_band(band, cfg) == f.blob(), road
                    assert spies.take()[0] == expected, road
    check_refusals(monkeypatch, [c for c in refusal_cases() if host_road_needs_a_device(c[1], c[2])])


def test_container_round_trip_at_dct_size_12(gpu, monkeypatch, spies):
    """Jpeg.compress -> Jpeg.decompress at N = 12, block_size 3 on a ragged three-band picture of 8-bit noise: the bands
    taken out of the container with file_format.read_data, each against the oracle both ways."""
    import file_format
    import pipeline
    from PIL import Image
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    h, w = 100, 136                                         # padded to 102 x 138, pooled to 34 x 46, padded to 36 x 48
    rng = np.random.default_rng(12)
    pixels = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    cfg = config_of(12, 3, "divide", 40.0, h, w)
    spies.take()
    data = pipeline.Jpeg(cfg).compress(Image.fromarray(pixels, mode="YCbCr"))
    assert spies.take()[0] == {"forward_fused_n": 3, "entropy_encode_n": 3}
    back = np.asarray(pipeline.Jpeg.decompress(data))
    assert spies.take()[0] == {"entropy_decode_n": 3, "inverse_fused_n": 3}
    assert back.shape == pixels.shape and back.dtype == np.uint8
    cfg2, bands = file_format.read_data(data)
    assert (cfg2.dct_size, cfg2.block_size, cfg2.height, cfg2.width) == (12, 3, h, w)
    for i, blob in enumerate((bands.y, bands.cb, bands.cr)):
        k = Known(pixels[:, :, i].astype(np.int64), 255, 12, 3, "divide", 40.0, "ties", "container band %d" % i)
        assert on.blocks_of(h, w, 3, 12) == (3, 4) and k.f.pre.shape == (36, 48)
        check_compressed(blob, k, k.what)
        check_decoded(np.ascontiguousarray(back[:, :, i]), k.inverse(blob), "ties", k.what, np.uint8)
