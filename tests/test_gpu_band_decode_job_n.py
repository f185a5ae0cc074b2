"""GPU: decompress_band / decompress_band_u8 for dct_size != 8 as ONE device job down to the band's samples
(jpegx.decompress_band_n: jpegx_host_decompress_band_n / _band_i64_n, the geometry steps as jpegx_inflate_crop_u8).

Against the product-free oracle of tests/codec_oracle_n.py over codec_oracle_n.matrix_cases() on the oracle's own bytes,
with spies showing that the job ran once and nothing else did (and that a divisor that is no integer keeps the parser
road); against the road of before, byte for byte, on the bands of tests/test_gpu_entropy_decode_n.py; the native entries
with a wider pitch and through their explicit-device twins; refused streams; two host threads; the gates; the container."""
import threading

import numpy as np
import pytest

import codec_oracle_n as on
from test_codec_oracle_n import case_id, check_decoded, config_of, known
from test_gpu_entropy_decode_n import BANDS, _config

pytestmark = pytest.mark.gpu

ENTRIES = ("decompress_band_n", "decompress_plane_n", "entropy_decode_n", "inverse_fused_n")
GATE = "DCTN_BAND_DECODE_JOB_MIN_SAMPLES"


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


ENTRY_FORMS = (("decompress_band", np.dtype(int), "i64"), ("decompress_band_u8", np.dtype(np.uint8), "u8"))


@pytest.mark.parametrize("case", on.matrix_cases(), ids=case_id)
def test_the_job_meets_the_oracle(gpu, monkeypatch, spies, case):
    import pipeline
    k = known(case)
    cfg = k.config()
    monkeypatch.setattr(pipeline, GATE, 0)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    whole = k.mode != "divide" or k.param == np.trunc(k.param)
    for name, dtype, out in ENTRY_FORMS:
        spies.take()
        got = getattr(pipeline, name)(k.blob, cfg)
        counts, calls = spies.take()
        what = "%s %s" % (name, k.what)
        if whole:
            assert counts == {"decompress_band_n": 1}, "the job did not run alone: %s %r" % (what, counts)
            assert calls[0][2]["out"] == out, what
            assert got.flags.c_contiguous and got.flags.writeable
        else:                                       # the job restores without the reference's truncation: it is not asked
            assert counts == {"entropy_decode_n": 1, "inverse_fused_n": 1}, (what, counts)
        check_decoded(got, k.inv, k.kind, what, dtype)


@pytest.mark.parametrize("bs,n,name,key,value,h,w", BANDS)
def test_the_job_equals_the_road_of_before(gpu, monkeypatch, spies, bs, n, name, key, value, h, w):
    import pipeline
    cfg = _config(bs, n, name, key, value, h, w)
    blob = pipeline.compress_band(np.random.default_rng(h * w + n).integers(0, 256, (h, w)), cfg)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    monkeypatch.setattr(pipeline, GATE, None)
    spies.take()
    want = [getattr(pipeline, f)(blob, cfg) for f, _, _ in ENTRY_FORMS]
    assert "decompress_band_n" not in spies.take()[0]
    monkeypatch.setattr(pipeline, GATE, 0)
    got = [getattr(pipeline, f)(blob, cfg) for f, _, _ in ENTRY_FORMS]
    counts, calls = spies.take()
    assert counts == {"decompress_band_n": 2} and [c[2]["out"] for c in calls] == ["i64", "u8"]
    for g, b, (_, dtype, _) in zip(got, want, ENTRY_FORMS):
        assert g.dtype == b.dtype == dtype and g.shape == b.shape == (h, w) and g.tobytes() == b.tobytes()
        assert g.flags.c_contiguous and g.flags.writeable
    monkeypatch.setattr(pipeline, GATE, 1 << 40)    # planes below a set gate keep the road of before
    assert pipeline.decompress_band(blob, cfg).tobytes() == want[0].tobytes() and spies.take()[0].get("decompress_band_n") is None


def _native(gpu, form, blob, rows, cols, bs, n, mode, param, out, pitch=None, device=None):
    L = gpu.lib()
    buf = np.frombuffer(blob, np.uint8)
    args = [buf.ctypes.data, buf.size, rows, cols, bs, n, gpu.mode_of(mode), float(param), out.ctypes.data]
    if form == "u8":
        args.append(pitch)
    name = "jpegx_host_decompress_band_n" if form == "u8" else "jpegx_host_decompress_band_i64_n"
    if device is not None:
        return getattr(L, name + "_on")(device, *args)
    return getattr(L, name)(*args)


@pytest.mark.parametrize("bs,n,h,w", [(1, 6, 53, 77), (5, 24, 233, 351), (3, 12, 100, 136)])
def test_native_entries_pitch_slack_and_twins(gpu, bs, n, h, w):
    import pipeline
    cfg = config_of(n, bs, "divide", 40.0, h, w)
    blob = pipeline.compress_band(np.random.default_rng(h + w).integers(0, 256, (h, w)), cfg)
    want = gpu.decompress_band_n(blob, h, w, bs, n, "divide", 40.0, out="u8")
    hh, ww = gpu.band_shape_n(h, w, bs, n)
    plane = gpu.decompress_plane_n(blob, hh, ww, n, "divide", 40.0, out="u8")
    assert np.array_equal(want, np.repeat(np.repeat(plane, bs, 0), bs, 1)[:h, :w])
    for device in (None, 0):
        out = np.full((h, w + 11), 0x5A, np.uint8)
        gpu.check(_native(gpu, "u8", blob, h, w, bs, n, "divide", 40.0, out, w + 11, device), "jpegx_host_decompress_band_n")
        assert np.array_equal(out[:, :w], want) and np.all(out[:, w:] == 0x5A), "the pitch slack was written"
        wide = np.full((h + 1, w), -77, np.int64)
        gpu.check(_native(gpu, "i64", blob, h, w, bs, n, "divide", 40.0, wide, None, device), "jpegx_host_decompress_band_i64_n")
        assert np.array_equal(wide[:h], want) and np.all(wide[h:] == -77)
    assert np.array_equal(gpu.decompress_band_n(blob, h, w, bs, n, "divide", 40.0, out="i64"), want)


@pytest.mark.parametrize("bs", [1, 3])
def test_a_damaged_blob_is_refused_alike_and_the_next_job_succeeds(gpu, monkeypatch, bs):
    import pipeline
    h, w, n = 64 * bs - (bs - 1), 48 * bs, 16
    cfg = config_of(n, bs, "divide", 40.0, h, w)
    blob = pipeline.compress_band(np.random.default_rng(3).integers(0, 256, (h, w)), cfg)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    monkeypatch.setattr(pipeline, GATE, 0)
    want = pipeline.decompress_band_u8(blob, cfg)
    for bad in (blob[:-1], blob + b"\x00", b"\x01" + blob):
        raised = []
        for setting in (None, 0):
            monkeypatch.setattr(pipeline, GATE, setting)
            for f in (pipeline.decompress_band, pipeline.decompress_band_u8):
                with pytest.raises(Exception) as exc:
                    f(bad, cfg)
                raised.append((type(exc.value), str(exc.value)))
        assert raised[0] == raised[2] and raised[1] == raised[3], raised
        out = np.full((h, w), 0x5A, np.uint8)
        assert _native(gpu, "u8", bad, h, w, bs, n, "divide", 40.0, out, w) == -1 and np.all(out == 0x5A), "a refused stream wrote the caller's samples"
        wide = np.full((h, w), 0x5A5A, np.int64)
        assert _native(gpu, "i64", bad, h, w, bs, n, "divide", 40.0, wide) == -1 and np.all(wide == 0x5A5A)
        with pytest.raises(gpu.JpegxError):
            gpu.decompress_band_n(bad, h, w, bs, n, "divide", 40.0)
        assert np.array_equal(gpu.decompress_band_n(blob, h, w, bs, n, "divide", 40.0), want)      # the next job succeeds
    monkeypatch.setattr(pipeline, GATE, 0)
    assert np.array_equal(pipeline.decompress_band(blob, cfg), want)


def test_two_host_threads_get_their_own_bands(gpu):
    import pipeline
    jobs = []
    for seed, (bs, n, h, w) in enumerate(((5, 24, 233, 351), (1, 4, 250, 333))):
        cfg = config_of(n, bs, "divide", 40.0, h, w)
        blob = pipeline.compress_band(np.random.default_rng(seed).integers(0, 256, (h, w)), cfg)
        jobs.append((blob, h, w, bs, n, gpu.decompress_band_n(blob, h, w, bs, n, "divide", 40.0)))
    failures = []

    def work(blob, h, w, bs, n, want):
        try:
            for i in range(6):
                got = gpu.decompress_band_n(blob, h, w, bs, n, "divide", 40.0, out="i64" if i % 2 else "u8")
                if not np.array_equal(got, want):
                    failures.append((bs, n, i))
        except Exception as exc:                    # pragma: no cover
            failures.append(repr(exc))
    threads = [threading.Thread(target=work, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert failures == []


def test_a_registry_that_is_not_stock_never_reaches_the_job(gpu, monkeypatch, spies):
    import pipeline
    from pipeline.base import AlgorithmStep, step_classes
    cfg = config_of(4, 1, "divide", 40.0, 64, 96)
    blob = pipeline.compress_band(np.random.default_rng(9).integers(0, 256, (64, 96)), cfg)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    monkeypatch.setattr(pipeline, GATE, 0)
    want = pipeline.decompress_band(blob, cfg)
    assert spies.take()[0] == {"decompress_band_n": 1}
    stock = list(step_classes)
    try:
        class PassThrough(AlgorithmStep):
            step_index = 9.5

            def execute(self, array):
                return array

            def invert(self, array):
                return array
        assert not pipeline._stock_registry()
        assert np.array_equal(pipeline.decompress_band(blob, cfg), want)
        assert np.array_equal(pipeline.decompress_band_u8(blob, cfg), want)
        assert "decompress_band_n" not in spies.take()[0]
    finally:
        step_classes[:] = stock


def test_the_gates_as_shipped(gpu, monkeypatch, spies):
    """The four older constants as committed; the new gate above 262 144 (planes of exactly that size are pinned to
    jpegx.decompress_plane_n by two older tests).  A block_size 1, N = 4 plane of exactly the gate's samples takes the job, one
    block row fewer takes jpegx.decompress_plane_n (None as shipped: the same at the smallest size that could ship)."""
    import pipeline
    assert (pipeline.DCTN_MIN_SAMPLES, pipeline.DCTN_ENTROPY_MIN_SAMPLES, pipeline.DCTN_ENTROPY_DECODE_MIN_SAMPLES,
            pipeline.DCTN_BAND_JOB_MIN_SAMPLES) == (1024, None, 262144, 16384)
    gate = getattr(pipeline, GATE)
    assert gate is None or gate > 262144
    if gate is None:
        gate = 576 * 576
        monkeypatch.setattr(pipeline, GATE, gate)
    w = next(v for v in (512, 576, 768) if gate % (4 * v) == 0)
    assert (gate // w - 4) * w >= 262144
    for h, used in ((gate // w, "decompress_band_n"), (gate // w - 4, "decompress_plane_n")):
        cfg = config_of(4, 1, "divide", 40.0, h, w)
        blob = pipeline.compress_band(np.random.default_rng(h).integers(0, 256, (h, w)).astype(np.uint8), cfg)
        spies.take()
        got, got_u8 = pipeline.decompress_band(blob, cfg), pipeline.decompress_band_u8(blob, cfg)
        assert spies.take()[0] == {used: 2}, (h, used)
        with monkeypatch.context() as m:
            m.setattr(pipeline, GATE, None)
            m.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", None)
            assert got.tobytes() == pipeline.decompress_band(blob, cfg).tobytes()
            assert got_u8.tobytes() == pipeline.decompress_band_u8(blob, cfg).tobytes()


def test_container_at_dct_size_12(gpu, monkeypatch, spies):
    """Jpeg.decompress on a ragged three-band picture at N = 12, block_size 3: three band jobs, the picture of before."""
    import pipeline
    from PIL import Image
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    h, w = 100, 136
    pixels = np.random.default_rng(12).integers(0, 256, (h, w, 3)).astype(np.uint8)
    data = pipeline.Jpeg(config_of(12, 3, "divide", 40.0, h, w)).compress(Image.fromarray(pixels, mode="YCbCr"))
    monkeypatch.setattr(pipeline, GATE, None)
    spies.take()
    want = np.asarray(pipeline.Jpeg.decompress(data))
    assert "decompress_band_n" not in spies.take()[0]
    monkeypatch.setattr(pipeline, GATE, 0)
    got = np.asarray(pipeline.Jpeg.decompress(data))
    counts, calls = spies.take()
    assert counts == {"decompress_band_n": 3} and all(c[2]["out"] == "u8" for c in calls)
    assert got.shape == (h, w, 3) and got.dtype == np.uint8 and np.array_equal(got, want)
