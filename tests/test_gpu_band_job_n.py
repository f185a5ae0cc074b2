"""compress_band for dct_size != 8 as one device job from the band's 8-bit samples (jpegx.compress_band_n behind
pipeline.DCTN_BAND_JOB_MIN_SAMPLES) against the roads of before, byte for byte: the same call with the gate at None
(NumPy steps 0-3, float64 upload, forward kernel, host coder) and, once per case, with the device switched off altogether
(the reference's host steps).  Dtypes, a strided view, every refusal, two host threads, and the gate itself."""
import threading

import numpy as np
import pytest

from test_gpu_entropy_n import BANDS

pytestmark = pytest.mark.gpu

HOST_ONLY = 1 << 62
CASES = BANDS + [(1, 4, "none", None, None, 53, 77), (3, 5, "divide", "divisor", 40, 31, 43)]


def _config(bs, n, name, key, value, h, w):
    import pipeline
    q = pipeline.QuantizationMethod(name, **({key: value} if key else {}))
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n, quantization=q)


@pytest.fixture
def counted(gpu, monkeypatch):
    """The gate at 0 (every plane that may take the band job takes it) and a list that grows with every job.  The smallest
    cases (15 x 15 samples enter step 4 of the 31 x 43 band at block_size 3, dct_size 5) lie below pipeline.DCTN_MIN_SAMPLES,
    under which no device road is taken at all: that gate is opened too, for the band job and for the road it is compared
    with alike."""
    import pipeline
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    calls = []
    real = gpu.compress_band_n
    monkeypatch.setattr(gpu, "compress_band_n", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(pipeline, "DCTN_BAND_JOB_MIN_SAMPLES", 0)
    return calls


def _roads_of_before(monkeypatch, band, cfg, host_too=True):
    """compress_band with the band job off, and with the device off."""
    import pipeline
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_BAND_JOB_MIN_SAMPLES", None)
        parent = pipeline.compress_band(band, cfg)
        host = None
        if host_too:
            m.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
            host = pipeline.compress_band(band, cfg)
    return parent, host


@pytest.mark.parametrize("bs,n,name,key,value,h,w", CASES)
def test_bytes_equal_the_road_of_before(gpu, monkeypatch, counted, bs, n, name, key, value, h, w):
    """Against compress_band with the gate at None: every dtype the job takes, a strided view and a view it must copy."""
    import pipeline
    cfg = _config(bs, n, name, key, value, h, w)
    band = np.random.default_rng(h * w + n).integers(0, 256, (h, w))
    parent, _ = _roads_of_before(monkeypatch, band, cfg, host_too=False)
    assert not counted and isinstance(parent, bytes)
    for k, dtype in enumerate((np.uint8, np.int32, np.int64)):
        got = pipeline.compress_band(band.astype(dtype), cfg)
        assert len(counted) == k + 1, "the band job was not used for %s" % np.dtype(dtype)
        assert isinstance(got, bytes) and got == parent, np.dtype(dtype)
    # rows a fixed distance apart (the entry's pitch), and a view that is not: every second column
    wide = np.zeros((h, w + 5), np.uint8)
    wide[:, :w] = band
    assert pipeline.compress_band(wide[:, :w], cfg) == parent and len(counted) == 4
    twice = np.repeat(band.astype(np.int32), 2, axis=1)
    assert pipeline.compress_band(twice[:, ::2], cfg) == parent and len(counted) == 5


def _band_off_the_ties(h, w, n):
    """An 8-bit band for quantiser 'none' at dct_size 4 whose stream is the same in every summation order.

    The device kernels and NumPy sum the transform's dot products in different orders, so the two roads agree only up to
    the criterion of DESIGN.md 4.7 (tests/dctn_criterion.py): a coefficient within tau = 7.2e-12 of m + 1/2 may round to
    either neighbour, and seeded noise puts 2.75 % of this case's coefficients there (23 of 4480 then differ by one
    between the device road and the NumPy road, the band job not involved).  A byte comparison across those two roads
    therefore needs a band without such coefficients, like flat_tiles_band in tests/test_gpu_dctn_adversarial.py.  At N = 4
    the matrix entries are 1, +-sqrt(1/2), +-c1 and +-c3 with c1^2 = (2 + sqrt 2) / 4, c3^2 = (2 - sqrt 2) / 4,
    c1 c3 = sqrt(2) / 4, so a coefficient is (a + b sqrt 2) / 4 with a, b integer combinations of the samples, or an
    irrational multiple of such a number; it is m + 1/2 only for b = 0 and a = 2 mod 4.  With every sample a multiple of 4
    a is a multiple of 4: the rational coefficients are integers, the others stay off the half-integers.  The caller
    asserts that on the reference's own values before rounding."""
    return (np.random.default_rng(h * w + n).integers(0, 64, (h, w)) * 4).astype(np.int64)


def _distance_from_a_tie(band, cfg):
    """Smallest | v - (m + 1/2) | over the reference's float64 coefficients v of the band (host steps 0-3, then the
    reference's transform block by block): nothing of the code under test."""
    import dctn_criterion as crit
    from pipeline import dct_padding, padding, subsampling
    plane = band
    for cls in (padding.Padding, subsampling.SubSampling, dct_padding.DCTPadding):
        plane = cls(cfg).execute(plane)
    v = crit.ref_dct(np.asarray(plane, dtype=np.float64), cfg.dct_size)
    return float(np.abs(v - np.floor(v) - 0.5).min())


@pytest.mark.parametrize("bs,n,name,key,value,h,w", CASES)
def test_bytes_equal_the_all_numpy_road(gpu, monkeypatch, counted, bs, n, name, key, value, h, w):
    """Once per case against the road with the device switched off (DCTN_MIN_SAMPLES = HOST_ONLY): the reference's steps in
    NumPy.  The case under 'none' runs on a band whose coefficients keep 1e-6 and more from every rounding tie
    (_band_off_the_ties; tau of the criterion is 7.2e-12 there); the noise band of that case is compared with the device
    road in test_bytes_equal_the_road_of_before."""
    import pipeline
    cfg = _config(bs, n, name, key, value, h, w)
    if name == "none":
        assert (bs, n) == (1, 4)
        band = _band_off_the_ties(h, w, n)
        assert band.max() > 200 and _distance_from_a_tie(band, cfg) > 1e-6
    else:
        band = np.random.default_rng(h * w + n).integers(0, 256, (h, w))
    _, host = _roads_of_before(monkeypatch, band, cfg)
    got = pipeline.compress_band(band, cfg)
    assert len(counted) == 1
    assert isinstance(got, bytes) and got == host
    assert np.array_equal(pipeline.decompress_band(got, cfg), pipeline.decompress_band(host, cfg))


def test_the_native_entry_with_a_pitch_and_its_device_twin(gpu):
    import ctypes
    band = np.random.default_rng(11).integers(0, 256, (31, 60)).astype(np.int64)
    want = gpu.compress_band_n(np.ascontiguousarray(band[:, :43]), 3, 5, "divide", 40.0)
    assert isinstance(want, bytes) and len(want)
    L = gpu.lib()
    for entry, args in ((L.jpegx_host_compress_begin_band_n, ()), (L.jpegx_host_compress_begin_band_n_on, (0,))):
        n = ctypes.c_size_t(0)
        gpu.check(entry(*args, band.ctypes.data, 8, 31, 43, 60, 3, 5, gpu.Q_DIVIDE, 40.0, ctypes.byref(n)), "begin_band_n")
        out = np.empty(n.value, np.uint8)
        gpu.check(L.jpegx_host_compress_finish(out.ctypes.data), "finish")
        assert out.tobytes() == want


def test_a_band_beyond_8_bits_keeps_the_road_of_before(gpu, monkeypatch, counted):
    import pipeline
    cfg = _config(1, 16, "divide", "divisor", 40, 64, 48)
    for bad in (256, -1):
        band = np.random.default_rng(3).integers(0, 256, (64, 48))
        band[40, 17] = bad
        parent, _ = _roads_of_before(monkeypatch, band, cfg, host_too=False)
        before = len(counted)
        assert pipeline.compress_band(band, cfg) == parent
        assert len(counted) == before + 1                      # asked, answered None ("not an 8-bit band"), nothing left open
        assert gpu.compress_band_n(band, 1, 16, "divide", 40.0) is None
        assert gpu.lib().jpegx_host_compress_finish(None) == -1


def test_what_never_reaches_the_band_job(gpu, monkeypatch, counted):
    import pipeline
    from pipeline.base import AlgorithmStep, step_classes
    cfg = _config(1, 16, "divide", "divisor", 40, 64, 48)
    band = np.random.default_rng(7).integers(0, 256, (64, 48))
    want = pipeline.compress_band(band, cfg)
    assert len(counted) == 1
    assert pipeline.compress_band(band.astype(np.float64), cfg) == want and len(counted) == 1      # a float band
    with monkeypatch.context() as m:                            # the device road off altogether
        m.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
        assert pipeline.compress_band(band, cfg) == want and len(counted) == 1
    with monkeypatch.context() as m:                            # a gate nothing reaches
        m.setattr(pipeline, "DCTN_BAND_JOB_MIN_SAMPLES", 1 << 40)
        assert pipeline.compress_band(band, cfg) == want and len(counted) == 1
    stock = list(step_classes)
    try:
        class Nothing(AlgorithmStep):
            step_index = 9.5

            def execute(self, array):
                return array

            def invert(self, array):
                return array
        assert not pipeline._stock_registry()
        assert pipeline.compress_band(band, cfg) == want and len(counted) == 1
    finally:
        step_classes[:] = stock
    assert pipeline.compress_band(band, cfg) == want and len(counted) == 2


def test_a_set_entropy_gate_keeps_compress_plane_n(gpu, monkeypatch, counted):
    import pipeline
    cfg = _config(1, 16, "divide", "divisor", 40, 64, 48)
    band = np.random.default_rng(7).integers(0, 256, (64, 48))
    plane_jobs = []
    real = gpu.compress_plane_n
    monkeypatch.setattr(gpu, "compress_plane_n", lambda *a, **k: (plane_jobs.append(1), real(*a, **k))[1])
    want = pipeline.compress_band(band, cfg)
    assert len(counted) == 1 and not plane_jobs
    monkeypatch.setattr(pipeline, "DCTN_ENTROPY_MIN_SAMPLES", 0)
    assert pipeline.compress_band(band, cfg) == want
    assert len(counted) == 1 and plane_jobs == [1]
    monkeypatch.setattr(pipeline, "DCTN_ENTROPY_MIN_SAMPLES", 64 * 48 + 1)      # a plane that gate does not admit
    assert pipeline.compress_band(band, cfg) == want
    assert len(counted) == 2 and plane_jobs == [1]


def test_beyond_15_bits_raises_the_references_error(gpu, monkeypatch, counted):
    import pipeline
    import util
    cfg = _config(1, 32, "none", None, None, 64, 96)
    band = np.full((64, 96), 255)                               # DC 255 * 32 * 32 = 261 120 under 'none'
    with pytest.raises(util.BadRleCodeError) as dev:            # the job refuses, the road of before raises
        pipeline.compress_band(band, cfg)
    assert len(counted) == 1
    with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
        gpu.compress_band_n(band, 1, 32, "none", 0.0)
    assert gpu.lib().jpegx_host_compress_finish(None) == -1      # the context was given back: no job is open
    ok = _config(1, 32, "divide", "divisor", 1000, 64, 96)
    blob = pipeline.compress_band(band, ok)                     # the next job on this thread succeeds
    assert isinstance(blob, bytes) and len(counted) == 3
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
        with pytest.raises(util.BadRleCodeError) as host:
            pipeline.compress_band(band, cfg)
        assert pipeline.compress_band(band, ok) == blob
    assert str(dev.value) == str(host.value)


def test_a_coefficient_that_could_leave_int32_keeps_the_road_of_before(gpu, monkeypatch, counted):
    """255 * N^2 / min(|d|, 1) beyond 2^31 - 1: the band job is not asked."""
    import pipeline
    cfg = _config(1, 32, "divide", "divisor", 1e-4, 64, 96)     # 255 * 1024 / 1e-4 = 2.6e9; this band's own DC is 10 000
    band = np.zeros((64, 96), np.uint8)
    band[0, 0] = 1
    parent, _ = _roads_of_before(monkeypatch, band, cfg, host_too=False)
    assert pipeline.compress_band(band, cfg) == parent and not counted


def test_two_host_threads_get_their_own_bytes(gpu, monkeypatch, counted):
    import pipeline
    cfgs = [_config(3, 5, "divide", "divisor", 40, 31, 43), _config(1, 16, "divide", "divisor", 40, 53, 77)]
    bands = [np.random.default_rng(k).integers(0, 256, (c.height, c.width)).astype(np.uint8) for k, c in enumerate(cfgs)]
    want = [_roads_of_before(monkeypatch, b, c, host_too=False)[0] for b, c in zip(bands, cfgs)]
    wrong, start = [], threading.Barrier(2)

    def work(k):
        try:
            start.wait()
            for _ in range(20):
                if pipeline.compress_band(bands[k], cfgs[k]) != want[k]:
                    wrong.append(k)
        except BaseException as exc:                            # noqa: BLE001  (reported by the assertion below)
            wrong.append(exc)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not wrong and len(counted) == 40


def _plane_of_exactly(samples):
    """(n, H, W) with H * W == samples, both whole n x n blocks, H >= 2 n -- or None."""
    for n in (4, 2, 16, 3, 5, 6, 7):
        for w in range(n, int(samples ** 0.5) + 1, n):
            h = samples // w
            if h * w == samples and h % n == 0 and h >= 2 * n:
                return n, h, w
    return None


def test_the_gate_as_shipped(gpu, monkeypatch):
    """A plane of exactly DCTN_BAND_JOB_MIN_SAMPLES samples takes the job, one block row fewer does not."""
    import pipeline
    gate = pipeline.DCTN_BAND_JOB_MIN_SAMPLES
    if gate is None:
        return                                                  # shipped switched off: nothing takes the job (checked below)
    shape = _plane_of_exactly(gate)
    assert shape is not None, "no plane of whole blocks holds exactly %d samples" % gate
    n, h, w = shape
    calls = []
    real = gpu.compress_band_n
    monkeypatch.setattr(gpu, "compress_band_n", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for rows, takes in ((h, True), (h - n + 1, True), (h - n, False)):      # h - n + 1 rows are padded back to h
        cfg = _config(1, n, "divide", "divisor", 40, rows, w)
        band = np.random.default_rng(rows).integers(0, 256, (rows, w)).astype(np.uint8)
        del calls[:]
        got = pipeline.compress_band(band, cfg)
        assert bool(calls) == takes, (rows, w, n)
        with monkeypatch.context() as m:
            m.setattr(pipeline, "DCTN_BAND_JOB_MIN_SAMPLES", None)
            assert pipeline.compress_band(band, cfg) == got


def test_switched_off_nothing_takes_the_job(gpu, monkeypatch):
    import pipeline

    def boom(*a, **k):
        raise AssertionError("compress_band took the band job")
    monkeypatch.setattr(gpu, "compress_band_n", boom)
    monkeypatch.setattr(pipeline, "DCTN_BAND_JOB_MIN_SAMPLES", None)
    cfg = _config(1, 16, "divide", "divisor", 40, 64, 48)
    assert isinstance(pipeline.compress_band(np.random.default_rng(3).integers(0, 256, (64, 48)), cfg), bytes)
