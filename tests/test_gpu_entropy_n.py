"""The run-time block length entropy stage on the device (csrc/jpegx_entropy_n.hip) against the host coder
jpegx.entropy_encode_n, byte for byte: the streams of adversarial_rle_n.py at every block length N^2 for N = 2..32 plus
1, 63, 64, 65 and 1000, at block counts that reach one block, a partly filled last wave and the crossing of a 64-block
scan group; output buffers at odd addresses between guard bytes; the pooled band job jpegx.compress_plane_n; and the
pipeline's compress_band against the same call with the device road switched off."""
import ctypes

import numpy as np
import pytest

import adversarial_rle_n as adv

pytestmark = pytest.mark.gpu

LENGTHS = sorted(set([n * n for n in range(2, 33)] + [1, 63, 64, 65, 1000]))
GUARD = 64
OFFSETS = (0, 1, 7, 15)


def counts_of(block_len):
    if block_len > 64:
        return (1, 3, 67)                       # a wave per block: one group, and across a group's end
    per = 64 // block_len                       # blocks per wave
    return (1, per + max(1, per // 2), 65, 130)


class Coder:
    """One stream on the device: sizes once, then as many emits as wanted."""

    def __init__(self, gpu, zz, block_len, ws=None, stream=None, device=None):
        self.g, self.L = gpu, gpu.lib()
        self.zz = np.ascontiguousarray(zz, dtype=np.int32)
        self.block_len, self.nblocks = block_len, self.zz.size // block_len
        self.stream, self.device = stream, device
        self.dzz = gpu.DeviceBuffer(self.zz.nbytes)
        self.own_ws = ws is None
        self.dws = ws if ws is not None else gpu.DeviceBuffer(self.L.jpegx_entropy_workspace_bytes_n(self.nblocks, block_len))
        self.dzz.upload(self.zz)
        if device is None:
            rc = self.L.jpegx_entropy_sizes_n(self.dzz.ptr, self.nblocks, block_len, self.dws.ptr, stream)
        else:
            rc = self.L.jpegx_entropy_sizes_n_on(device, self.dzz.ptr, self.nblocks, block_len, self.dws.ptr, stream)
        gpu.check(rc, "jpegx_entropy_sizes_n")

    def total_rc(self):
        total = ctypes.c_ulonglong(0)
        rc = self.L.jpegx_entropy_total(self.dws.ptr, ctypes.byref(total), self.stream)
        return rc, total.value

    def block_sizes(self):
        out = np.empty(self.nblocks, np.uint32)
        self.g.check(self.L.jpegx_entropy_block_sizes(self.dws.ptr, self.nblocks, out.ctypes.data, self.stream), "jpegx_entropy_block_sizes")
        return out

    def emit(self, total, offset=0):
        """The whole output buffer after the emit: [16 + GUARD + total + GUARD] bytes pre-filled with 0xA5, the stream
        starting `offset` bytes behind a 16-byte boundary; returns (front guard, bytes, back guard)."""
        size = 16 + GUARD + total + GUARD + 16
        dout = self.g.DeviceBuffer(size)
        try:
            assert dout.ptr % 16 == 0
            dout.upload(np.full(size, 0xA5, np.uint8))
            at = 64 + offset                    # GUARD = 64 is a multiple of 16: the start is `offset` behind a boundary
            if self.device is None:
                rc = self.L.jpegx_entropy_emit_n(self.dzz.ptr, self.nblocks, self.block_len, self.dws.ptr, dout.ptr + at, self.stream)
            else:
                rc = self.L.jpegx_entropy_emit_n_on(self.device, self.dzz.ptr, self.nblocks, self.block_len, self.dws.ptr, dout.ptr + at, self.stream)
            self.g.check(rc, "jpegx_entropy_emit_n")
            self.g.check(self.L.jpegx_stream_synchronize(self.stream), "jpegx_stream_synchronize")
            buf = dout.download((size,), np.uint8)
            return buf[:at], buf[at:at + total].tobytes(), buf[at + total:]
        finally:
            dout.free()

    def free(self):
        self.dzz.free()
        if self.own_ws:
            self.dws.free()


@pytest.mark.parametrize("block_len", LENGTHS)
def test_every_class_byte_for_byte(gpu, block_len):
    for nblocks in counts_of(block_len):
        for cls in adv.CLASSES:
            want, want_sizes = adv.host_bytes(cls, block_len, nblocks)
            c = Coder(gpu, adv.build(cls, block_len, nblocks), block_len)
            try:
                rc, total = c.total_rc()
                where = "%s, %d blocks of %d" % (cls, nblocks, block_len)
                assert rc == 0 and total == len(want), where
                assert np.array_equal(c.block_sizes(), want_sizes), where
                for offset in OFFSETS:
                    front, got, back = c.emit(total, offset)
                    assert got == want, "%s, offset %d" % (where, offset)
                    assert np.all(front == 0xA5) and np.all(back == 0xA5), "%s, offset %d: guard bytes written" % (where, offset)
            finally:
                c.free()


@pytest.mark.parametrize("block_len", [1, 9, 64, 65, 576, 1024])
def test_bad_amplitude_is_refused_and_nothing_is_written(gpu, block_len):
    nblocks = 130 if block_len <= 64 else 67
    for value in (16384, -16384):
        c = Coder(gpu, adv.bad(value, block_len, nblocks), block_len)
        try:
            rc, _ = c.total_rc()
            assert rc == -1 and b"BadRleCodeError" in gpu.lib().jpegx_last_error()
            front, got, back = c.emit(4096, 3)
            assert np.all(front == 0xA5) and got == bytes([0xA5]) * 4096 and np.all(back == 0xA5)
        finally:
            c.free()
        with pytest.raises(gpu.JpegxError, match="BadRleCodeError") as dev:
            gpu.entropy_encode_n_gpu(adv.bad(value, block_len, nblocks))
        with pytest.raises(gpu.JpegxError, match="BadRleCodeError") as host:
            gpu.entropy_encode_n(adv.bad(value, block_len, nblocks))
        # the library's text is the same; in front of it stands the entry that failed
        assert str(dev.value).split(": ", 1)[1] == str(host.value).split(": ", 1)[1]
    ok = adv.bad(-16383, block_len, nblocks)                     # the legal control
    assert gpu.entropy_encode_n_gpu(ok) == gpu.entropy_encode_n(ok)


def test_block_len_64_gives_the_bytes_of_the_int16_stage(gpu):
    for cls in ("mixed", "runs", "widths"):
        z = adv.build(cls, 64, 130)
        assert np.abs(z).max() <= 32767
        assert gpu.entropy_encode_n_gpu(z) == gpu.entropy_encode(z.astype(np.int16))


def test_explicit_device_twins_and_a_stream(gpu):
    z = adv.build("mixed", 576, 67)
    want = gpu.entropy_encode_n(z)
    st = ctypes.c_void_p()
    gpu.check(gpu.lib().jpegx_stream_create(ctypes.byref(st)), "jpegx_stream_create")
    try:
        for kwargs in ({"device": 0}, {"stream": st}, {"device": 0, "stream": st}):
            c = Coder(gpu, z, 576, **kwargs)
            try:
                rc, total = c.total_rc()
                assert rc == 0 and total == len(want)
                front, got, back = c.emit(total, 5)
                assert got == want and np.all(front == 0xA5) and np.all(back == 0xA5)
            finally:
                c.free()
    finally:
        gpu.check(gpu.lib().jpegx_stream_destroy(st), "jpegx_stream_destroy")


def test_a_workspace_is_reused_as_it_is(gpu):
    """Back to back on one workspace: a bad stream, then good ones of other shapes -- no flag, size or offset of an earlier
    call shows in a later one."""
    L = gpu.lib()
    ws = gpu.DeviceBuffer(max(L.jpegx_entropy_workspace_bytes_n(130, 16), L.jpegx_entropy_workspace_bytes_n(67, 1000)))
    try:
        for z, block_len, good in [(adv.bad(16384, 16, 130), 16, False), (adv.build("mixed", 16, 130), 16, True),
                                   (adv.build("dense_max", 1000, 67), 1000, True), (adv.build("zeros", 16, 65), 16, True),
                                   (adv.build("mixed", 1000, 3), 1000, True)]:
            c = Coder(gpu, z, block_len, ws=ws)
            try:
                rc, total = c.total_rc()
                if not good:
                    assert rc == -1
                    continue
                want = gpu.entropy_encode_n(z)
                assert rc == 0 and total == len(want)
                assert c.emit(total, 9)[1] == want
            finally:
                c.free()
    finally:
        ws.free()


# ---- the pooled band job --------------------------------------------------------------------------------------------
JOB_SHAPES = [(3, 39, 201), (5, 35, 45), (16, 48, 32), (24, 48, 72), (32, 64, 96)]
JOB_QUANTISERS = [("none", 0.0), ("discard", 2.0), ("divide", 40.0)]


@pytest.mark.parametrize("n,h,w", JOB_SHAPES)
def test_compress_plane_n(gpu, n, h, w):
    rng = np.random.default_rng(n * 100000 + h * 1000 + w)
    y, x = np.mgrid[0:h, 0:w]
    # small samples: quantiser 'none' stays within 15 bits (a DC is the sum of N * N samples)
    planes = [rng.integers(-3, 4, (h, w)).astype(np.float64), ((3 * x + 5 * y) % 16).astype(np.float64) - 7.5,
              rng.integers(0, 256, (h, w)).astype(np.float64) - 128.0]
    for plane in planes:
        for mode, param in JOB_QUANTISERS:
            zz = gpu.forward_fused_n(plane, n, mode, param)
            if np.abs(zz).max() > 16383:
                with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
                    gpu.compress_plane_n(plane, n, mode, param)
                continue
            got = gpu.compress_plane_n(plane, n, mode, param)
            assert isinstance(got, bytes) and got == gpu.entropy_encode_n(zz, n * n), (n, h, w, mode)


def test_compress_plane_n_refuses_a_bad_amplitude_and_gives_the_context_back(gpu):
    plane = np.full((64, 96), 255.0)                            # DC 255 * 32 * 32 = 261 120 under 'none'
    assert np.abs(gpu.forward_fused_n(plane, 32, "none", 0.0)).max() == 261120
    with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
        gpu.compress_plane_n(plane, 32, "none", 0.0)
    assert gpu.lib().jpegx_host_compress_finish(None) == -1      # no job is open
    small = np.full((64, 96), 3.0)
    assert gpu.compress_plane_n(small, 32, "none", 0.0) == gpu.entropy_encode_n(gpu.forward_fused_n(small, 32, "none", 0.0))


# ---- the pipeline ---------------------------------------------------------------------------------------------------
# (block_size, dct_size, quantiser, parameter name, value, height, width)
BANDS = [(5, 24, "divide", "divisor", 1000, 240, 360),          # the reference README's configuration
         (2, 3, "divide", "divisor", 40, 96, 120),
         (1, 16, "divide", "divisor", 40, 64, 48),
         (1, 16, "divide", "divisor", 40, 53, 77)]              # ragged: Padding and DCTPadding on the host first


def _config(bs, n, name, key, value, h, w):
    import pipeline
    q = pipeline.QuantizationMethod(name, **({key: value} if key else {}))
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n, quantization=q)


@pytest.mark.parametrize("bs,n,name,key,value,h,w", BANDS)
def test_compress_band_gives_the_bytes_of_the_host_coder_road(gpu, monkeypatch, bs, n, name, key, value, h, w):
    import pipeline
    cfg = _config(bs, n, name, key, value, h, w)
    band = np.random.default_rng(h * w + n).integers(0, 256, (h, w))
    calls = []
    real = gpu.compress_plane_n
    monkeypatch.setattr(gpu, "compress_plane_n", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_ENTROPY_MIN_SAMPLES", 0)      # the job road on for every plane
        got = pipeline.compress_band(band, cfg)
    assert calls == [1], "the device job was not used"
    back = pipeline.decompress_band(got, cfg)
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_MIN_SAMPLES", 1 << 62)        # the device road off: the reference's host steps
        want = pipeline.compress_band(band, cfg)
        want_back = pipeline.decompress_band(want, cfg)
    assert isinstance(got, bytes) and got == want
    assert np.array_equal(back, want_back)
    with monkeypatch.context() as m:                             # and against the other device road: forward kernel + host coder
        m.setattr(pipeline, "DCTN_ENTROPY_MIN_SAMPLES", None)
        assert pipeline.compress_band(band, cfg) == got and calls == [1]


def test_a_non_stock_registry_keeps_its_road(gpu, monkeypatch):
    import pipeline
    from pipeline.base import AlgorithmStep, step_classes
    cfg = _config(1, 16, "divide", "divisor", 40, 64, 48)
    band = np.random.default_rng(7).integers(0, 256, (64, 48))
    monkeypatch.setattr(pipeline, "DCTN_ENTROPY_MIN_SAMPLES", 0)
    want = pipeline.compress_band(band, cfg)
    calls = []
    real = gpu.compress_plane_n
    monkeypatch.setattr(gpu, "compress_plane_n", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    stock = list(step_classes)
    try:
        class Nothing(AlgorithmStep):
            step_index = 9.5

            def execute(self, array):
                return array

            def invert(self, array):
                return array
        assert not pipeline._stock_registry()
        assert pipeline.compress_band(band, cfg) == want and not calls
    finally:
        step_classes[:] = stock


def test_compress_band_beyond_15_bits_raises_the_references_error(gpu, monkeypatch):
    import pipeline
    import util
    cfg = _config(1, 32, "none", None, None, 64, 96)
    band = np.full((64, 96), 1000)                              # a DC far beyond 15 bits
    calls = []
    real = gpu.compress_plane_n
    monkeypatch.setattr(gpu, "compress_plane_n", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_ENTROPY_MIN_SAMPLES", 0)
        with pytest.raises(util.BadRleCodeError) as dev:        # the job refuses, the road of before raises
            pipeline.compress_band(band, cfg)
        assert calls == [1]
        ok = _config(1, 32, "divide", "divisor", 1000, 64, 96)
        assert isinstance(pipeline.compress_band(band, ok), bytes) and calls == [1, 1]     # the next job on this thread succeeds
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_MIN_SAMPLES", 1 << 62)
        with pytest.raises(util.BadRleCodeError) as host:
            pipeline.compress_band(band, cfg)
    assert str(dev.value) == str(host.value)


def test_the_job_road_is_off_by_default(gpu, monkeypatch):
    import pipeline
    assert pipeline.DCTN_ENTROPY_MIN_SAMPLES is None

    def boom(*a, **k):
        raise AssertionError("compress_band took the device job")
    monkeypatch.setattr(gpu, "compress_plane_n", boom)
    cfg = _config(1, 16, "divide", "divisor", 40, 64, 48)
    assert isinstance(pipeline.compress_band(np.random.default_rng(3).integers(0, 256, (64, 48)), cfg), bytes)
