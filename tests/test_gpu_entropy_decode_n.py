"""The run-time block length entropy DECODER on the device (csrc/jpegx_entropy_decode_n.hip) against the host parser
jpegx.entropy_decode_n, exactly: the streams of adversarial_rle_n.py at every block length N^2 for N = 2..32 plus 1, 63,
64, 65 and 1000 at block counts around one decode workgroup and across the chain rounds' powers of two; caller buffers at
every dword offset between guard bytes, a reused workspace, a stream and the explicit-device forms; the streams of
adversarial_decode_n.py; the refusal parity fuzz of decode_n_model.py; the pooled job jpegx.decompress_plane_n; and the
pipeline's decompress_band / decompress_band_u8 with the job road on against the same calls with it off."""
import ctypes

import numpy as np
import pytest

import adversarial_decode_n as advd
import adversarial_rle_n as adv
import decode_n_model as model

pytestmark = pytest.mark.gpu

LENGTHS = sorted(set([n * n for n in range(2, 33)] + [1, 63, 64, 65, 1000]))
GUARD = 64


def bpw_of(block_len):
    """Blocks per workgroup of the decode kernel: a 32 KiB tile of int32, at most one block per lane."""
    return min(64, 8192 // block_len)


def counts_of(block_len):
    return sorted(set((1, 2, 3, bpw_of(block_len) + 1, 67, 130)))


@pytest.mark.parametrize("block_len", LENGTHS)
def test_every_class_round_trips(gpu, block_len):
    for nblocks in counts_of(block_len):
        for cls in adv.CLASSES:
            z = adv.build(cls, block_len, nblocks)
            got = gpu.entropy_decode_n_gpu(gpu.entropy_encode_n(z), nblocks, block_len)
            assert got.dtype == np.int32 and np.array_equal(got, z), "%s, %d blocks of %d" % (cls, nblocks, block_len)


@pytest.mark.parametrize("block_len,nblocks", [(16, 5000), (1024, 300)])
def test_long_streams(gpu, block_len, nblocks):
    """Chain rounds beyond 2^12 blocks; the long walk of 1024-coefficient blocks over many workgroups."""
    z = adv.build("mixed", block_len, nblocks)
    assert np.array_equal(gpu.entropy_decode_n_gpu(gpu.entropy_encode_n(z), nblocks, block_len), z)


class Caller:
    """The device entries on buffers of the test's own: the stream with 16 zero bytes behind it, a workspace, and the
    coefficients `offset` bytes behind a 16-byte boundary between guard regions of 0xA5."""

    def __init__(self, gpu, ws_bytes):
        self.g, self.L = gpu, gpu.lib()
        self.dws = gpu.DeviceBuffer(ws_bytes)

    def decode(self, blob, nblocks, block_len, offset=0, stream=None, device=None):
        g, L = self.g, self.L
        nbytes = len(blob)
        assert L.jpegx_entropy_decode_workspace_bytes_n(nbytes, nblocks, block_len) <= self.dws.nbytes
        dbytes = g.DeviceBuffer(nbytes + 16)
        out_bytes = nblocks * block_len * 4
        size = GUARD + 16 + out_bytes + GUARD
        dzz = g.DeviceBuffer(size)
        try:
            assert dbytes.ptr % 4 == 0 and dzz.ptr % 16 == 0 and self.dws.ptr % 16 == 0
            dbytes.upload(np.frombuffer(blob + bytes(16), np.uint8))
            dzz.upload(np.full(size, 0xA5, np.uint8))
            at = GUARD + offset
            if device is None:
                rc = L.jpegx_entropy_decode_n(dbytes.ptr, nbytes, nblocks, block_len, self.dws.ptr, dzz.ptr + at, stream)
                g.check(rc, "jpegx_entropy_decode_n")
                status = L.jpegx_entropy_decode_status_n(self.dws.ptr, stream)
            else:
                rc = L.jpegx_entropy_decode_n_on(device, dbytes.ptr, nbytes, nblocks, block_len, self.dws.ptr, dzz.ptr + at, stream)
                g.check(rc, "jpegx_entropy_decode_n_on")
                status = L.jpegx_entropy_decode_status_n_on(device, self.dws.ptr, stream)
            buf = dzz.download((size,), np.uint8)
            zz = buf[at:at + out_bytes].copy().view(np.int32).reshape(nblocks, block_len)
            return status, zz, buf[:at], buf[at + out_bytes:]
        finally:
            dbytes.free()
            dzz.free()

    def free(self):
        self.dws.free()


@pytest.mark.parametrize("block_len,nblocks", [(9, 67), (65, 67), (729, 23), (1024, 9)])
def test_coefficients_at_every_dword_offset_between_guards(gpu, block_len, nblocks):
    """bpw * block_len is no multiple of 4 at 729 (bpw 11) and 65: tiles start and end at every offset inside a 16-byte piece."""
    z = adv.build("mixed", block_len, nblocks)
    blob = gpu.entropy_encode_n(z)
    c = Caller(gpu, gpu.lib().jpegx_entropy_decode_workspace_bytes_n(len(blob), nblocks, block_len))
    try:
        for offset in (0, 4, 8, 12):
            status, got, front, back = c.decode(blob, nblocks, block_len, offset)
            assert status == 0 and np.array_equal(got, z), offset
            assert np.all(front == 0xA5) and np.all(back == 0xA5), "offset %d: guard bytes written" % offset
    finally:
        c.free()


def test_a_refused_stream_writes_only_the_coefficients(gpu):
    blob, nblocks = advd.refusals(64)["one_block_more"]
    c = Caller(gpu, gpu.lib().jpegx_entropy_decode_workspace_bytes_n(len(blob), nblocks, 64))
    try:
        status, _, front, back = c.decode(blob, nblocks, 64, 4)
        assert status == -1 and b"device decoder" in gpu.lib().jpegx_last_error()
        assert np.all(front == 0xA5) and np.all(back == 0xA5)
    finally:
        c.free()


def test_a_workspace_is_reused_as_it_is(gpu):
    """Long, short, long on one workspace that nobody clears; a refusal in between leaves nothing behind either."""
    L = gpu.lib()
    long_z, short_z = adv.build("mixed", 16, 1300), adv.build("mixed", 576, 3)
    long_blob, short_blob = gpu.entropy_encode_n(long_z), gpu.entropy_encode_n(short_z)
    bad_blob, bad_n = advd.refusals(16)["cut_by_one_byte"]
    c = Caller(gpu, max(L.jpegx_entropy_decode_workspace_bytes_n(len(long_blob), 1300, 16),
                        L.jpegx_entropy_decode_workspace_bytes_n(len(short_blob), 3, 576)))
    try:
        for blob, z, n, length in [(long_blob, long_z, 1300, 16), (short_blob, short_z, 3, 576), (bad_blob, None, bad_n, 16),
                                   (long_blob, long_z, 1300, 16), (short_blob, short_z, 3, 576)]:
            status, got, _, _ = c.decode(blob, n, length)
            if z is None:
                assert status == -1
            else:
                assert status == 0 and np.array_equal(got, z)
    finally:
        c.free()


def test_explicit_device_twins_and_a_stream(gpu):
    z = adv.build("mixed", 576, 67)
    blob = gpu.entropy_encode_n(z)
    L = gpu.lib()
    st = ctypes.c_void_p()
    gpu.check(L.jpegx_stream_create(ctypes.byref(st)), "jpegx_stream_create")
    c = Caller(gpu, L.jpegx_entropy_decode_workspace_bytes_n(len(blob), 67, 576))
    try:
        for kwargs in ({"device": 0}, {"stream": st}, {"device": 0, "stream": st}):
            status, got, front, back = c.decode(blob, 67, 576, 8, **kwargs)
            assert status == 0 and np.array_equal(got, z) and np.all(front == 0xA5) and np.all(back == 0xA5)
        out = np.empty((67, 576), np.int32)
        buf = np.frombuffer(blob, np.uint8)
        gpu.check(L.jpegx_host_entropy_decode_n_gpu_on(0, buf.ctypes.data, buf.size, 67, 576, out.ctypes.data), "jpegx_host_entropy_decode_n_gpu_on")
        assert np.array_equal(out, z)
    finally:
        c.free()
        gpu.check(L.jpegx_stream_destroy(st), "jpegx_stream_destroy")


def test_entropy_decode_n_device_raises_on_a_refused_stream(gpu):
    z = adv.build("mixed", 64, 5)
    blob = gpu.entropy_encode_n(z)
    L = gpu.lib()
    dbytes, dzz = gpu.DeviceBuffer(len(blob) + 16), gpu.DeviceBuffer(z.nbytes)
    dws = gpu.DeviceBuffer(L.jpegx_entropy_decode_workspace_bytes_n(len(blob), 6, 64))
    try:
        dbytes.upload(np.frombuffer(blob + bytes(16), np.uint8))
        gpu.entropy_decode_n_device(dbytes.ptr, len(blob), 5, 64, dws.ptr, dzz.ptr)
        assert np.array_equal(dzz.download((5, 64), np.int32), z)
        with pytest.raises(gpu.JpegxError, match="device decoder"):
            gpu.entropy_decode_n_device(dbytes.ptr, len(blob), 4, 64, dws.ptr, dzz.ptr)
        with pytest.raises(gpu.JpegxError, match="device decoder"):
            gpu.entropy_decode_n_device(dbytes.ptr, len(blob) - 1, 5, 64, dws.ptr, dzz.ptr)
    finally:
        for b in (dbytes, dzz, dws):
            b.free()


# ---- streams built against a decoder that finds block starts ---------------------------------------------------------
@pytest.mark.parametrize("block_len,nblocks,dense", advd.FALSE_STARTS)
def test_false_starts(gpu, block_len, nblocks, dense):
    z = advd.false_starts(block_len, nblocks, dense)
    blob = gpu.entropy_encode_n(z)
    assert np.array_equal(gpu.entropy_decode_n_gpu(blob, nblocks, block_len), gpu.entropy_decode_n(blob, nblocks, block_len))


@pytest.mark.parametrize("block_len", [4, 9, 64, 65, 576, 1024])
def test_one_byte_blocks_longest_blocks_and_refusals(gpu, block_len):
    for nblocks in (67, 700):
        z = advd.one_byte_blocks(block_len, nblocks)
        assert np.array_equal(gpu.entropy_decode_n_gpu(gpu.entropy_encode_n(z), nblocks, block_len), z)
    for cls in ("dense_max", "last_only"):
        z = adv.build(cls, block_len, 67)
        assert np.array_equal(gpu.entropy_decode_n_gpu(gpu.entropy_encode_n(z), 67, block_len), z)
    blob, nblocks = advd.chain_then_end(block_len)
    assert not gpu.entropy_decode_n_gpu(blob, nblocks, block_len).any()
    for name, (blob, nblocks) in advd.controls(block_len).items():
        assert np.array_equal(gpu.entropy_decode_n_gpu(blob, nblocks, block_len), gpu.entropy_decode_n(blob, nblocks, block_len)), name
    for name, (blob, nblocks) in advd.refusals(block_len).items():
        with pytest.raises(gpu.JpegxError):
            gpu.entropy_decode_n(blob, nblocks, block_len)
        with pytest.raises(gpu.JpegxError, match="device decoder"):
            gpu.entropy_decode_n_gpu(blob, nblocks, block_len)


def test_more_blocks_than_bytes_is_refused(gpu):
    """The grid of the first kernel then covers the blocks, not the bytes; every start stays NIL."""
    for blob, nblocks, block_len in [(b"\x00", 5000, 16), (bytes(3), 300, 1024), (b"\x00", 2, 1)]:
        with pytest.raises(gpu.JpegxError):
            gpu.entropy_decode_n(blob, nblocks, block_len)
        with pytest.raises(gpu.JpegxError, match="device decoder"):
            gpu.entropy_decode_n_gpu(blob, nblocks, block_len)
    assert not gpu.entropy_decode_n_gpu(bytes(3), 3, 1024).any()


def test_refusal_parity_fuzz(gpu):
    """The device never accepts what the host parser refuses; what both accept is equal; it is stricter only on damaged
    padding (at most 5 cases of 200, the count the model has on the CPU).  This checks refusals, not robustness by trial:
    why every load and store is in range is written at the load or store."""
    stricter, both = [], 0
    for block_len in model.FUZZ_LENGTHS:
        for kind, blob, nblocks in model.fuzz_cases(block_len):
            host = model.host_decode(blob, nblocks, block_len)
            try:
                got = gpu.entropy_decode_n_gpu(blob, nblocks, block_len)
            except gpu.JpegxError:
                got = None
            assert not (got is not None and host is None), "the device accepts what the host parser refuses: %s, %d" % (kind, block_len)
            if host is not None and got is None:
                stricter.append(kind)
            elif host is not None:
                both += 1
                assert np.array_equal(host, got), (kind, block_len)
    assert both >= 30
    assert len(stricter) <= 5 and set(stricter) <= {"padding"}, stricter


# ---- the pooled job ----------------------------------------------------------------------------------------------------
# (N, height, width): three decode workgroups' worth of blocks
JOB_SHAPES = [(3, 36, 48), (4, 48, 64), (16, 128, 192), (24, 144, 168), (32, 128, 192)]
JOB_QUANTISERS = [("none", 0.0), ("discard", 3.0), ("divide", 40.0)]


@pytest.mark.parametrize("n,h,w", JOB_SHAPES)
def test_decompress_plane_n(gpu, n, h, w):
    assert (h // n) * (w // n) == 3 * bpw_of(n * n)
    rng = np.random.default_rng(n * 100000 + h * 1000 + w)
    y, x = np.mgrid[0:h, 0:w]
    planes = [rng.integers(0, 256, (h, w)).astype(np.float64) - 128.0, ((3 * x + 5 * y) % 256).astype(np.float64) - 128.0]
    ran = 0
    for plane in planes:
        for mode, param in JOB_QUANTISERS:
            if np.abs(gpu.forward_fused_n(plane, n, mode, param)).max() > 16383:
                continue                                 # no coded form: an amplitude beyond 15 bits (a DC is the sum of N * N samples)
            ran += 1
            blob = gpu.compress_plane_n(plane, n, mode, param)
            zz = gpu.entropy_decode_n(blob, (h // n) * (w // n), n * n).reshape(h // n, w // n, n * n)
            for out, dtype in (("u8", np.uint8), ("i32", np.int32)):
                got = gpu.decompress_plane_n(blob, h, w, n, mode, param, out=out)
                assert got.dtype == dtype and got.shape == (h, w)
                assert np.array_equal(got, gpu.inverse_fused_n(zz, n, mode, param, out=out)), (n, mode, out)
    assert ran >= 3


def test_decompress_plane_n_refuses_and_gives_the_context_back(gpu):
    plane = np.random.default_rng(11).integers(0, 256, (64, 96)).astype(np.float64) - 128.0
    blob = gpu.compress_plane_n(plane, 16, "divide", 40.0)
    want = gpu.decompress_plane_n(blob, 64, 96, 16, "divide", 40.0)
    L = gpu.lib()
    for bad in (blob[:-1], blob + b"\x00", blob[:10] + b"\x01" + blob[10:]):
        buf = np.frombuffer(bad, np.uint8)
        out = np.full((64, 96), 0x5A, np.uint8)
        rc = L.jpegx_host_decompress_plane_n(buf.ctypes.data, buf.size, 64, 96, 16, gpu.mode_of("divide"), 40.0, gpu.F_CLAMP_U8, out.ctypes.data, 96)
        if rc == 0:                                      # an inserted byte may leave a stream the host parser takes too
            assert np.array_equal(gpu.entropy_decode_n(bad, 24, 256), gpu.entropy_decode_n_gpu(bad, 24, 256))
            continue
        assert rc == -1 and np.all(out == 0x5A), "a refused stream wrote the caller's samples"
        with pytest.raises(gpu.JpegxError):
            gpu.decompress_plane_n(bad, 64, 96, 16, "divide", 40.0)
        assert np.array_equal(gpu.decompress_plane_n(blob, 64, 96, 16, "divide", 40.0), want)      # the next job succeeds
    out = np.full((64, 100), 0x5A, np.uint8)                # a wider pitch: the slack behind the rows stays the caller's
    buf = np.frombuffer(blob, np.uint8)
    gpu.check(L.jpegx_host_decompress_plane_n_on(0, buf.ctypes.data, buf.size, 64, 96, 16, gpu.mode_of("divide"), 40.0, gpu.F_CLAMP_U8,
                                                 out.ctypes.data, 100), "jpegx_host_decompress_plane_n_on")
    assert np.array_equal(out[:, :96], want) and np.all(out[:, 96:] == 0x5A)


# ---- the pipeline ------------------------------------------------------------------------------------------------------
# (block_size, dct_size, quantiser, parameter name, value, height, width)
BANDS = [(1, 4, "divide", "divisor", 40, 64, 96),
         (1, 4, "none", None, None, 53, 77),                      # ragged: Padding and DCTPadding cropped on the host
         (1, 6, "discard", "keep", 5, 60, 84),
         (1, 6, "divide", "divisor", 40, 53, 77),
         (5, 24, "divide", "divisor", 1000, 240, 360),            # the reference README's configuration
         (5, 24, "divide", "divisor", 300, 233, 351)]             # ragged at block_size 5


def _config(bs, n, name, key, value, h, w):
    import pipeline
    q = pipeline.QuantizationMethod(name, **({key: value} if key else {}))
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n, quantization=q)


@pytest.mark.parametrize("bs,n,name,key,value,h,w", BANDS)
def test_decompress_band_with_the_job_road_equals_the_road_of_before(gpu, monkeypatch, bs, n, name, key, value, h, w):
    import pipeline
    cfg = _config(bs, n, name, key, value, h, w)
    band = np.random.default_rng(h * w + n).integers(0, 256, (h, w))
    blob = pipeline.compress_band(band, cfg)
    assert isinstance(blob, bytes)
    calls = []
    real = gpu.decompress_plane_n
    monkeypatch.setattr(gpu, "decompress_plane_n", lambda *a, **k: (calls.append(k.get("out")), real(*a, **k))[1])
    with monkeypatch.context() as m:                         # the road of before: host parser + jpegx_inverse_fused_n
        m.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", None)
        want, want_u8 = pipeline.decompress_band(blob, cfg), pipeline.decompress_band_u8(blob, cfg)
    assert calls == []
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", 0)
        got, got_u8 = pipeline.decompress_band(blob, cfg), pipeline.decompress_band_u8(blob, cfg)
    assert calls == ["i32", "u8"], "the device job was not used"
    assert got.dtype == want.dtype and got.shape == want.shape == (h, w) and got.tobytes() == want.tobytes()
    assert got_u8.dtype == want_u8.dtype == np.uint8 and got_u8.shape == want_u8.shape and got_u8.tobytes() == want_u8.tobytes()
    with monkeypatch.context() as m:                         # planes below the threshold keep the road of before
        m.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", 1 << 40)
        assert pipeline.decompress_band(blob, cfg).tobytes() == want.tobytes() and calls == ["i32", "u8"]


def test_the_gate_as_it_is_set(gpu, monkeypatch):
    """A plane of exactly pipeline.DCTN_ENTROPY_DECODE_MIN_SAMPLES samples takes the job, one block row fewer does not."""
    import pipeline
    gate = pipeline.DCTN_ENTROPY_DECODE_MIN_SAMPLES
    if gate is None:
        gate = 1 << 16
        monkeypatch.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", gate)
    w = 256
    assert gate % (4 * w) == 0 and gate // w > 4
    calls = []
    real = gpu.decompress_plane_n
    monkeypatch.setattr(gpu, "decompress_plane_n", lambda *a, **k: (calls.append(k.get("out")), real(*a, **k))[1])
    for h, used in ((gate // w, ["u8"]), (gate // w - 4, [])):
        cfg = _config(1, 4, "divide", "divisor", 40, h, w)
        band = np.random.default_rng(h).integers(0, 256, (h, w))
        blob = pipeline.compress_band(band, cfg)
        del calls[:]
        got = pipeline.decompress_band_u8(blob, cfg)
        assert calls == used, (h, calls)
        with monkeypatch.context() as m:
            m.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", None)
            assert got.tobytes() == pipeline.decompress_band_u8(blob, cfg).tobytes()


def test_a_damaged_blob_raises_the_same_exception_on_both_roads(gpu, monkeypatch):
    import pipeline
    cfg = _config(1, 16, "divide", "divisor", 40, 64, 48)
    blob = pipeline.compress_band(np.random.default_rng(3).integers(0, 256, (64, 48)), cfg)
    for bad in (blob[:-1], blob + b"\x00", b"\x01" + blob):
        raised = []
        for setting in (None, 0):
            monkeypatch.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", setting)
            for f in (pipeline.decompress_band, pipeline.decompress_band_u8):
                with pytest.raises(Exception) as exc:
                    f(bad, cfg)
                raised.append((type(exc.value), str(exc.value)))
        assert raised[0] == raised[2] and raised[1] == raised[3], raised
    monkeypatch.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", 0)
    assert pipeline.decompress_band(blob, cfg).shape == (64, 48)          # the pool is usable afterwards
