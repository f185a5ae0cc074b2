"""GPU: the batch codec on device buffers for dct_size != 8 (jpegx_batch_compress_n / _status_n / _emit_n / _decompress_n) and
its Python surface.  Every comparison is exact.

Two references.  The per-band device road, jpegx.compress_band_n / decompress_band_n: the batch runs the same kernels on
the same numbers, so its bytes and samples must be those, band for band, on ANY content -- 8-bit noise included.  And the
product-free oracle of tests/codec_oracle_n.py on its tie-free bands (tests/test_codec_oracle_n.py: Known asserts the
distance of every coefficient and sample from a rounding tie when a case is built).

The shapes are the smallest that reach each mechanism: block lengths below 64 (several blocks in one wave) and above,
1, 35, 64 and 65 blocks per plane with 1, 2, 65 and 130 planes (waves and groups of 64 blocks that straddle planes),
group_planes 1, 2 and 0 with a short last group, destinations 0, 1, 7 and 15 bytes behind a 16-byte boundary, and ONE
workspace for all of them that is filled once and never cleared."""
import numpy as np
import pytest

import codec_oracle_n as on
from batch_n_dev import CANARY, Fenced, band_shape, noise_bands
from test_codec_oracle_n import case_id, known

pytestmark = pytest.mark.gpu

WORKSPACE_BYTES = 96 << 20

# (N, bs, block rows, block columns, ragged, planes, group_planes, destination skew, mode, param)
COMPRESS_CASES = [
    (2, 1, 5, 7, False, 130, 0, 0, "none", 0.0),
    (2, 3, 8, 8, True, 65, 2, 1, "divide", 0.75),
    (3, 2, 1, 1, True, 65, 2, 1, "none", 0.0),
    (3, 1, 5, 13, False, 2, 1, 7, "discard", 2.0),
    (5, 1, 8, 8, False, 65, 1, 7, "divide", 40.0),
    (5, 3, 5, 13, True, 2, 0, 15, "discard", 2.0),
    (5, 1, 1, 1, False, 130, 2, 0, "none", 0.0),
    (8, 1, 5, 7, True, 130, 2, 0, "divide", 40.0),
    (12, 1, 5, 13, False, 65, 2, 1, "divide", 40.0),
    (24, 5, 1, 1, True, 130, 0, 7, "divide", 1000.0),
    (24, 1, 5, 7, True, 5, 2, 15, "divide", 40.0),
    (32, 1, 8, 8, False, 2, 1, 0, "divide", 40.0),
    (32, 2, 5, 13, True, 1, 0, 1, "divide", 1000.0),
]


def compress_id(c):
    return "N%d-bs%d-%dx%d%s-p%d-g%d-s%d-%s%g" % (c[0], c[1], c[2], c[3], "r" if c[4] else "", c[5], c[6], c[7], c[8], c[9])


@pytest.fixture(scope="module")
def workspace(gpu):
    """One workspace for every case of this module: filled with a pattern once, never cleared between calls."""
    buf = gpu.DeviceBuffer(WORKSPACE_BYTES)
    gpu.check(gpu.lib().jpegx_memset(buf.ptr, 0xC3, WORKSPACE_BYTES, None), "jpegx_memset")
    gpu.check(gpu.lib().jpegx_device_synchronize())
    yield buf
    buf.free()


@pytest.fixture(scope="module")
def reference():
    """(bands, blobs by the per-band device road) per compress case, made once and shared by the tests both ways."""
    cache = {}

    def get(gpu, case):
        if case not in cache:
            n, bs, hb, wb, ragged, nplanes, _, _, mode, param = case
            rows, cols = band_shape(hb, wb, n, bs, ragged)
            bands = noise_bands([n, bs, hb, wb, nplanes], nplanes, rows, cols, smooth_every=3)
            blobs = [gpu.compress_band_n(b, bs, n, mode, param) for b in bands]
            assert all(isinstance(b, bytes) and b for b in blobs)
            bands.setflags(write=False)
            cache[case] = (bands, blobs)
        return cache[case]
    return get


def offsets_of(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    return off


@pytest.mark.parametrize("case", COMPRESS_CASES, ids=compress_id)
def test_compress_equals_the_per_band_road(gpu, workspace, reference, case):
    n, bs, hb, wb, ragged, nplanes, gp, skew, mode, param = case
    bands, want = reference(gpu, case)
    _, rows, cols = bands.shape
    shape = (nplanes, rows, cols, bs, n)
    assert gpu.band_shape_n(rows, cols, bs, n) == (hb * n, wb * n)
    assert 0 < gpu.batch_workspace_bytes_n(*shape, gp) <= WORKSPACE_BYTES
    off, total = offsets_of(want), sum(len(b) for b in want)
    assert total <= gpu.batch_max_bytes_n(*shape)
    pitch = cols + 5
    din = Fenced(gpu, nplanes * rows * pitch, skew=3)
    dout = Fenced(gpu, total + 64, skew=skew)
    try:
        stacked = np.full((nplanes * rows, pitch), 0xEE, np.uint8)
        stacked[:, :cols] = bands.reshape(nplanes * rows, cols)
        din.upload(stacked)
        # sizes only
        gpu.batch_compress_n_device(din.ptr, *shape, workspace.ptr, None, 0, mode, param, gp, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status_n(workspace.ptr, *shape, gp)
        assert (rc, got_total) == (0, total)
        assert np.array_equal(got_off, off)
        # one byte short: nothing is written, the total is right, and the emit step completes the job
        gpu.batch_compress_n_device(din.ptr, *shape, workspace.ptr, dout.ptr, total - 1, mode, param, gp, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status_n(workspace.ptr, *shape, gp)
        assert (rc, got_total) == (1, total) and np.array_equal(got_off, off)
        assert b"needs %d bytes" % total in gpu.lib().jpegx_last_error()
        dout.untouched("a compress one byte short")
        gpu.batch_emit_n_device(workspace.ptr, *shape, dout.ptr, total, gp)
        rc, got_total, _ = gpu.batch_compress_status_n(workspace.ptr, *shape, gp)
        assert (rc, got_total) == (0, total)
        assert dout.payload(total, "emit").tobytes() == b"".join(want)
        # exactly the total, in one go
        dout.fill()
        gpu.batch_compress_n_device(din.ptr, *shape, workspace.ptr, dout.ptr, total, mode, param, gp, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status_n(workspace.ptr, *shape, gp)
        assert (rc, got_total) == (0, total) and np.array_equal(got_off, off)
        got = dout.payload(total, "compress").tobytes()
        for p in range(nplanes):
            assert got[int(off[p]):int(off[p + 1])] == want[p], "band %d of %s" % (p, compress_id(case))
    finally:
        din.free()
        dout.free()


@pytest.mark.parametrize("case", COMPRESS_CASES, ids=compress_id)
def test_decompress_equals_the_per_band_road(gpu, workspace, reference, case):
    n, bs, hb, wb, ragged, nplanes, gp, skew, mode, param = case
    if mode == "divide" and param != np.trunc(param):
        mode, param = "divide", 3.0                       # the same streams under a whole divisor: any well-formed stream decodes
    bands, blobs = reference(gpu, case)
    _, rows, cols = bands.shape
    shape = (nplanes, rows, cols, bs, n)
    want = np.stack([gpu.decompress_band_n(b, rows, cols, bs, n, mode, param) for b in blobs])
    off, total = offsets_of(blobs), sum(len(b) for b in blobs)
    first = gpu.batch_groups_n(off, *shape, gp)
    if gp:
        assert np.array_equal(first, list(range(0, nplanes, gp)) + [nplanes])
    assert 0 < gpu.batch_decompress_workspace_bytes_n(total, *shape, gp) <= WORKSPACE_BYTES
    opitch = cols + 7
    din = Fenced(gpu, total, skew=skew)                   # no slack behind the stream, any alignment
    dout = Fenced(gpu, nplanes * rows * opitch, skew=1)
    try:
        din.upload(np.frombuffer(b"".join(blobs), np.uint8))
        gpu.batch_decompress_n_device(din.ptr, off, *shape, workspace.ptr, dout.ptr, opitch, mode, param, gp)
        got = dout.payload(dout.nbytes, "decompress").reshape(nplanes, rows, opitch)
        assert np.array_equal(got[:, :, :cols], want)
        assert np.all(got[:, :, cols:] == CANARY), "the pitch slack was written"
    finally:
        din.free()
        dout.free()


FREE_CASES = [c for c in on.matrix_cases() if c[5] == "free"]


@pytest.mark.parametrize("case", FREE_CASES, ids=case_id)
def test_both_ways_against_the_oracle(gpu, case):
    """Three copies of a tie-free band as one batch in groups of two: the oracle's bytes, three times, with the index of
    that, and the oracle's band back.  A divisor that is no integer decodes as jpegx_host_decompress_band_n decodes it
    (without the reference's truncation), so there the way back is compared with that entry instead."""
    k = known(case)
    band = np.ascontiguousarray(k.band, np.uint8)
    blobs = gpu.batch_compress_n(np.stack([band] * 3), k.bs, k.n, k.mode, k.param, group_planes=2)
    assert blobs == [k.blob] * 3, k.what
    back = gpu.batch_decompress_n(blobs, k.h, k.w, k.bs, k.n, k.mode, k.param, group_planes=2)
    assert back.dtype == np.uint8 and back.shape == (3, k.h, k.w)
    whole = k.mode != "divide" or k.param == np.trunc(k.param)
    want = k.inv.band if whole else gpu.decompress_band_n(k.blob, k.h, k.w, k.bs, k.n, k.mode, k.param)
    for p in range(3):
        assert np.array_equal(back[p], want), (k.what, p)


def test_an_amplitude_beyond_15_bits_in_the_middle_of_the_batch(gpu, workspace):
    """Peak 255 at N 16 without a divisor: a DC of 255 * 256 = 65280.  One such plane among five quiet ones."""
    n, bs, rows, cols, nplanes = 16, 1, 32, 48, 5
    bands = np.full((nplanes, rows, cols), 8, np.uint8)
    bands[2] = 255
    shape = (nplanes, rows, cols, bs, n)
    din, dout = Fenced(gpu, bands.nbytes), Fenced(gpu, 4096, skew=1)
    try:
        din.upload(bands)
        gpu.batch_compress_n_device(din.ptr, *shape, workspace.ptr, dout.ptr, 4096, "none", 0.0, 2)
        rc, _, _ = gpu.batch_compress_status_n(workspace.ptr, *shape, 2)
        assert rc == -1 and b"BadRleCodeError" in gpu.lib().jpegx_last_error()
        dout.untouched("a refused compress")
        gpu.batch_emit_n_device(workspace.ptr, *shape, dout.ptr, 4096, 2)
        assert gpu.batch_compress_status_n(workspace.ptr, *shape, 2)[0] == -1
        dout.untouched("an emit after a refused compress")
        with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
            gpu.batch_compress_n(bands, bs, n, "none", 0.0)
        # the same workspace takes the next batch as it is
        bands[2] = 8
        din.upload(bands)
        gpu.batch_compress_n_device(din.ptr, *shape, workspace.ptr, dout.ptr, 4096, "none", 0.0, 2)
        rc, total, off = gpu.batch_compress_status_n(workspace.ptr, *shape, 2)
        assert rc == 0
        want = gpu.compress_band_n(bands[0], bs, n, "none", 0.0)
        assert dout.payload(total, "compress").tobytes() == want * nplanes
    finally:
        din.free()
        dout.free()


def test_a_damaged_plane_in_the_second_group(gpu, workspace):
    """Seven planes in groups of three whose second group starts at an offset that is no multiple of 4; plane 4 is cut
    short by a byte the host parser refuses (a chain code that runs past the block).  The error names planes 3..5, the
    first group's bands are written, nothing of the second or the third group is."""
    n, bs, nplanes, gp = 4, 2, 7, 3
    rows, cols = band_shape(3, 4, n, bs, True)
    bands = noise_bands(5, nplanes, rows, cols)
    shape = (nplanes, rows, cols, bs, n)
    blobs = [gpu.compress_band_n(b, bs, n, "divide", 3.0) for b in bands]
    if sum(len(b) for b in blobs[:3]) % 4 == 0:          # keep the second group off a dword boundary
        bands = bands.copy()
        for v in range(1, 64):
            bands[0, 0, 0] ^= v
            blobs[0] = gpu.compress_band_n(bands[0], bs, n, "divide", 3.0)
            if sum(len(b) for b in blobs[:3]) % 4:
                break
    off = offsets_of(blobs)
    assert int(off[3]) % 4 != 0
    want = np.stack([gpu.decompress_band_n(b, rows, cols, bs, n, "divide", 3.0) for b in blobs])
    stream = np.frombuffer(b"".join(blobs), np.uint8).copy()
    din, dout = Fenced(gpu, stream.size), Fenced(gpu, nplanes * rows * cols)
    try:
        din.upload(stream)
        gpu.batch_decompress_n_device(din.ptr, off, *shape, workspace.ptr, dout.ptr, cols, "divide", 3.0, gp)
        assert np.array_equal(dout.payload(dout.nbytes, "decompress").reshape(nplanes, rows, cols), want)
        # 0xF0 chain codes from the first byte of plane 4 on: more than 16 zeros in a block of 16 coefficients
        stream[int(off[4]):int(off[4]) + 2] = 0xF0
        bad = stream[int(off[4]):int(off[5])].tobytes()
        with pytest.raises(gpu.JpegxError):
            gpu.entropy_decode_n(bad, 12, n * n)           # the host parser refuses it
        din.upload(stream)
        dout.fill()
        with pytest.raises(gpu.JpegxError, match=r"planes 3\.\.5"):
            gpu.batch_decompress_n_device(din.ptr, off, *shape, workspace.ptr, dout.ptr, cols, "divide", 3.0, gp)
        got = dout.payload(3 * rows * cols, "a refused second group").reshape(3, rows, cols)
        assert np.array_equal(got, want[:3])
        with pytest.raises(gpu.JpegxError, match=r"planes 3\.\.5"):
            gpu.batch_decompress_n(blobs[:4] + [bad] + blobs[5:], rows, cols, bs, n, "divide", 3.0, group_planes=gp)
    finally:
        din.free()
        dout.free()


@pytest.mark.parametrize("bs,quant", [(1, "qtable"), (2, "qtable"), (4, "divide")])
def test_pipeline_functions_at_dct_size_8(gpu, bs, quant):
    """dct_size 8 goes through the existing jpegx.batch_compress / batch_decompress: the per-band functions' results."""
    import pipeline
    rows, cols = 5 * 8 * bs, 6 * 8 * bs
    bands = noise_bands([8, bs], 4, rows, cols, smooth_every=2)
    q = pipeline.QuantizationMethod("qtable") if quant == "qtable" else pipeline.QuantizationMethod("divide", divisor=7)
    cfg = pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=8, quantization=q)
    calls = []
    real_c, real_d = gpu.batch_compress, gpu.batch_decompress
    try:
        gpu.batch_compress = lambda *a, **k: calls.append("c") or real_c(*a, **k)
        gpu.batch_decompress = lambda *a, **k: calls.append("d") or real_d(*a, **k)
        blobs = pipeline.compress_bands(list(bands), cfg)
        back = pipeline.decompress_bands_u8(blobs, cfg)
    finally:
        gpu.batch_compress, gpu.batch_decompress = real_c, real_d
    assert calls == ["c", "d"], "the batch road did not run"
    assert blobs == [pipeline.compress_band(b, cfg) for b in bands]
    for got, blob in zip(back, blobs):
        ref = pipeline.decompress_band_u8(blob, cfg)
        assert got.dtype == ref.dtype == np.uint8 and np.array_equal(got, ref)


@pytest.mark.parametrize("n,bs", [(4, 1), (4, 5), (24, 1), (24, 5)])
def test_python_surface_equals_the_per_band_functions(gpu, n, bs):
    """jpegx.batch_compress_n / batch_decompress_n against compress_band_n / decompress_band_n, and pipeline.compress_bands /
    decompress_bands_u8 against compress_band / decompress_band_u8, on a batch of noise and smooth bands."""
    import pipeline
    from test_codec_oracle_n import config_of
    mode, param = ("divide", 40.0)
    rows, cols = band_shape(2, 3, 24, bs, True)           # 48 x 72 samples after pooling at either N: above DCTN_MIN_SAMPLES
    bands = noise_bands([n, bs], 5, rows, cols, smooth_every=2)
    want = [gpu.compress_band_n(b, bs, n, mode, param) for b in bands]
    assert gpu.batch_compress_n(bands, bs, n, mode, param) == want
    want_back = [gpu.decompress_band_n(b, rows, cols, bs, n, mode, param) for b in want]
    assert np.array_equal(gpu.batch_decompress_n(want, rows, cols, bs, n, mode, param), np.stack(want_back))
    cfg = config_of(n, bs, mode, param, rows, cols)
    calls = []
    real_c, real_d = gpu.batch_compress_n, gpu.batch_decompress_n
    try:
        gpu.batch_compress_n = lambda *a, **k: calls.append("c") or real_c(*a, **k)
        gpu.batch_decompress_n = lambda *a, **k: calls.append("d") or real_d(*a, **k)
        blobs = pipeline.compress_bands(list(bands), cfg)
        back = pipeline.decompress_bands_u8(blobs, cfg)
    finally:
        gpu.batch_compress_n, gpu.batch_decompress_n = real_c, real_d
    assert calls == ["c", "d"], "the batch road did not run"
    assert blobs == [pipeline.compress_band(b, cfg) for b in bands] == want
    per_band = [pipeline.decompress_band_u8(b, cfg) for b in blobs]
    assert len(back) == len(per_band)
    for got, ref in zip(back, per_band):
        assert got.dtype == ref.dtype == np.uint8 and np.array_equal(got, ref)
