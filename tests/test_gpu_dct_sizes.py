"""DCT sizes other than 8 on the device (csrc/jpegx_dctn.hip) against the reference's code under the criterion of
dctn_criterion.py: the fused forward and inverse entries, the float64 stage entries, pitches, the explicit-device twins,
a non-default stream, and the pipeline roads.  Shapes are the smallest that reach every hazard of a run-time-N kernel:
N^2 not a multiple of 64, several blocks per wave, a block count that is no multiple of the blocks per workgroup,
pitch != W, odd N, and planes that are not symmetric (a swapped pass order or a transposed table shows)."""
import ctypes
import functools

import numpy as np
import pytest

import dctn_criterion as crit
from dctn_dev import forward_dev, inverse_dev

pytestmark = pytest.mark.gpu

# N, H, W, input pitch (None = W)
SHAPES = [(2, 36, 260, 264), (3, 9, 3, None), (3, 39, 201, None), (5, 35, 45, None), (12, 24, 36, None), (16, 48, 32, None),
          (24, 48, 72, None), (24, 240, 264, None), (32, 64, 96, None)]
PLANES = ["noise", "ramp", "all255", "all0", "pooled"]


def quantisers(n):
    return [("none", 0.0)] + [("discard", float(k)) for k in (1, 2, n, n + 3)] + [("divide", d) for d in (40.0, 1000.0, 2.0, 0.75, -7.0)]


@functools.lru_cache(maxsize=None)
def plane_of(kind, h, w):
    rng = np.random.default_rng(h * 1000 + w)
    if kind == "noise":
        a = rng.integers(0, 256, (h, w)).astype(np.float64)
    elif kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        a = ((3 * x + 5 * y) % 256).astype(np.float64)
    elif kind == "all255":
        a = np.full((h, w), 255.0)
    elif kind == "all0":
        a = np.zeros((h, w))
    else:
        raw = rng.integers(0, 256, (2 * h, 2 * w)).astype(np.float64)
        a = raw.reshape(h, 2, w, 2).mean(axis=(1, 3))                       # quarter-integer samples
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_dct_of(kind, n, h, w):
    out = crit.ref_dct(plane_of(kind, h, w), n)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("n,h,w,pitch", SHAPES)
def test_forward_fused_n(gpu, n, h, w, pitch):
    from pipeline.zigzag_order import Zigzag
    for kind in PLANES:
        plane, dct = plane_of(kind, h, w), ref_dct_of(kind, n, h, w)
        for mode, param in quantisers(n):
            zz = forward_dev(gpu, plane, n, mode, param, pitch) if pitch else gpu.forward_fused_n(plane, n, mode, param)
            assert zz.dtype == np.int32 and zz.shape == (h // n, w // n, n * n)
            k = crit.from_stream(zz, n)
            crit.check_forward(k, dct, n, mode, param, what="%s %dx%d" % (kind, h, w), cap=0.02 if (mode, param) == ("divide", 40.0) else None)
            if kind == "all255" and mode == "none":
                assert np.all(zz[:, :, 0] == 255 * n * n) and not np.any(zz[:, :, 1:])      # 261120 at N = 32: beyond int16
            if kind == "all0":
                assert not np.any(zz)
        # the zigzag order itself, exactly: a plane whose coefficients ARE its positions cannot be built for the
        # transform, so compare the scatter through the float64 stage entry instead
        coef = gpu.dct_f64_n(plane, n)
        assert np.abs(coef - dct).max() <= crit.tau(n)
        zz = gpu.forward_fused_n(plane, n, "none")
        assert np.array_equal(zz, np.rint(coef).astype(np.int32).reshape(h // n, n, w // n, n).swapaxes(1, 2)
                              .reshape(h // n, w // n, n * n)[:, :, Zigzag(n).flat_indices()])


@pytest.mark.parametrize("n,h,w,pitch", SHAPES)
def test_inverse_fused_n(gpu, n, h, w, pitch):
    """Streams produced by the forward REFERENCE (samples come back near integers only by accident for 'divide')."""
    for kind in ("noise", "ramp", "all255", "pooled"):
        dct = ref_dct_of(kind, n, h, w)
        for mode, param in quantisers(n):
            v, _ = crit.quantiser_value(dct, n, mode, param)
            zz = crit.to_stream(np.round(v), n).astype(np.int32)
            restored = crit.from_stream(zz, n).astype(np.float64) * (param if mode == "divide" else 1.0)
            x_ref = crit.ref_idct(restored, n)
            what = "%s %dx%d %s %g" % (kind, h, w, mode, param)
            got = gpu.inverse_fused_n(zz, n, mode, param) if not pitch else inverse_dev(gpu, zz, n, mode, param, out_pitch=w + 3)
            assert got.dtype == np.int32
            crit.check_inverse(got, restored, n, what=what, x_ref=x_ref)
            u8 = gpu.inverse_fused_n(zz, n, mode, param, out="u8") if not pitch else inverse_dev(gpu, zz, n, mode, param, u8=True, out_pitch=w + 5)
            assert u8.dtype == np.uint8
            crit.check_inverse(u8, restored, n, what=what + " u8", clamp=True, x_ref=x_ref)
            assert np.array_equal(u8, np.clip(got, 0, 255).astype(np.uint8))                # the clamp, exactly
    # unclamped int32: a stream whose samples leave 0..255 on both sides
    big = np.zeros((h // n, w // n, n * n), np.int32)
    big[:, :, 0] = 700 * n * n
    big[0, 0, 0] = -300 * n * n
    out = gpu.inverse_fused_n(big, n, "none")
    assert out.max() == 700 and out.min() == -300
    assert np.array_equal(gpu.inverse_fused_n(big, n, "none", out="u8"), np.clip(out, 0, 255).astype(np.uint8))


@pytest.mark.parametrize("n,h,w,pitch", SHAPES)
def test_float64_stage_entries(gpu, n, h, w, pitch):
    for kind in ("noise", "ramp", "pooled"):
        plane, dct = plane_of(kind, h, w), ref_dct_of(kind, n, h, w)
        coef = gpu.dct_f64_n(plane, n)
        assert np.abs(coef - dct).max() <= crit.tau(n)
        x_ref = crit.ref_idct(dct, n)
        t = crit.tau_inv_plane(dct, n)
        back = gpu.idct_f64_n(dct, n, do_round=False)
        assert np.all(np.abs(back - x_ref) <= t)
        crit.check_inverse(gpu.idct_f64_n(dct, n, do_round=True), dct, n, what="idct_f64_n " + kind, x_ref=x_ref)
    if pitch:                                                    # plane-to-plane with both pitches off the width
        plane, dct = plane_of("ramp", h, w), ref_dct_of("ramp", n, h, w)
        L = gpu.lib()
        src = np.full((h, pitch), np.nan)
        src[:, :w] = plane
        opitch = w + 7
        din, dout = gpu.DeviceBuffer(src.nbytes), gpu.DeviceBuffer(h * opitch * 8)
        try:
            din.upload(src)
            dout.upload(np.full((h, opitch), -1.0))
            gpu.check(L.jpegx_dct_f64_n_on(0, din.ptr, h, w, pitch, n, dout.ptr, opitch, None), "jpegx_dct_f64_n_on")
            coef = dout.download((h, opitch), np.float64)
            assert np.all(coef[:, w:] == -1.0) and np.abs(coef[:, :w] - dct).max() <= crit.tau(n)
            gpu.check(L.jpegx_idct_f64_n_on(0, dout.ptr, h, w, opitch, n, din.ptr, pitch, 1, None), "jpegx_idct_f64_n_on")
            back = din.download((h, pitch), np.float64)
            assert np.array_equal(back[:, :w], plane) and np.all(np.isnan(back[:, w:]))
        finally:
            din.free()
            dout.free()


def test_on_twins_and_a_non_default_stream(gpu):
    n, h, w = 5, 35, 45
    plane, dct = plane_of("ramp", h, w), ref_dct_of("ramp", n, h, w)
    want = gpu.forward_fused_n(plane, n, "divide", 40.0)
    L = gpu.lib()
    st = ctypes.c_void_p()
    gpu.check(L.jpegx_stream_create(ctypes.byref(st)), "jpegx_stream_create")
    try:
        for on, stream in ((True, None), (False, st), (True, st)):
            assert np.array_equal(forward_dev(gpu, plane, n, "divide", 40.0, pitch=48, on=on, stream=stream), want)
            back = inverse_dev(gpu, want, n, "divide", 40.0, on=on, stream=stream)
            assert np.array_equal(back, gpu.inverse_fused_n(want, n, "divide", 40.0))
            assert np.array_equal(inverse_dev(gpu, want, n, "divide", 40.0, u8=True, out_pitch=64, on=on, stream=stream),
                                  np.clip(back, 0, 255).astype(np.uint8))
        crit.check_forward(crit.from_stream(want, n), dct, n, "divide", 40.0, what="twins", cap=0.02)
        # the float64 stage entries: plain and _on forms, null and created stream, both pitches off the width
        coef_want, ipitch, opitch = gpu.dct_f64_n(plane, n), w + 3, w + 7
        back_want = gpu.idct_f64_n(coef_want, n, do_round=True)
        assert np.array_equal(back_want, plane)
        src = np.full((h, ipitch), np.nan)
        src[:, :w] = plane
        din, dmid = gpu.DeviceBuffer(src.nbytes), gpu.DeviceBuffer(h * opitch * 8)
        try:
            for on, stream in ((False, None), (False, st), (True, st)):
                din.upload(src)
                dmid.upload(np.full((h, opitch), -1.0))
                fwd = (din.ptr, h, w, ipitch, n, dmid.ptr, opitch, stream)
                gpu.check(L.jpegx_dct_f64_n_on(0, *fwd) if on else L.jpegx_dct_f64_n(*fwd), "jpegx_dct_f64_n")
                gpu.check(L.jpegx_stream_synchronize(stream), "sync")
                coef = dmid.download((h, opitch), np.float64)
                assert np.array_equal(coef[:, :w], coef_want) and np.all(coef[:, w:] == -1.0)
                inv = (dmid.ptr, h, w, opitch, n, din.ptr, ipitch, 1, stream)
                gpu.check(L.jpegx_idct_f64_n_on(0, *inv) if on else L.jpegx_idct_f64_n(*inv), "jpegx_idct_f64_n")
                gpu.check(L.jpegx_stream_synchronize(stream), "sync")
                back = din.download((h, ipitch), np.float64)
                assert np.array_equal(back[:, :w], back_want) and np.all(np.isnan(back[:, w:]))
        finally:
            din.free()
            dmid.free()
        # the host-pointer inverse leaves the caller's pitch slack alone, like the device-pointer entry
        for dtype, flag in ((np.int32, 0), (np.uint8, gpu.F_CLAMP_U8)):
            res = np.full((h, w + 4), 77, dtype=dtype)
            gpu.check(L.jpegx_host_inverse_fused_n(want.ctypes.data, h, w, n, gpu.Q_DIVIDE, 40.0, flag, res.ctypes.data, w + 4),
                      "jpegx_host_inverse_fused_n")
            assert np.all(res[:, w:] == 77)
            assert np.array_equal(res[:, :w], gpu.inverse_fused_n(want, n, "divide", 40.0, out="u8" if flag else "i32"))
    finally:
        gpu.check(L.jpegx_stream_destroy(st), "jpegx_stream_destroy")


def test_block_length_64_equals_the_device_entropy_coder(gpu):
    rng = np.random.default_rng(64)
    zz = rng.integers(-200, 201, (3, 5, 64)).astype(np.int32)
    zz[rng.random(zz.shape) < 0.7] = 0
    zz[1, 2] = 0
    zz[2, 4, 63] = -16383
    assert gpu.entropy_encode_n(zz) == gpu.entropy_encode(zz.astype(np.int16))


# ---- pipeline level ---------------------------------------------------------------------------------------------------
HOST_ONLY = 1 << 62


def _config(h, w, bs, n, mode, **kw):
    import pipeline
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n, quantization=pipeline.QuantizationMethod(mode, **kw))


def _pooled_reference(blob, cfg):
    """(restored coefficient plane, x_ref) of a band's stream, by the host parser and the reference's inverse."""
    import jpegx
    from pipeline.run_length_encoding import RunLengthEncoding
    n = cfg.dct_size
    rle = RunLengthEncoding(cfg)
    zz = jpegx.entropy_decode_n(blob, rle._height_in_blocks() * rle._width_in_blocks(), n * n)
    zz = zz.reshape(rle._height_in_blocks(), rle._width_in_blocks(), n * n)
    mode, param = cfg.quantization.gpu_mode()
    restored = crit.from_stream(zz, n).astype(np.float64) * (param if mode == "divide" else 1.0)
    return restored, crit.ref_idct(restored, n)


def _check_band(band, blob, cfg, what):
    """A decompressed band against the reference's unrounded samples: every sample is the clamped, rounded pooled sample
    it was replicated from."""
    from pipeline.geometry import band_geometry
    restored, x_ref = _pooled_reference(blob, cfg)
    (rows, cols), _, _, _ = band_geometry(cfg)
    bs, n = cfg.block_size, cfg.dct_size
    grow = lambda a: np.repeat(np.repeat(a, bs, axis=0), bs, axis=1)[:rows, :cols]            # noqa: E731
    t = grow(crit.tau_inv_plane(restored, n))
    want = grow(np.clip(x_ref, 0.0, 255.0))
    err = np.abs(np.asarray(band, dtype=np.float64) - want)
    print("%s: max|k-x| %.12f, mismatch share %.6f" % (what, float(err.max()), float(np.mean(band != np.round(want)))))
    assert band.shape == (rows, cols) and np.all(err <= 0.5 + t)


def test_readme_configuration_bytes_and_bands(gpu, monkeypatch):
    """block_size 5, dct_size 24, divide 1000 on a 203 x 317 band (both paddings ragged): the tie share is ~0 here, so
    the device road's bytes must be the host road's."""
    import pipeline
    cfg = _config(203, 317, 5, 24, "divide", divisor=1000)
    band = np.random.default_rng(5).integers(0, 256, (203, 317)).astype(np.uint8)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
    host_blob = pipeline.compress_band(band, cfg)
    host_band, host_u8 = pipeline.decompress_band(host_blob, cfg), pipeline.decompress_band_u8(host_blob, cfg)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 0)
    calls = []
    real = gpu.forward_fused_n
    monkeypatch.setattr(gpu, "forward_fused_n", lambda *a, **k: calls.append(1) or real(*a, **k))
    blob = pipeline.compress_band(band, cfg)
    assert calls == [1], "the device road did not run"
    assert isinstance(blob, bytes) and blob == host_blob
    dev_band, dev_u8 = pipeline.decompress_band(blob, cfg), pipeline.decompress_band_u8(blob, cfg)
    assert dev_band.dtype == host_band.dtype and dev_u8.dtype == np.uint8 and dev_u8.shape == host_u8.shape
    for got, what in ((dev_band, "device int"), (dev_u8, "device u8"), (host_band, "host int"), (host_u8, "host u8")):
        _check_band(got, blob, cfg, what)
    assert np.array_equal(dev_u8, dev_band.astype(np.uint8))


def test_dct_size_4_divide_40(gpu, monkeypatch):
    import pipeline
    cfg = _config(64, 64, 1, 4, "divide", divisor=40)
    band = np.random.default_rng(4).integers(0, 256, (64, 64)).astype(np.uint8)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 0)
    blob = pipeline.compress_band(band, cfg)
    zz = gpu.entropy_decode_n(blob, 256, 16).reshape(16, 16, 16)
    crit.check_forward(crit.from_stream(zz, 4), crit.ref_dct(band, 4), 4, "divide", 40.0, what="compress_band", cap=0.02)
    _check_band(pipeline.decompress_band(blob, cfg), blob, cfg, "device int")
    _check_band(pipeline.decompress_band_u8(blob, cfg), blob, cfg, "device u8")
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
    _check_band(pipeline.decompress_band(blob, cfg), blob, cfg, "host int")


def test_user_step_between_the_hot_steps(gpu, monkeypatch):
    """A step registered between BasisChange and Quantization: BasisChange runs stand-alone on the device, everything
    behind it on the host."""
    import pipeline
    from pipeline.base import AlgorithmStep, step_classes
    cfg = _config(60, 90, 1, 5, "divide", divisor=40)
    band = np.random.default_rng(9).integers(0, 256, (60, 90)).astype(np.uint8)
    stock = list(step_classes)
    try:
        class DampLastRows(AlgorithmStep):
            step_index = 4.5

            def execute(self, array):
                out = np.array(array, dtype=np.float64)
                out[4::5, :] *= 0.5
                return out

            def invert(self, array):
                out = np.array(array, dtype=np.float64)
                out[4::5, :] *= 2.0
                return out
        assert pipeline._hot_run(list(step_classes)) is None
        monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 0)
        stage, fused = [], []
        real = gpu.dct_f64_n
        monkeypatch.setattr(gpu, "dct_f64_n", lambda *a, **k: stage.append(1) or real(*a, **k))
        monkeypatch.setattr(gpu, "forward_fused_n", lambda *a, **k: fused.append(1))
        blob = pipeline.compress_band(band, cfg)
        assert stage == [1] and not fused
        zz = gpu.entropy_decode_n(blob, 12 * 18, 25).reshape(12, 18, 25)
        dct = crit.ref_dct(band, 5)
        dct[4::5, :] *= 0.5
        crit.check_forward(crit.from_stream(zz, 5), dct, 5, "divide", 40.0, what="user step", cap=0.02)
        back = pipeline.decompress_band(blob, cfg)
        monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
        host_back = pipeline.decompress_band(blob, cfg)
        restored = crit.from_stream(zz, 5).astype(np.float64) * 40.0
        restored[4::5, :] *= 2.0
        assert back.shape == host_back.shape == band.shape
        crit.check_inverse(back, restored, 5, what="user step, device", clamp=True)
        crit.check_inverse(host_back, restored, 5, what="user step, host", clamp=True)
    finally:
        step_classes[:] = stock


def test_jpeg_round_trip_at_dct_size_16(gpu, monkeypatch):
    import pipeline
    from PIL import Image
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 0)
    rng = np.random.default_rng(16)
    y, x = np.mgrid[0:70, 0:100]
    pixels = np.stack([(2 * x + y) % 256, (x + 3 * y) % 256, rng.integers(0, 256, (70, 100))], axis=2).astype(np.uint8)
    image = Image.fromarray(pixels, mode="YCbCr")
    cfg = _config(70, 100, 1, 16, "divide", divisor=40)      # ('none' cannot code a DC of 255 * 256: beyond 15 bits)
    calls = []
    real = gpu.forward_fused_n
    monkeypatch.setattr(gpu, "forward_fused_n", lambda *a, **k: calls.append(1) or real(*a, **k))
    data = pipeline.Jpeg(cfg).compress(image)
    assert len(calls) == 3
    back = np.asarray(pipeline.Jpeg.decompress(data))
    assert back.shape == pixels.shape and back.dtype == np.uint8
    import file_format
    cfg2, bands = file_format.read_data(data)
    assert (cfg2.dct_size, cfg2.height, cfg2.width) == (16, 70, 100)
    for i, blob in enumerate((bands.y, bands.cb, bands.cr)):
        _check_band(back[:, :, i], blob, cfg2, "Jpeg band %d" % i)
    # sanity against the picture: a coefficient moves by a uniform error of variance 40^2 / 12, a sample by that times
    # sum (Cn Cn Dinv Dinv)^2 <= (2 / 16)^2 (unit rows) = 2.08, plus 1 / 12 for its own rounding; the clamp only helps
    rms = float(np.sqrt(np.mean((back.astype(np.float64) - pixels) ** 2)))
    print("round trip rms error %.3f" % rms)
    assert rms <= np.sqrt(2.08 + 1.0 / 12.0)


def test_small_bands_stay_on_the_host_by_default(gpu, monkeypatch):
    import pipeline
    assert pipeline.DCTN_MIN_SAMPLES >= 1024

    def boom(*a, **k):
        raise AssertionError("a 4 x 4 band went to the device")
    for name in ("forward_fused_n", "inverse_fused_n", "dct_f64_n", "idct_f64_n", "entropy_encode_n", "entropy_decode_n"):
        monkeypatch.setattr(gpu, name, boom)
    cfg = _config(4, 4, 1, 2, "none")
    band = np.arange(16).reshape(4, 4)
    blob = pipeline.compress_band(band, cfg)
    assert np.array_equal(pipeline.decompress_band(blob, cfg), band)
    assert np.array_equal(pipeline.decompress_band_u8(blob, cfg), band.astype(np.uint8))


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_both_roads_against_the_recorded_reference_at_24(gpu, kind, monkeypatch):
    """tests/golden/dct_sizes.npz (the unmodified reference) at dct_size 24: the device entries, and the host step classes
    whose quantiser objects need a device at this size."""
    import os
    import pipeline
    from conftest import GOLDEN
    from pipeline.quantization import Quantization
    rec = np.load(os.path.join(GOLDEN, "dct_sizes.npz"))
    for n in (3, 4, 24):
        tag = "%d_%s" % (n, kind)
        pre, dct = rec["pre_" + tag], rec["dct_" + tag]
        for suffix, mode, param, kw in (("none", "none", 0.0, {}), ("discard2", "discard", 2.0, {"keep": 2}),
                                        ("divide40", "divide", 40.0, {"divisor": 40})):
            zz = gpu.forward_fused_n(pre, n, mode, param)
            crit.check_forward(crit.from_stream(zz, n), dct, n, mode, param, what="device " + tag, cap=0.02 if mode == "divide" else None)
            ref_zz = rec["zz_%s_%s" % (tag, suffix)]
            crit.check_inverse(gpu.inverse_fused_n(ref_zz, n, mode, param), rec["restore_%s_%s" % (tag, suffix)], n,
                               what="device " + tag, x_ref=rec["idctf_%s_%s" % (tag, suffix)])
            monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
            cfg = _config(pre.shape[0], pre.shape[1], 1, n, mode, **kw)
            crit.check_forward(Quantization(cfg).execute(dct), dct, n, mode, param, what="host " + tag, cap=0.02 if mode == "divide" else None)
