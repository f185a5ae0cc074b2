"""The dct_size-N kernels (csrc/jpegx_dctn.hip) on the inputs of tests/adversarial_dctn.py: every size 2 .. 32 on a
layout that reaches each launch hazard of that size, the rounding rule (half to even) pinned where the value before
rounding is exact in any summation order, non-finite and huge samples beside ordinary blocks, saturation to int32, and
the branches of the pipeline road that need a device.  Every comparison is exact equality on values
tests/test_adversarial_dctn.py shows to be exact, or the criterion of dctn_criterion.py as it stands."""
import numpy as np
import pytest

import adversarial_dctn as ad
import dctn_criterion as crit
from dctn_dev import dct_f64_dev, forward_dev, idct_f64_dev, inverse_dev

pytestmark = pytest.mark.gpu

ALL_N = pytest.mark.parametrize("n", ad.SIZES)
HOST_ONLY = 1 << 62
SIGNED_PEAK = 300.0


def quantisers(n):
    return [("none", 0.0), ("discard", 1.0), ("discard", float(n))] + [("divide", d) for d in (40.0, 0.75, -7.0, 2.0, 0.5)]


def planes_of(n):
    """(name, plane, peak): integer noise, quarter-integer (block_size 2 pooling) and signed fractional samples."""
    h, w, _ = ad.layout(n)
    rng = np.random.default_rng(7000 + n)
    noise = rng.integers(0, 256, (h, w)).astype(np.float64)
    pooled = rng.integers(0, 256, (2 * h, 2 * w)).astype(np.float64).reshape(h, 2, w, 2).mean(axis=(1, 3))
    signed = rng.uniform(-SIGNED_PEAK, SIGNED_PEAK, (h, w))
    return [("noise", noise, 255.0), ("pooled", pooled, 255.0), ("signed", signed, SIGNED_PEAK)]


def references(n, plane):
    """The reference's coefficients: transforms.DCT on the CPU; at N = 8 also the CPU oracle of the 8 x 8 road."""
    refs = [("reference", ad.ref_dct(plane, n), lambda r: ad.ref_idct(r, n))]
    if n == 8:
        import oracle
        refs.append(("oracle", oracle.dct_plane(plane), lambda r: oracle.idct_plane(r, rounded=False)))
    return refs


@ALL_N
def test_every_size_every_entry(gpu, n):
    h, w, pitch = ad.layout(n)
    worst = {"forward": (0.0, 0.0), "inverse": (0.0, 0.0)}
    for name, plane, peak in planes_of(n):
        for ref_name, dct, idct in references(n, plane):
            what = "%s %s %dx%d" % (ref_name, name, h, w)
            coef = dct_f64_dev(gpu, plane, n, pitch=pitch, out_pitch=w + 7)
            assert np.abs(coef - dct).max() <= crit.tau(n, peak=peak)
            x_ref, t = idct(dct), crit.tau_inv_plane(dct, n)
            back = idct_f64_dev(gpu, dct, n, False, pitch=pitch, out_pitch=w + 1)
            assert np.all(np.abs(back - x_ref) <= t)
            crit.check_inverse(idct_f64_dev(gpu, dct, n, True, pitch=pitch, out_pitch=w + 5), dct, n, what="idct_f64_n " + what, x_ref=x_ref)
            for mode, param in quantisers(n):
                zz = forward_dev(gpu, plane, n, mode, param, pitch)
                assert zz.dtype == np.int32 and zz.shape == (h // n, w // n, n * n)
                res = crit.check_forward(crit.from_stream(zz, n), dct, n, mode, param, what=what, peak=peak)
                worst["forward"] = max(worst["forward"], res)
                # the inverse on the stream the REFERENCE's forward gives
                v, _ = crit.quantiser_value(dct, n, mode, param)
                ref_zz = crit.to_stream(np.round(v), n).astype(np.int32)
                restored = crit.from_stream(ref_zz, n).astype(np.float64) * (param if mode == "divide" else 1.0)
                x_ref = idct(restored)
                tag = "%s %s %g" % (what, mode, param)
                got = inverse_dev(gpu, ref_zz, n, mode, param, out_pitch=w + 3)
                res = crit.check_inverse(got, restored, n, what=tag, x_ref=x_ref)
                worst["inverse"] = max(worst["inverse"], res)
                u8 = inverse_dev(gpu, ref_zz, n, mode, param, u8=True, out_pitch=w + 5)
                crit.check_inverse(u8, restored, n, what=tag + " u8", clamp=True, x_ref=x_ref)
                assert np.array_equal(u8, np.clip(got, 0, 255).astype(np.uint8))            # the clamp, exactly
    print("N=%d worst (mismatch share, tie share): forward %.5f %.5f, inverse %.5f %.5f"
          % ((n,) + worst["forward"] + worst["inverse"]))


# ---- the rounding rule ----------------------------------------------------------------------------------------------------
@ALL_N
def test_forward_rounds_exact_dc_ties_half_to_even(gpu, n):
    tie_blocks = blocks = 0
    for signed in (False, True):
        for q in ad.TIE_DIVISORS:
            t = ad.dc_tie_plane(n, q, signed)
            dct = ad.ref_dct(t.plane, n)
            assert np.array_equal(ad.dc_of(gpu.dct_f64_n(t.plane, n), n), t.sums)           # DC is the block sum, exactly
            modes = [("none", 0.0), ("discard", float(n)), ("discard", 1.0)] if q == 1.0 else [("divide", q)]
            for mode, param in modes:
                zz = gpu.forward_fused_n(t.plane, n, mode, param)
                bad = zz[:, :, 0] != t.dc
                assert not bad.any(), (n, mode, param, signed, t.sums[bad][:4], zz[:, :, 0][bad][:4], t.dc[bad][:4])
                crit.check_forward(crit.from_stream(zz, n), dct, n, mode, param, what="dc ties, signed %s" % signed)
            tie_blocks += int(t.ties.sum())
            blocks += t.ties.size
    print("N=%d exact DC ties: %d of %d blocks" % (n, tie_blocks, blocks))


@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("mode,param", [("none", 0.0), ("divide", 2.0), ("divide", 0.5)])
def test_inverse_rounds_exact_sample_ties_half_to_even(gpu, n, mode, param):
    zz, m = ad.inverse_tie_stream(n, mode, param)
    w = zz.shape[1] * n
    x = np.repeat(np.repeat(m + 0.5, n, axis=0), n, axis=1)
    want = np.round(x)
    assert want.min() < 0 and np.any(want != np.floor(x + 0.5))
    got = inverse_dev(gpu, zz, n, mode, param, out_pitch=w + 3)
    assert got.dtype == np.int32 and np.array_equal(got, want.astype(np.int32))
    assert np.array_equal(gpu.inverse_fused_n(zz, n, mode, param), got)
    u8 = inverse_dev(gpu, zz, n, mode, param, u8=True, out_pitch=w + 5)
    assert np.array_equal(u8, np.clip(want, 0, 255).astype(np.uint8))                       # -0.5 -> 0, 254.5 -> 254, 255.5 -> 255
    for mm, k in ((-1, 0), (254, 254), (255, 255)):
        assert set(u8[x == mm + 0.5].tolist()) == {k}
    restored = crit.from_stream(zz, n).astype(np.float64) * (param if mode == "divide" else 1.0)
    assert np.array_equal(gpu.idct_f64_n(restored, n, do_round=False), x)
    assert np.array_equal(gpu.idct_f64_n(restored, n, do_round=True), want)


# ---- containment and saturation -------------------------------------------------------------------------------------------
CONTAINED = [2, 3, 5, 11, 12, 17, 32]


def _others(a, n, wb, block, stream=False):
    """Everything but one block, of a plane or of a (hb, wb, n*n) stream."""
    if stream:
        return np.delete(a.reshape(-1, n * n), block, axis=0)
    mask = np.ones(a.shape, bool)
    mask[ad.block_slices(n, wb, block)] = False
    return a[mask]


@pytest.mark.parametrize("n", CONTAINED)
def test_non_finite_and_huge_samples_stay_inside_their_block(gpu, n):
    h, w, pitch = ad.layout(n)
    hb, wb = h // n, w // n
    clean = np.random.default_rng(n).integers(0, 256, (h, w)).astype(np.float64)
    for block in ad.poison_blocks(n, hb, wb):
        z = ad.zeroed(clean, n, block)
        quant = (("none", 0.0), ("divide", 1e-9), ("divide", 40.0))
        base_zz = {q: forward_dev(gpu, z, n, q[0], q[1], pitch) for q in quant}
        base_coef, base_back = gpu.dct_f64_n(z, n), gpu.idct_f64_n(z, n, do_round=False)
        for what in ad.POISONS:
            p = ad.poisoned(clean, n, block, what)
            for q in quant:
                zz = forward_dev(gpu, p, n, q[0], q[1], pitch)
                assert np.array_equal(_others(zz, n, wb, block, True), _others(base_zz[q], n, wb, block, True)), (block, what, q)
                own = zz.reshape(-1, n * n)[block]
                if what.startswith("huge") and q[1] != 40.0:
                    # every coefficient of such a block is beyond 2^40 (asserted on the CPU): all of it saturates, by sign
                    coef = ad.ref_dct(p[ad.block_slices(n, wb, block)], n) / (q[1] if q[0] == "divide" else 1.0)
                    sat = np.where(crit.to_stream(coef, n)[0, 0] > 0, ad.INT32_MAX, ad.INT32_MIN)
                    assert own[0] == (ad.INT32_MAX if what == "huge+" else ad.INT32_MIN)
                    assert np.array_equal(own, sat), (block, what, q)
                if what in ("1e300", "+inf"):
                    assert own[0] == ad.INT32_MAX
                if what == "-inf":
                    assert own[0] == ad.INT32_MIN
            assert np.array_equal(_others(gpu.dct_f64_n(p, n), n, wb, block), _others(base_coef, n, wb, block)), (block, what)
            assert np.array_equal(_others(gpu.idct_f64_n(p, n, do_round=False), n, wb, block), _others(base_back, n, wb, block)), (block, what)


@pytest.mark.parametrize("n", CONTAINED)
def test_inverse_saturates_and_keeps_it_inside_the_block(gpu, n):
    """Amplitudes of +-(2^31 - 1) under `divide 1e30`: samples of the order 1e39.  Where the reference's sample is beyond
    1e30 -- far beyond any summation error, which is below 1e-12 of the block's 1-norm -- the output is the saturated
    value of its sign; every other block is what it is with that block zeroed."""
    h, w, _ = ad.layout(n)
    hb, wb = h // n, w // n
    rng = np.random.default_rng(31 + n)
    zz = rng.integers(-50, 51, (hb, wb, n * n)).astype(np.int32)
    for block in ad.poison_blocks(n, hb, wb):
        dirty, zero = zz.copy(), zz.copy()
        dirty.reshape(-1, n * n)[block] = np.where(rng.random(n * n) < 0.5, ad.INT32_MAX, -ad.INT32_MAX)
        zero.reshape(-1, n * n)[block] = 0
        sl = ad.block_slices(n, wb, block)
        x_ref = ad.ref_idct(crit.from_stream(dirty, n).astype(np.float64)[sl] * 1e30, n)
        sure = np.abs(x_ref) >= 1e30
        assert sure.mean() > 0.9
        for u8 in (False, True):
            got = inverse_dev(gpu, dirty, n, "divide", 1e30, u8=u8, out_pitch=w + 3)
            base = inverse_dev(gpu, zero, n, "divide", 1e30, u8=u8, out_pitch=w + 3)
            assert np.array_equal(_others(got, n, wb, block), _others(base, n, wb, block)), (block, u8)
            hi, lo = (255, 0) if u8 else (ad.INT32_MAX, ad.INT32_MIN)
            assert np.array_equal(got[sl][sure], np.where(x_ref > 0, hi, lo)[sure]), (block, u8)


# ---- pipeline roads -------------------------------------------------------------------------------------------------------
def _config(h, w, bs, n, mode, **kw):
    import pipeline
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n, quantization=pipeline.QuantizationMethod(mode, **kw))


def _count(monkeypatch, gpu, name):
    calls = []
    real = getattr(gpu, name)
    monkeypatch.setattr(gpu, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.parametrize("n,bs", ad.FLAT_PAIRS)
@pytest.mark.parametrize("mode,kw,q", [("none", {}, 1.0), ("divide", {"divisor": 2}, 2.0)])
def test_both_roads_give_the_same_bytes_on_exact_ties(gpu, monkeypatch, n, bs, mode, kw, q):
    """Bands whose whole stream is determined exactly (flat_tiles_band): the device road's bytes are the host road's, and
    the stream is the exact one -- the same picture content codes to the same bytes whichever road its size selects."""
    import pipeline
    f = ad.flat_tiles_band(n, bs)
    cfg = _config(f.height, f.width, bs, n, mode, **kw)
    band = np.array(f.band)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
    host_blob = pipeline.compress_band(band, cfg)
    host_band, host_u8 = pipeline.decompress_band(host_blob, cfg), pipeline.decompress_band_u8(host_blob, cfg)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 0)
    fwd, inv = _count(monkeypatch, gpu, "forward_fused_n"), _count(monkeypatch, gpu, "inverse_fused_n")
    blob = pipeline.compress_band(band, cfg)
    assert fwd == [1], "the device road did not run"
    dc, ties = ad.flat_tiles_dc(n, bs, q)
    zz = gpu.entropy_decode_n(blob, f.hb * f.wb, n * n).reshape(f.hb, f.wb, n * n)
    assert np.array_equal(zz[:, :, 0], dc) and not np.any(zz[:, :, 1:])
    print("N=%d bs=%d %s: %d of %d blocks are exact DC ties" % (n, bs, mode, int(ties.sum()), ties.size))
    assert isinstance(blob, bytes) and blob == host_blob
    dev_band, dev_u8 = pipeline.decompress_band(blob, cfg), pipeline.decompress_band_u8(blob, cfg)
    assert inv == [1, 1]
    assert dev_band.shape == host_band.shape == f.band.shape and dev_band.dtype == host_band.dtype
    assert np.array_equal(dev_band, host_band)
    assert dev_u8.dtype == host_u8.dtype == np.uint8 and np.array_equal(dev_u8, host_u8)
    assert np.array_equal(dev_u8, dev_band.astype(np.uint8))


def test_an_amplitude_beyond_15_bits_on_the_device_road(gpu, monkeypatch):
    """N = 16, `none`, a block of 255s: DC = 65280.  The device road runs, the native coder refuses the amplitude and the
    host steps raise the reference's error."""
    import pipeline
    import util
    cfg = _config(64, 64, 1, 16, "none")
    band = np.random.default_rng(16).integers(0, 40, (64, 64)).astype(np.uint8)
    band[16:32, 32:48] = 255
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
    with pytest.raises(util.BadRleCodeError):
        pipeline.compress_band(band, cfg)
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 0)
    calls = _count(monkeypatch, gpu, "forward_fused_n")
    with pytest.raises(util.BadRleCodeError):
        pipeline.compress_band(band, cfg)
    assert calls == [1], "the device road did not run"
    zz = pipeline._hot_forward_n(band, cfg)
    assert zz[1, 2, 0] == 255 * 256


@pytest.mark.parametrize("mode,kw,scale", [("none", {}, 1.0), ("divide", {"divisor": 0.5}, 2.0), ("divide", {"divisor": -40}, 1.0)])
def test_the_reach_guard_of_the_forward_road(gpu, monkeypatch, mode, kw, scale):
    """_hot_forward_n keeps a plane whose coefficients could leave int32 on the host: reach = max|x| N^2 / min(|d|, 1)
    at or above 2^31 returns None, the largest double below runs on the device."""
    import pipeline
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 0)
    n = 4
    cfg = _config(32, 48, 1, n, mode, **kw)
    edge = 2.0 ** 27 / scale                                            # edge * 16 * scale == 2^31
    rng = np.random.default_rng(27)
    plane = rng.uniform(-edge / 2, edge / 2, (32, 48))
    calls = _count(monkeypatch, gpu, "forward_fused_n")
    for top in (edge, -edge, edge * 1.5, np.nan, np.inf):
        p = plane.copy()
        p[5, 7] = top
        assert pipeline._hot_forward_n(p, cfg) is None
    assert not calls
    param = float(kw.get("divisor", 0.0))
    below = np.nextafter(edge, 0.0)
    for top in (below, -below):                                         # one sample just below: on the device
        p = plane.copy()
        p[5, 7] = top
        zz = pipeline._hot_forward_n(p, cfg)
        assert zz is not None and zz.dtype == np.int32
        crit.check_forward(crit.from_stream(zz, n), crit.ref_dct(p, n), n, mode, param, what="reach %g" % top, peak=edge)
    assert calls == [1, 1]
    # a whole block just below: under `none` and `divide 0.5` its DC is +-(2^31 - 2^-22), which rounds to +-2^31.  The
    # negative one is an int32; the positive one is not, the kernel saturates it, and the road must not hand that out
    for top in (below, -below):
        p = plane.copy()
        p[4:8, 4:8] = top
        dct = crit.ref_dct(p, n)
        v, _ = crit.quantiser_value(dct, n, mode, param)
        assert dct[4, 4] == 16 * top
        zz = pipeline._hot_forward_n(p, cfg)
        if np.round(v).max() > ad.INT32_MAX:
            assert zz is None, "a saturated coefficient left the device road"
        else:
            crit.check_forward(crit.from_stream(zz, n), dct, n, mode, param, what="reach, block of %g" % top, peak=edge)
            assert zz[1, 1, 0] == np.round(v[4, 4])
    assert len(calls) == 4


def test_the_inverse_road_takes_integral_streams_of_any_dtype(gpu, monkeypatch):
    import pipeline
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 0)
    n = 5
    cfg = _config(35, 45, 1, n, "divide", divisor=3)
    zz = np.random.default_rng(5).integers(-90, 91, (7, 9, 25)).astype(np.int32)
    want = pipeline._hot_inverse_n(zz, cfg)
    assert want is not None and want.shape == (35, 45) and want.dtype == np.dtype(int)
    assert np.array_equal(want, gpu.inverse_fused_n(zz, n, "divide", 3.0))
    for other in (zz.astype(np.int64), zz.astype(np.float64), zz.astype(np.int16), zz.astype(np.float32)):
        got = pipeline._hot_inverse_n(other, cfg)
        assert got is not None and got.dtype == want.dtype and np.array_equal(got, want)
    calls = _count(monkeypatch, gpu, "inverse_fused_n")
    frac = zz.astype(np.float64)
    frac[3, 4, 7] += 0.5
    assert pipeline._hot_inverse_n(frac, cfg) is None
    big = zz.astype(np.int64)
    big[0, 0, 0] = 2 ** 31
    assert pipeline._hot_inverse_n(big, cfg) is None
    assert pipeline._hot_inverse_n(zz.astype(np.float64) * np.nan, cfg) is None
    assert not calls
