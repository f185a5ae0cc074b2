"""DCT sizes other than 8, the parts that need no device: the tables the kernels use, libjpegx's sequential entropy
coder for blocks of any length, argument validation, and the package's host road against arrays recorded from the
unmodified reference (tests/golden/dct_sizes.npz, written by tests/golden/make_golden_dct_sizes.py).  CPU only."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
import dctn_criterion as crit

SIZES = list(range(2, 33))


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("n", SIZES)
def test_tables_are_the_reference_matrices(n):
    """Observed on the build machine: C bit-identical to transforms.dct_matrix for every size (glibc cos == np.cos);
    the bound is 1 ulp in case a libm disagrees.  Cn and Dinv within 4 ulp (np.linalg.norm sums in BLAS order)."""
    import jpegx
    import transforms
    from pipeline.zigzag_order import Zigzag
    c, cn, dinv, zig = jpegx.dct_tables_n(n)
    want = transforms.dct_matrix(n)
    print("N=%d C bit-identical: %s" % (n, np.array_equal(c, want)))
    assert np.all(_ulps(c, want) <= 1.0)
    assert np.all(_ulps(cn, transforms.dct_matrix_normalized(n)) <= 4.0)
    assert np.all(_ulps(dinv, np.diag(transforms.normalization_matrix(n))) <= 4.0)
    assert np.array_equal(zig.astype(np.intp), Zigzag(n).flat_indices())


def _blocks(length, rng):
    """Streams of blocks of `length` coefficients that reach every branch of the coder."""
    rows = [np.zeros(length, np.int32), np.zeros(length, np.int32)]           # all-zero blocks
    last = np.zeros(length, np.int32)
    last[-1] = 5                                                              # lone last coefficient: chains of (15, 0, 0)
    rows.append(last)
    for run in (15, 16, 30, 31):                                              # runs of exactly these many zeros
        if run < length:
            b = np.zeros(length, np.int32)
            b[run] = -3
            rows.append(b)
            if run + 1 + run < length:
                b = b.copy()
                b[0] = 7
                b[run + 1 + run] = 2 if run + 1 + run != run else 0
                rows.append(b)
    for amp in (1, -1, 16383, -16383):
        b = np.zeros(length, np.int32)
        b[0], b[min(2, length - 1)] = amp, -amp
        rows.append(b)
    full = rng.integers(-300, 301, length).astype(np.int32)                   # every coefficient set
    full[full == 0] = 1
    rows.append(full)
    for _ in range(6):
        b = rng.integers(-40, 41, length).astype(np.int32)
        b[rng.random(length) < 0.8] = 0
        rows.append(b)
    return np.stack(rows).reshape(1, len(rows), length)


def _config(nblocks, n):
    import pipeline
    return pipeline.Configuration(width=nblocks * n, height=n, block_size=1, dct_size=n)


@pytest.mark.parametrize("n", [2, 3, 4, 8, 17, 24, 32])
def test_entropy_coder_equals_the_step_classes(n):
    import jpegx
    from pipeline.rle_byte_stream import RleBytestream
    from pipeline.run_length_encoding import RunLengthEncoding
    zz = _blocks(n * n, np.random.default_rng(n))
    cfg = _config(zz.shape[1], n)
    want = RleBytestream(cfg).execute(RunLengthEncoding(cfg).execute(zz))
    got = jpegx.entropy_encode_n(zz)
    assert isinstance(got, bytes) and got == want
    back = jpegx.entropy_decode_n(got, zz.shape[1], n * n)
    assert back.dtype == np.int32 and np.array_equal(back.reshape(zz.shape), zz)
    assert np.array_equal(RunLengthEncoding(cfg).invert(RleBytestream(cfg).invert(got)), zz)


@pytest.mark.parametrize("n", [2, 3, 8, 24])
def test_an_amplitude_beyond_15_bits_is_the_references_error(n):
    import jpegx
    import util
    from pipeline.run_length_encoding import RunLengthEncoding
    zz = np.zeros((1, 2, n * n), np.int32)
    zz[0, 1, 1] = 16384
    with pytest.raises(jpegx.JpegxError, match="BadRleCodeError"):
        jpegx.entropy_encode_n(zz)
    with pytest.raises(util.BadRleCodeError):
        RunLengthEncoding(_config(2, n)).execute(zz)
    zz[0, 1, 1] = -16383
    assert len(jpegx.entropy_encode_n(zz)) == 1 + 4


MALFORMED_64 = {
    "truncated inside a block": bytes([0x02, 0xC0]),
    "truncated amplitude": bytes([0x0F]),
    "bytes behind the last block": bytes([0x00, 0x00]),
    "zero chain overruns": bytes([0xF0] * 5 + [0x00]),
    "run overruns": bytes([0xF0] * 4 + [0x52, 0xC0, 0x00]),
    "size 1": bytes([0x01, 0x80, 0x00]),
    "non-terminal run with size 0": bytes([0x30, 0x00]),
    "empty": b"",
}


@pytest.mark.parametrize("name", sorted(MALFORMED_64))
def test_malformed_streams_are_refused_like_the_64_form(name):
    import jpegx
    blob = MALFORMED_64[name]
    with pytest.raises(jpegx.JpegxError) as old:
        jpegx.entropy_decode(blob, 1)
    with pytest.raises(jpegx.JpegxError) as new:
        jpegx.entropy_decode_n(blob, 1, 64)
    assert str(new.value).split(": ", 1)[1] == str(old.value).split(": ", 1)[1]


def test_malformed_streams_other_lengths():
    import jpegx
    for blob, length, text in ((bytes([0xF0, 0x00]), 9, "zero chain overruns"), (bytes([0x92, 0xC0, 0x00]), 9, "run overruns"),
                               (bytes([0x42, 0xC0, 0x00]), 4, "run overruns"), (bytes([0x02, 0xC0]), 576, "ends inside a block"),
                               (bytes([0x00, 0x00, 0x00]), 4, "ValueError")):
        with pytest.raises(jpegx.JpegxError, match=text):
            jpegx.entropy_decode_n(blob, 2 if text == "ValueError" else 1, length)
    assert np.array_equal(jpegx.entropy_decode_n(bytes([0x82, 0xC0, 0x00]), 1, 9), [[0] * 8 + [1]])


def test_arguments_are_checked_before_any_device_work():
    import jpegx
    L = jpegx.lib()
    buf = ctypes.create_string_buffer(64 * 64 * 8)
    p = ctypes.addressof(buf)
    err = lambda: L.jpegx_last_error()                                                        # noqa: E731
    assert L.jpegx_host_forward_fused_n(p, 8, 8, 1, 0, 0.0, p) == -1 and b"2 .. 32" in err()
    assert L.jpegx_host_forward_fused_n(p, 33, 33, 33, 0, 0.0, p) == -1 and b"2 .. 32" in err()
    assert L.jpegx_host_forward_fused_n(p, 6, 6, 3, 3, 0.0, p) == -1 and b"qtable" in err()
    assert L.jpegx_host_forward_fused_n(p, 7, 6, 3, 0, 0.0, p) == -1 and b"multiples of dct_size" in err()
    assert L.jpegx_host_forward_fused_n(p, 6, 7, 3, 0, 0.0, p) == -1
    assert L.jpegx_host_forward_fused_n(None, 6, 6, 3, 0, 0.0, p) == -1 and b"null" in err()
    assert L.jpegx_host_forward_fused_n(p, 6, 6, 3, 1, -1.0, p) == -1
    assert L.jpegx_host_forward_fused_n(p, 6, 6, 3, 2, 0.0, p) == -1
    assert L.jpegx_host_forward_fused_n(p, 6, 6, 3, 9, 0.0, p) == -1
    assert L.jpegx_host_inverse_fused_n(p, 6, 6, 3, 3, 0.0, 0, p, 6) == -1 and b"qtable" in err()
    assert L.jpegx_host_inverse_fused_n(p, 6, 6, 1, 0, 0.0, 0, p, 6) == -1
    assert L.jpegx_host_inverse_fused_n(p, 6, 6, 3, 0, 0.0, 0, p, 5) == -1 and b"pitch" in err()
    assert L.jpegx_host_inverse_fused_n(p, 6, 6, 3, 0, 0.0, 0, None, 6) == -1
    assert L.jpegx_host_dct_f64_n(p, 10, 6, 3, p) == -1 and L.jpegx_host_idct_f64_n(p, 6, 6, 40, p, 1) == -1
    # the device-pointer entries run the same checks first
    assert L.jpegx_forward_fused_n(p, 6, 6, 6, 33, 0, 0.0, p, None) == -1
    assert L.jpegx_forward_fused_n(p, 6, 6, 5, 3, 0, 0.0, p, None) == -1 and b"pitch" in err()
    assert L.jpegx_inverse_fused_n(p, 6, 6, 3, 3, 0.0, 0, p, 6, None) == -1
    assert L.jpegx_dct_f64_n(p, 6, 8, 8, 3, p, 8, None) == -1 and L.jpegx_idct_f64_n(None, 6, 6, 6, 3, p, 6, 1, None) == -1
    one = np.zeros(4)
    assert L.jpegx_dct_tables_n(1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data) == -1
    n = ctypes.c_size_t(0)
    assert L.jpegx_host_entropy_encode_n(p, 1, 0, None, 0, ctypes.byref(n)) == -1
    assert L.jpegx_host_entropy_encode_n(None, 1, 4, None, 0, ctypes.byref(n)) == -1
    assert L.jpegx_host_entropy_decode_n(p, 1, 0, 4, p) == -1
    assert L.jpegx_version() >= 200


def test_small_planes_stay_on_the_host_and_the_threshold_is_public():
    import pipeline
    assert isinstance(pipeline.DCTN_MIN_SAMPLES, int) and pipeline.DCTN_MIN_SAMPLES > 0
    cfg = pipeline.Configuration(width=4, height=4, block_size=1, dct_size=2)
    assert not pipeline.dctn_on_device(cfg, 16)


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, "dct_sizes.npz"))


QUANT = [("none", "none", 0.0), ("discard2", "discard", 2.0), ("divide40", "divide", 40.0)]


def _quantise(cfg, dct, n, mode, param):
    """Quantization.execute -- except for sizes that are multiples of 8: there the stock quantiser objects hand every
    n x n block to libjpegx's float64 quantiser kernel (quantizers.py, any 2-D float array of whole 8 x 8 tiles), which
    needs a device; this CPU test then applies the same formulae (quantizers.py:4-31) itself.  test_gpu_dct_sizes.py
    runs the step class for that size."""
    from pipeline.quantization import Quantization
    if n % 8:
        return Quantization(cfg).execute(dct)
    v, _ = crit.quantiser_value(dct, n, mode, param)
    return np.round(v)


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("n", [3, 4, 24])
def test_host_road_against_the_recorded_reference(recorded, n, kind):
    """The package's NumPy road for these sizes (planes far below DCTN_MIN_SAMPLES, so no device is involved) against
    what the unmodified reference produced, under the criterion of dctn_criterion.py."""
    import pipeline
    from pipeline.basis_change import BasisChange
    from pipeline.quantization import Quantization
    from pipeline.zigzag_order import ZigzagOrder
    tag = "%d_%s" % (n, kind)
    pre, dct = recorded["pre_" + tag], recorded["dct_" + tag]
    assert np.abs(crit.ref_dct(pre, n) - dct).max() <= crit.tau(n)          # the criterion's own reference vs the recording
    for suffix, mode, param in QUANT:
        kw = {"keep": int(param)} if mode == "discard" else ({"divisor": param} if mode == "divide" else {})
        cfg = pipeline.Configuration(width=pre.shape[1], height=pre.shape[0], block_size=1, dct_size=n,
                                     quantization=pipeline.QuantizationMethod(mode, **kw))
        got_dct = BasisChange(cfg).execute(pre)
        assert np.abs(got_dct - dct).max() <= crit.tau(n)
        q = _quantise(cfg, got_dct, n, mode, param)
        crit.check_forward(q, dct, n, mode, param, what="host " + tag, cap=0.02 if mode == "divide" else None)
        zz = ZigzagOrder(cfg).execute(q)
        assert np.array_equal(zz, crit.to_stream(q, n))
        assert np.array_equal(crit.to_stream(recorded["q_%s_%s" % (tag, suffix)], n), recorded["zz_%s_%s" % (tag, suffix)])
        # inverse, fed with the REFERENCE's stream
        ref_zz = recorded["zz_%s_%s" % (tag, suffix)]
        rest = Quantization(cfg).invert(ZigzagOrder(cfg).invert(ref_zz)) if n % 8 else \
            ZigzagOrder(cfg).invert(ref_zz) * (param if mode == "divide" else 1)
        assert np.array_equal(rest, recorded["restore_%s_%s" % (tag, suffix)])
        back = BasisChange(cfg).invert(rest)
        crit.check_inverse(back, rest, n, what="host " + tag, x_ref=recorded["idctf_%s_%s" % (tag, suffix)])
        crit.check_inverse(recorded["idct_%s_%s" % (tag, suffix)], rest, n, what="recorded " + tag)
