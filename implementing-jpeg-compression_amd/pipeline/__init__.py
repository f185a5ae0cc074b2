"""Codec facade and configuration with the reference's names (reference: pipeline/__init__.py).

``compress_band`` / ``decompress_band`` walk the registered steps like the reference, except
that for the accelerated configuration (transform 'DCT', dct_size 8) the three hot steps --
BasisChange, Quantization, ZigzagOrder -- are replaced by ONE fused GPU kernel launch
(libjpegx ``jpegx_forward_fused`` / ``jpegx_inverse_fused``) whose integer output is bit-exact
with the step-by-step float64 pipeline.  There is no CPU fallback for the accelerated
configuration: without libjpegx.so or a GPU the call raises ``jpegx.JpegxError``.

Any other dct_size 2..32 with transform 'DCT' takes the all-float64 kernels of csrc/jpegx_dctn.hip
(``jpegx_forward_fused_n`` / ``jpegx_inverse_fused_n``, entropy stage by libjpegx's sequential host coder; with
``DCTN_ENTROPY_MIN_SAMPLES`` set, compressing runs the entropy stage on the device behind the forward kernel,
csrc/jpegx_entropy_n.hip; with ``DCTN_ENTROPY_DECODE_MIN_SAMPLES`` set, decompressing runs the entropy decoder on the
device in front of the inverse kernel, csrc/jpegx_entropy_decode_n.hip; planes of at least
``DCTN_BAND_JOB_MIN_SAMPLES`` samples compress as one device job from the band's 8-bit samples, steps 0-3 included,
csrc/jpegx_band_n.hip; with ``DCTN_BAND_DECODE_JOB_MIN_SAMPLES`` set, decompressing is one device job down to the band's
samples, the geometry steps a scatter kernel of the same file; Jpeg.compress / Jpeg.decompress on three-band 8-bit pictures
are one device job each from ``DCTN_IMAGE_JOB_MIN_SAMPLES`` / ``DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES`` samples per plane on) when a
device is usable and the plane holds at least ``DCTN_MIN_SAMPLES`` samples; otherwise -- unlike dct_size 8 -- the host
NumPy road runs, exactly as the reference does it.
"""
import json
import operator

import numpy as np

import file_format
from quantizers import DiscardingQuantizer, DivisionQuantizer, JpegQuantizationTable, RoundingQuantizer
from util import band_to_array
from . import (basis_change, dct_padding, geometry, normalization, padding, quantization,  # noqa: F401  (registration)
               rle_byte_stream, run_length_encoding, subsampling, zigzag_order)
from .base import step_classes


class BadQuantizationError(Exception):
    pass


class QuantizationMethod:
    """Named quantiser + its keyword parameters (pipeline/__init__.py:13-47)."""
    name_to_quantizer = {
        "none": RoundingQuantizer,
        "discard": DiscardingQuantizer,
        "divide": DivisionQuantizer,
        "qtable": JpegQuantizationTable,
    }

    def __init__(self, name, **kwargs):
        self.name = name
        self.params = kwargs
        self.quantizer = self._get_quantizer()

    def _get_quantizer(self):
        error_msg = "name {}, params {}".format(self.name, self.params)
        factory = self.name_to_quantizer.get(self.name)
        if factory is None:
            raise BadQuantizationError(error_msg)
        try:
            return factory(**self.params)
        except Exception:
            raise BadQuantizationError(error_msg)

    def to_json(self):
        d = dict(self.params)
        d["quantization_scheme_name"] = self.name
        return json.dumps(d)

    @staticmethod
    def from_json(s):
        d = json.loads(s)
        name = d.pop("quantization_scheme_name")
        return QuantizationMethod(name, **d)

    def gpu_mode(self):
        """(mode name, scalar parameter) understood by libjpegx, or None if not expressible.  Only the STOCK
        quantiser objects qualify: a replaced or subclassed quantiser, or an edited luminance table, is a
        different function and goes through the object's own quantize/restore like in the reference."""
        q = self.quantizer
        if type(q) is not self.name_to_quantizer.get(self.name):
            return None
        if self.name == "discard":
            return ("discard", float(q.keep)) if isinstance(q.keep, (int, np.integer)) and q.keep >= 0 else None
        if self.name == "divide":
            try:
                d = float(q.divisor)
            except (TypeError, ValueError):
                return None
            return ("divide", d) if d != 0 and np.isfinite(d) else None
        if self.name == "qtable":
            stock = np.array(JpegQuantizationTable.table)
            same = np.array_equal(np.asarray(q.table), stock) and np.array_equal(getattr(q, "_qtable", stock), stock)
            return ("qtable", 0.0) if same else None
        return ("none", 0.0) if self.name == "none" else None


class Configuration:
    """pipeline/__init__.py:50-64"""

    def __init__(self, width, height, block_size=2, dct_size=8, transform="DCT", quantization=None):
        self.width = width
        self.height = height
        self.block_size = block_size
        self.dct_size = dct_size
        self.transform = transform
        if quantization is None:
            quantization = QuantizationMethod("none")
        elif quantization.name == "qtable" and dct_size != 8:
            raise BadQuantizationError()
        self.quantization = quantization


# dct_size other than 8: planes below this many samples stay on the host NumPy road.  Measured (DESIGN.md 4.7,
# profiles/dct_sizes.json): at 1024 samples, the smallest plane measured, the device road already takes 0.06-0.13 ms
# against 1.0-1.2 ms on the host, and its lead only grows with the plane; below that nothing was measured, and planes
# of a few blocks are what unit tests and a machine's first steps with the step classes use
DCTN_MIN_SAMPLES = 1024

# The device entropy stage behind the forward kernel as one job (jpegx.compress_plane_n): planes of at least this many
# samples take it; None: the job road is off and compress_band keeps jpegx_forward_fused_n + the host coder.  Measured
# (profiles/dctn_entropy.json): the job road is 5-7x faster on a 3000 x 4000 band and wins from 16384 samples
# on, loses 13-17 us below, and lost 3 % at one N = 24 size above -- so it is not the default; 16384 is the value to set.
DCTN_ENTROPY_MIN_SAMPLES = None

# The way back as one device job (jpegx.decompress_plane_n: the run-time block length entropy decoder of
# csrc/jpegx_entropy_decode_n.hip + the inverse kernel, the coefficient stream never on the host): planes of at least this
# many samples take it; None: the job road is off and decompress_band keeps the host parser + jpegx_inverse_fused_n.
# Measured (profiles/dctn_decode.json): on a 3000 x 4000 band at block_size 1 decompress_band_u8 takes 1.5 ms
# instead of 45-47 ms (30x) and decompress_band 48 instead of 93 ms; from 262 144 samples on the job road was no slower
# than the parent's at every measured configuration (N = 4, 16: 4-7x faster there; N = 24 with divisor 1000, 16 KB of code:
# equal within 1 %), below that its launches cost more than the host parser saves -- at N = 24 up to 147 456 samples, at
# N = 16 up to 36 864, at N = 4 up to 16 384.  Hence the smallest measured size with no miss at or above it.
DCTN_ENTROPY_DECODE_MIN_SAMPLES = 262144

# compress_band for dct_size other than 8 as ONE device job from the band's 8-bit samples (jpegx.compress_band_n: the band
# up as bytes, steps 0-3 as the kernel of csrc/jpegx_band_n.hip, then the launches of jpegx.compress_plane_n): planes of at
# least this many samples ENTERING STEP 4 (H * W after both paddings, like the two constants above) take it; None: the road
# is off and compress_band walks steps 0-3 in NumPy and uploads the float64 plane as before.  A plane that a set
# DCTN_ENTROPY_MIN_SAMPLES admits keeps taking jpegx.compress_plane_n.  Measured (profiles/dctn_band.json):
# on a 3000 x 4000 band a call takes 0.3-1.6 ms (uint8) / 1.3-2.0 ms (int64) instead of 18-182 / 29-191 ms; on square bands
# the job loses 4-6 us at 1024 samples and wins at every measured size from 2304 on.  The smallest measured size with no
# configuration slower than the road of before at or above it is therefore 2304; the constant stands at the next measured
# size above the planes (3456 and 8960 samples) that tests/test_gpu_dct_sizes.py pins to jpegx.forward_fused_n.
DCTN_BAND_JOB_MIN_SAMPLES = 16384

# decompress_band / decompress_band_u8 for dct_size other than 8 as ONE device job from the bytes to the band's samples
# (jpegx.decompress_band_n: the launches of jpegx.decompress_plane_n with the clamp, then DCTPadding.invert,
# SubSampling.invert and Padding.invert as the scatter kernel of csrc/jpegx_band_n.hip, the int64 band widened natively):
# planes of at least this many samples LEAVING THE INVERSE (H * W with both paddings, like the three constants above) take
# it; None: the road is off and both entries finish in NumPy as before.  Measured (DESIGN.md 4.12,
# profiles/dctn_band_decode.json): on a 3000 x 4000 band decompress_band takes 8.01-8.07 ms instead of 50.35-50.41 ms (block_size 1) and
# 7.15 instead of 12.69 ms (README bs 5 N 24), decompress_band_u8 0.360 instead of 3.26 ms at bs 5 and the same 1.48 ms at block_size 1 (the same
# launches and copy).  On the ladder of square planes, 262 144 .. 4 194 304 samples at N 4, 16 and 24, no configuration and no entry
# was slower than the parent's road; planes of exactly 262 144 samples are pinned to jpegx.decompress_plane_n by
# tests/test_gpu_dctn_roads.py and tests/test_gpu_entropy_decode_n.py, so the constant stands at the smallest measured size
# above that with no miss at or above it.
DCTN_BAND_DECODE_JOB_MIN_SAMPLES = 331776

# Jpeg.compress for dct_size other than 8 as ONE device job from the picture's interleaved pixels to the finished container
# (jpegx.compress_image_packed_n: one upload, steps 0-3 of all three bands as one launch of csrc/jpegx_band_n.hip, the bands'
# forward and entropy stages on two streams, one allocation for the container): pictures whose planes hold at least this
# many samples ENTERING STEP 4 (H * W of one band, like the four constants above) take it; None: the road is off and
# Jpeg.compress splits the image and calls compress_band three times as before.  Independent of DCTN_BAND_JOB_MIN_SAMPLES.
# Measured (profiles/dctn_image.json): on a 3000 x 4000 x 3 picture Jpeg.compress takes 19.1 instead of
# 27.1 ms (README bs 5 N 24), 23.5 instead of 59.9 ms (bs 1 N 4) and 21.4 instead of 67.8 ms (bs 1 N 16); on the ladder of
# square pictures, 16 384 .. 1 048 576 samples per plane at N 4, 16 and 24, no configuration was slower than the parent's
# road (1.15-6.0x faster).  The smallest measured size with no miss at or above it is the smallest measured, 16 384, which is
# also the lowest this constant may take: the pictures of 36 x 48 and 80 x 112 planes that tests/test_gpu_dctn_roads.py and
# tests/test_gpu_dct_sizes.py pin to jpegx.forward_fused_n lie below it.
DCTN_IMAGE_JOB_MIN_SAMPLES = 16384

# Jpeg.decompress for dct_size other than 8 as ONE device job from the container's three streams to the interleaved pixels
# (jpegx.decompress_image_n: the bands' decoders and inverse kernels on two streams, then DCTPadding.invert,
# SubSampling.invert, Padding.invert and the np.dstack as one scatter of csrc/jpegx_band_n.hip and one copy down): planes of
# at least this many samples LEAVING THE INVERSE take it; None: the road is off and Jpeg.decompress calls decompress_band_u8
# three times and stacks on the host as before.  Independent of DCTN_BAND_DECODE_JOB_MIN_SAMPLES.
# Measured (profiles/dctn_image.json): on a 3000 x 4000 x 3 picture Jpeg.decompress takes 18.2 instead of
# 30.9 ms (README bs 5 N 24), 33.7 instead of 46.9 ms (bs 1 N 4) and 34.8 instead of 39.6 ms (bs 1 N 16).  On the ladder the
# job lost once, at 16 384 samples and N 16 (0.424 against 0.373 ms: three device decoders cost more there than the host
# parser), and was 1.2-6.2x faster at every configuration from 36 864 samples on: the smallest measured size with no miss
# at or above it.  Never to stand below 16 384 (the 36 x 48 planes that tests/test_gpu_band_decode_job_n.py pins to
# jpegx.decompress_band_n with that gate at 0).
DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES = 36864

_device_seen = False


def _device_usable():
    """True when libjpegx loads and sees a GPU; never raises (a machine without one keeps the host road)."""
    global _device_seen
    if not _device_seen:
        try:
            import jpegx
            _device_seen = jpegx.device_count() > 0
        except Exception:
            return False
    return _device_seen


def _dctn_config(config):
    n = config.dct_size
    return config.transform == "DCT" and isinstance(n, (int, np.integer)) and 2 <= n <= 32 and n != 8 and _device_usable()


def dctn_on_device(config, samples):
    """The dispatch rule for dct_size != 8: transform 'DCT', 2 <= dct_size <= 32, a plane of at least
    DCTN_MIN_SAMPLES samples and a usable device."""
    return samples >= max(DCTN_MIN_SAMPLES, 1) and _dctn_config(config)


def _dctn_mode(config):
    """(mode, param) for the dct_size-N kernels (stock 'none', 'discard', 'divide' quantisers), else None."""
    args = config.quantization.gpu_mode()
    return args if args is not None and args[0] != "qtable" else None


# ---------------------------------------------------------------------------------------------------------------------
# the questions every road asks, each answered in one place
# ---------------------------------------------------------------------------------------------------------------------
def _admits(gate, config, samples):
    """What a DCTN_<X>_MIN_SAMPLES constant means.  ``gate`` is its value as the road reads it from this module when it
    is called: the road is on, the plane holds at least that many samples, and dctn_on_device takes such a plane."""
    return gate is not None and samples >= gate and dctn_on_device(config, samples)


def _kept_for_plane_job(samples):
    """A set DCTN_ENTROPY_MIN_SAMPLES that admits this plane keeps it: the plane goes on taking jpegx.compress_plane_n
    behind the host steps, not the band job or the picture job."""
    return DCTN_ENTROPY_MIN_SAMPLES is not None and samples >= DCTN_ENTROPY_MIN_SAMPLES


def _job_sizes(config):
    """(block_size, dct_size) as the device jobs for dct_size N take them, or None: block_size is no integer in 1..255, or
    the configuration is not one for the dct_size-N kernels (_dctn_config)."""
    bs = config.block_size
    if not isinstance(bs, (int, np.integer)) or not 1 <= bs <= 255 or not _dctn_config(config):
        return None
    return int(bs), int(config.dct_size)


def _job_mode(config):
    """(mode, param) for a device job that fuses whole groups of steps at dct_size N, or None: the registry is not stock or
    the quantiser is none the kernels take."""
    return _dctn_mode(config) if _stock_registry() else None


def _blocked_shape(rows, cols, bs, n):
    """(H, W) of the plane of whole n x n blocks that a rows x cols band becomes (geometry.band_geometry's last pair, from
    the numbers: the band job sizes from the band it is handed, the decoding jobs from the configuration)."""
    return tuple(-(-(-(-v // bs)) // n) * n for v in (rows, cols))


def _compress_job_n(config, rows, cols, gate):
    """(block_size, dct_size, mode, param) for a job that compresses 8-bit samples of rows x cols per band at dct_size N, or
    None.  The cheap questions come first, since most calls end at the gate: the road is off, _job_sizes says no, the
    plane of whole blocks holds more than 2^31 - 1 samples, ``gate`` does not admit it or a set DCTN_ENTROPY_MIN_SAMPLES
    keeps it; then _job_mode says no, or a coefficient could reach 2^31 - 1 -- _device_job_n's guard with the 8-bit bound
    255 in place of a scan."""
    sizes = None if gate is None else _job_sizes(config)
    if sizes is None:
        return None
    bs, n = sizes
    h, w = _blocked_shape(rows, cols, bs, n)
    if h * w > 2 ** 31 - 1 or not _admits(gate, config, h * w) or _kept_for_plane_job(h * w):
        return None
    args = _job_mode(config)
    if args is None or not _reach(255.0, n, *args) <= 2.0 ** 31 - 1.0:
        return None
    return (bs, n) + tuple(args)


def _decompress_job_n(config, blobs, gate):
    """(rows, cols, block_size, dct_size, mode, param) for a job that decodes ``blobs`` to bands of the configured size at
    dct_size N, or None.  Cheap questions first: the road is off, _job_sizes says no, height or width is no integer of at
    least 1 or they hold more than 2^31 - 1 samples, ``gate`` does not admit the plane of whole blocks; then _job_mode says
    no, the divisor is no integer (the jobs restore without the reference's truncation, _whole_divisor), or a blob is not
    coded bytes."""
    sizes = None if gate is None else _job_sizes(config)
    rows, cols = config.height, config.width
    if sizes is None or not isinstance(rows, (int, np.integer)) or not isinstance(cols, (int, np.integer)) \
            or rows < 1 or cols < 1 or rows * cols > 2 ** 31 - 1:
        return None
    bs, n = sizes
    h, w = _blocked_shape(rows, cols, bs, n)
    if not _admits(gate, config, h * w):
        return None
    args = _job_mode(config)
    if args is None or not _whole_divisor(args) or not all(_is_coded(b) for b in blobs):
        return None
    return (int(rows), int(cols), bs, n) + tuple(args)


def _blocks(config):
    """(hb, wb): the blocks of the configured band's plane, as RunLengthEncoding.invert counts them."""
    rle = run_length_encoding.RunLengthEncoding(config)
    return rle._height_in_blocks(), rle._width_in_blocks()


def _reach(peak, n, mode, param):
    """The largest magnitude a quantised coefficient of an n x n block can take when no sample exceeds ``peak``.  The roads
    differ in the peak (a scan of the plane, or the 8-bit bound 255) and in the bound they hold it against, which stay
    with them."""
    return peak * n * n / (min(abs(param), 1.0) if mode == "divide" else 1.0)


def _is_coded(blob):
    """Coded bytes as the device decoders take them: bytes or bytearray, not empty."""
    return isinstance(blob, (bytes, bytearray)) and len(blob) > 0


def _inverse_8_refuses(mode, param):
    """The fused 8x8 inverse kernels restore in fp32 from int16: a divisor that takes 32767 past 2^24 is not exact there."""
    return mode == "divide" and abs(param) * 32767 >= 2 ** 24


def _none_on_bad_rle(entry, *args, **kwargs):
    """entry(*args, **kwargs); None where the job met an amplitude beyond 15 bits -- the caller's road of before then ends
    in the host step raising the reference's BadRleCodeError with its own text.  Any other failure is the caller's."""
    import jpegx
    try:
        return entry(*args, **kwargs)
    except jpegx.JpegxError as exc:
        if "BadRleCodeError" not in str(exc):
            raise
        return None


def _none_on_refusal(entry, *args, **kwargs):
    """entry(*args, **kwargs); None for whatever libjpegx refuses or fails at.  For the decoding roads: the road of before
    then ends in the host parser and the host steps, which name the fault with the reference's exceptions."""
    import jpegx
    try:
        return entry(*args, **kwargs)
    except jpegx.JpegxError:
        return None


def _walk(classes, method, a, config, at=None, hot=None):
    """``method`` ('execute' or 'invert') of every class in turn; with ``at``, the three hot steps that stand there are
    one call of ``hot`` in their place."""
    for k, cls in enumerate(classes):
        if at is not None and at < k <= at + 2:
            continue                                    # folded into the fused launch at `at`
        a = hot(a, config) if k == at else getattr(cls(config), method)(a)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# dct_size other than 8
# ---------------------------------------------------------------------------------------------------------------------
def _forward_plane_n(pre, config):
    """(float64 plane, reach, mode, param) for the forward kernels of dct_size N, or None when this plane stays on the host:
    too small, not real, not whole blocks, or a quantiser the kernels do not take."""
    n = config.dct_size
    pre = np.asarray(pre)
    args = _dctn_mode(config)
    if args is None or pre.ndim != 2 or pre.dtype.kind not in "fiu" or not dctn_on_device(config, pre.size) \
            or pre.shape[0] % n or pre.shape[1] % n:
        return None
    pre = pre.astype(np.float64, copy=False)
    return (pre, _reach(max(abs(float(pre.max())), abs(float(pre.min()))), n, *args)) + tuple(args)


def _hot_forward_n(pre, config):
    """Steps 4+5+6 for dct_size N in one launch: int32 (H/N, W/N, N*N), or None when this plane stays on the host
    (too small, not real, not whole blocks, or coefficients that could leave the int32 range)."""
    todo = _forward_plane_n(pre, config)
    if todo is None:
        return None
    pre, reach, mode, param = todo
    if not reach < 2.0 ** 31:                       # also catches NaN
        return None
    import jpegx
    zz = jpegx.forward_fused_n(pre, config.dct_size, mode, param)
    # a coefficient in [2^31 - 0.5, 2^31) rounds to 2^31, which the kernel saturates to 2^31 - 1: not the reference's
    # integer, so such a plane stays on the host as well (-2^31 itself is an int32)
    if reach > 2.0 ** 31 - 1.0 and zz.max() == 2 ** 31 - 1:
        return None
    return zz


def _whole_divisor(args):
    """False for 'divide' with a divisor that is no integer.  Quantization.invert stores a * divisor into an array of the
    dtype it was handed, and step 7 hands back integers: the reference then truncates every restored coefficient toward
    zero (2773.5 -> 2773, -7.5 -> -7), which the device kernels, multiplying in float64, do not."""
    return args[0] != "divide" or args[1] == np.trunc(args[1])


def _restored_stream_n(zz, args):
    """(stream, mode, param) for jpegx.inverse_fused_n on an INTEGER stream as the reference restores it: as they are with a
    whole divisor; else the coefficients restored here, truncated like the reference's integer array does it, and handed
    over under 'none'.  None when such a coefficient leaves the int32 range."""
    if _whole_divisor(args) or zz.dtype.kind not in "iu":
        return (zz,) + tuple(args)
    restored = np.trunc(zz.astype(np.float64) * args[1])
    if restored.size and not np.abs(restored).max() < 2.0 ** 31:
        return None
    return restored.astype(np.int32), "none", 0.0


def _hot_inverse_n(zz, config, out="i32"):
    """Steps 6+5+4 inverted for dct_size N in one launch (int samples; for out 'u8' the uint8 samples with the clamp of
    Normalization.invert fused), or None when the stream stays on the host."""
    n = config.dct_size
    zz = np.asarray(zz)
    args = _dctn_mode(config)
    if args is None or zz.ndim != 3 or zz.shape[2] != n * n or zz.dtype.kind not in "fiu" \
            or not dctn_on_device(config, zz.size):
        return None
    todo = _restored_stream_n(zz, args)
    if todo is None:
        return None
    zz, mode, param = todo
    if zz.dtype != np.int32:
        if np.abs(zz).max() >= 2 ** 31 or not np.array_equal(zz, np.rint(zz)):
            return None
        zz = zz.astype(np.int32)
    import jpegx
    plane = jpegx.inverse_fused_n(zz, n, mode, param, out=out)
    return plane.astype(int) if out == "i32" else plane


def _device_job_n(pre, config):
    """Steps 4-8 for dct_size N as one pooled device job (jpegx.compress_plane_n: forward kernel + the run-time block length
    entropy stage, the coefficient stream never leaves the device), or None: the job road is switched off
    (DCTN_ENTROPY_MIN_SAMPLES), _hot_forward_n's preconditions do not hold, a coefficient could reach 2^31 - 1 (where the
    kernel's saturation would go unseen), or the job met an amplitude beyond 15 bits."""
    if not _admits(DCTN_ENTROPY_MIN_SAMPLES, config, np.asarray(pre).size):
        return None
    todo = _forward_plane_n(pre, config)
    if todo is None:
        return None
    pre, reach, mode, param = todo
    if not reach <= 2.0 ** 31 - 1.0:                # also catches NaN
        return None
    import jpegx
    return _none_on_bad_rle(jpegx.compress_plane_n, pre, config.dct_size, mode, param)


def _band_job_n(band, config):
    """All nine steps for dct_size N as one device job from the band's 8-bit samples (jpegx.compress_band_n), or None: the
    band is not what the job takes (a real 2-D non-empty band of an integer dtype; the job itself refuses samples outside
    0..255), _compress_job_n says no for DCTN_BAND_JOB_MIN_SAMPLES, or the job met an amplitude beyond 15 bits."""
    band = np.asarray(band)
    if band.ndim != 2 or band.size == 0 or band.dtype.kind not in "ui":
        return None
    job = _compress_job_n(config, band.shape[0], band.shape[1], DCTN_BAND_JOB_MIN_SAMPLES)     # sized from the band itself
    if job is None:
        return None
    import jpegx
    native = band if band.dtype in (np.uint8, np.int32, np.int64) else band.astype(np.int64)
    return _none_on_bad_rle(jpegx.compress_band_n, native, *job)


def _compress_band_n(a, config):
    """compress_band for dct_size != 8: where DCTN_BAND_JOB_MIN_SAMPLES admits the plane, all nine steps as one device job
    from the band's 8-bit samples (_band_job_n), before any host step runs.  Otherwise host steps 0-3 as they are, then the three hot steps as one device launch
    (jpegx_forward_fused_n) and -- in a stock registry -- libjpegx's sequential entropy coder on the host; or, where the
    job road is switched on (DCTN_ENTROPY_MIN_SAMPLES) and the registry is stock, steps 4-8 as one device job
    (_device_job_n).  None when the road does not apply; the caller then walks the steps on the host as before."""
    import jpegx
    todo = list(step_classes)
    at = _hot_run(todo)
    if at is None or _dctn_mode(config) is None:
        return None
    blob = _band_job_n(a, config)
    if blob is not None:
        return blob                                 # all nine steps in one device job
    a = _walk(todo[:at], "execute", a, config)
    if _stock_registry():
        blob = _device_job_n(a, config)
        if blob is not None:
            return blob                             # steps 4-8 in one device job
    zz = _hot_forward_n(a, config)
    if zz is None:
        return _walk(todo[at:], "execute", a, config)
    if _stock_registry():
        try:
            return jpegx.entropy_encode_n(zz, config.dct_size ** 2)
        except jpegx.JpegxError:
            pass                                    # an amplitude beyond 15 bits: the host step raises the reference's error
    # what Quantization + ZigzagOrder hand to the next step
    return _walk(todo[at + 3:], "execute", zz.astype(np.float64), config)


def _decode_stream_n(blob, config, blocks=None):
    """Steps 8+7 inverted by libjpegx's sequential parser: int32 (hb, wb, N*N), or None (a malformed stream: the host
    steps then name the fault as they always did).  Asks for no stock registry and no whole divisor itself.  ``blocks``:
    _blocks(config), where the caller has it already."""
    import jpegx
    hb, wb = blocks or _blocks(config)
    nn = config.dct_size ** 2
    if not _is_coded(blob) or hb * wb <= 0 or _dctn_mode(config) is None or not dctn_on_device(config, hb * wb * nn):
        return None
    zz = _none_on_refusal(jpegx.entropy_decode_n, blob, hb * wb, nn)
    return None if zz is None else zz.reshape(hb, wb, nn)


def _decode_job_n(blob, config, out, blocks=None):
    """Steps 8-4 inverted for dct_size N as one pooled device job (jpegx.decompress_plane_n): the samples of the plane of
    whole N x N blocks, uint8 (clamped) for out 'u8' or int32 for 'i32'; or None -- the job road is switched off
    (DCTN_ENTROPY_DECODE_MIN_SAMPLES), _decode_stream_n's preconditions do not hold, the registry is not stock, the divisor
    is no integer (the job restores without the reference's truncation, _whole_divisor), or the device refused the stream:
    the caller's road of before then ends in the host parser and the host steps naming the fault.  The plane has no
    block_size, so unlike the band jobs this one does not ask about it.  ``blocks``: _blocks(config), where the caller has
    it already."""
    import jpegx
    hb, wb = blocks or _blocks(config)
    n = config.dct_size
    if hb * wb <= 0 or not _admits(DCTN_ENTROPY_DECODE_MIN_SAMPLES, config, hb * wb * n * n):
        return None                                 # the cheap question first: most calls end at the gate
    args = _job_mode(config)
    if args is None or not _whole_divisor(args) or not _is_coded(blob):
        return None
    return _none_on_refusal(jpegx.decompress_plane_n, blob, hb * n, wb * n, n, *args, out=out)


def _band_decode_job_n(blob, config, out):
    """All nine steps inverted for dct_size N as one pooled device job (jpegx.decompress_band_n): the band at its configured
    size, uint8 for out 'u8' or int64 for 'i64'; or None -- _decompress_job_n says no for DCTN_BAND_DECODE_JOB_MIN_SAMPLES,
    or the device refused the stream: the caller's road of before then names the fault with the reference's exceptions."""
    job = _decompress_job_n(config, (blob,), DCTN_BAND_DECODE_JOB_MIN_SAMPLES)
    if job is None:
        return None
    import jpegx
    return _none_on_refusal(jpegx.decompress_band_n, blob, *job, out=out)


def _decode_n(blob, config, want):
    """The way back for dct_size N, for ``want`` 'u8' (displayable samples) or 'int' (the reference's integers), as
    (array, whether it is the finished band): the band decode job's band; else the plane of whole blocks by the plane
    decode job, else by libjpegx's host parser and jpegx.inverse_fused_n -- the caller's geometry steps remain; else
    (None, False) and the host steps run.  A JpegxError of the inverse kernel is the caller's to map."""
    band_out, plane_out = ("u8", "u8") if want == "u8" else ("i64", "i32")
    band = _band_decode_job_n(blob, config, band_out)
    if band is not None:
        return band, True                           # all nine steps inverted in one device job
    blocks = _blocks(config)                        # once for both roads below
    plane = _decode_job_n(blob, config, plane_out, blocks)
    if plane is not None:
        return (plane if want == "u8" else plane.astype(int)), False
    zz = _decode_stream_n(blob, config, blocks)
    return (None if zz is None else _hot_inverse_n(zz, config, plane_out)), False


# ---------------------------------------------------------------------------------------------------------------------
# dct_size 8
# ---------------------------------------------------------------------------------------------------------------------
def _mode_8(config):
    """(mode, param) of the accelerated configuration -- transform 'DCT', dct_size 8, a quantiser libjpegx holds -- else None."""
    return config.quantization.gpu_mode() if config.transform == "DCT" and config.dct_size == 8 else None


def _accelerated(config):
    return _mode_8(config) is not None


def _job_config_8(config):
    """(block_size, mode, param) where the 8x8 device jobs take the configuration, or None: not the accelerated
    configuration, a registry that is not stock, or a block_size beyond 1..255 (one that is no integer, such as 2.0, passes:
    the native entries take int(block_size))."""
    args = _mode_8(config)
    if args is None or not _stock_registry() or not 1 <= config.block_size <= 255:
        return None
    return (config.block_size,) + tuple(args)


def _decode_job_8(config):
    """(height, width, block_size, mode, param) of the plane for the 8x8 device decoding entries, or None: _job_config_8
    says no, or the divisor is one the fused inverse refuses."""
    job = _job_config_8(config)
    if job is None:
        return None
    bs, mode, param = job
    if _inverse_8_refuses(mode, param):
        return None
    hb, wb = _blocks(config)
    return hb * 8, wb * 8, bs, mode, param


def _hot_forward(pre, config):
    """Steps 4+5+6 on the plane that leaves step 3: one fused launch when the samples are exact in
    fp32 (always the case for 8-bit data with block_size 1, 2, 4, ...), else the exact float64 kernels."""
    import jpegx
    mode, param = config.quantization.gpu_mode()
    pre = np.asarray(pre)
    as32 = pre.astype(np.float32)
    if np.array_equal(as32.astype(np.float64), pre.astype(np.float64)):
        return jpegx.forward_fused(as32, mode, param).astype(np.float64)
    pre = pre.astype(np.float64)
    if pre.shape[1] % 2 == 0:
        zz = jpegx.forward_fused_f64(pre, mode, param)          # one all-float64 launch
        if zz.min() > -32768 and zz.max() < 32767:              # int16 saturation would hide larger values (np.abs wraps at -32768)
            return zz.astype(np.float64)
    coeffs = jpegx.quantize_f64(jpegx.dct8x8_f64(pre), mode, param)
    return jpegx.zigzag(coeffs)


def _hot_inverse(zz, config):
    """Steps 6+5+4 inverted: fused launch for int16-range coefficients, float64 kernels otherwise."""
    import jpegx
    mode, param = config.quantization.gpu_mode()
    zz = np.asarray(zz)
    if zz.size and np.abs(zz).max() <= 32767 and np.array_equal(zz, np.rint(zz)) and not _inverse_8_refuses(mode, param):
        return jpegx.inverse_fused(zz.astype(np.int16), mode, param, out="f32").astype(int)
    plane = jpegx.restore_f64(jpegx.unzigzag(zz.astype(np.float64)), mode, param)
    return jpegx.idct8x8_f64(plane, do_round=True).astype(int)


_HOT_STEPS = (basis_change.BasisChange, quantization.Quantization, zigzag_order.ZigzagOrder)
_BUILTIN_STEPS = (padding.Padding, subsampling.SubSampling, dct_padding.DCTPadding, normalization.Normalization,
                  basis_change.BasisChange, quantization.Quantization, zigzag_order.ZigzagOrder,
                  run_length_encoding.RunLengthEncoding, rle_byte_stream.RleBytestream)


def _stock_registry():
    """True while nobody has registered extra steps: only then may whole groups of steps be fused."""
    return len(step_classes) == len(_BUILTIN_STEPS) and all(map(operator.is_, step_classes, _BUILTIN_STEPS))


def _hot_run(classes):
    """Index at which the three built-in hot steps stand directly one after another in ``classes`` (only
    then may steps 4+5+6 be one launch: a user step registered between them, or a subclass standing in for
    one of them, must run at its own place in the order, like in the reference), else None."""
    for i in range(len(classes) - 2):
        if all(a is b for a, b in zip(classes[i:i + 3], _HOT_STEPS)):
            return i
    return None


def _bad_rle(exc):
    """libjpegx reports the reference's BadRleCodeError condition (amplitude beyond 15 bits, illegal code in a
    stream) in its error text; callers of the pipeline API get the reference's exception type."""
    import util
    if "BadRleCodeError" in str(exc):
        return util.BadRleCodeError(str(exc))
    if "ValueError" in str(exc):                    # what the reference raises for these streams (int('', 2) / reshape)
        return ValueError(str(exc))
    return exc


def _front_end_fused(band, config, with_entropy):
    """Steps 0-6 (or 0-8 when with_entropy) on the GPU.  With the entropy stage an integer band of any shape is ONE
    native call: range check, upload into a device plane of the padded shape, Padding and DCTPadding as a margin fill
    there, SubSampling + BasisChange + Quantization + ZigzagOrder in the forward kernels, RunLengthEncoding +
    RleBytestream (jpegx_entropy_*) with the coefficients never leaving the device.  What that call refuses (a band
    outside 0..255, a divisor below 0.5 at block sizes 1, 2, 4) and the road without the entropy stage pad -- and, where
    DCT padding is needed, pool -- on the host first.  Returns None when not applicable."""
    bs = config.block_size
    band = np.asarray(band)
    if not 1 <= bs <= 255 or band.ndim != 2 or band.size == 0 or band.dtype.kind not in "ui":
        return None
    import jpegx
    mode, param = config.quantization.gpu_mode()
    if with_entropy:
        # one native call whatever the band's shape: range check, upload, steps 0..8, bytes back
        native = band if band.dtype in (np.uint8, np.int32, np.int64) else band.astype(np.int64)
        blob = jpegx.compress_plane_native(np.ascontiguousarray(native), bs, mode, param, ragged=True)
        if blob is not None:
            return blob
    padded = band if bs == 1 else padding.Padding(config).execute(band)
    if bs not in (1, 2, 4) or (band.dtype != np.uint8 and (band.min() < 0 or band.max() > 255)):
        return None
    if padded.shape[0] % (8 * bs) or padded.shape[1] % (8 * bs):
        # DCT padding is needed: it replicates POOLED edge samples (dct_padding.py:8-9), so pool on
        # the host first (steps 1-3), then the device does steps 4-8 on the padded plane
        pre = _walk((subsampling.SubSampling, dct_padding.DCTPadding, normalization.Normalization), "execute", padded, config)
        if not np.array_equal(pre.astype(np.float32).astype(np.float64), pre):
            return None
        plane = pre.astype(np.uint8) if np.array_equal(pre, np.rint(pre)) else pre.astype(np.float32)
        if with_entropy:
            return jpegx.compress_plane(plane, 1, mode, param)
        return jpegx.forward_fused(plane.astype(np.float32), mode, param, pixel_input=True).astype(np.float64)
    if with_entropy:
        return jpegx.compress_plane(padded, bs, mode, param)      # uint8 upload when the shape allows
    return jpegx.forward_fused_pooled(padded.astype(np.float32), bs, mode, param, pixel_input=True).astype(np.float64)


def _back_end_fused(zz, config):
    """Steps 6-0 inverted in one launch: un-zigzag, dequantise, IDCT, round, clamp to [0, 255]
    (Normalization.invert), replicate block_size x block_size (SubSampling.invert) on the GPU,
    then the two crops (DCTPadding.invert, Padding.invert) as one slice."""
    bs = config.block_size
    zz = np.asarray(zz)
    mode, param = config.quantization.gpu_mode()
    if not 1 <= bs <= 255 or zz.ndim != 3 or zz.shape[2] != 64 or zz.size == 0 or _inverse_8_refuses(mode, param):
        return None
    if zz.dtype != np.int16:                  # the C++ entropy decoder hands over int16; anything else is checked
        if np.abs(zz).max() > 32767 or not np.array_equal(zz, np.rint(zz)):
            return None
        zz = zz.astype(np.int16)
    import jpegx
    full = jpegx.inverse_fused_u8(zz, mode, param, inflate=bs)
    return full[:config.height, :config.width].astype(int)


# ---------------------------------------------------------------------------------------------------------------------
# the public entries
# ---------------------------------------------------------------------------------------------------------------------
def compress_band(a, config):
    """Run every registered step forward (pipeline/__init__.py:71-76)."""
    import jpegx
    fused = _accelerated(config)
    todo = list(step_classes)
    try:
        if not fused and _dctn_config(config):
            out = _compress_band_n(a, config)
            if out is not None:
                return out
        if fused and _stock_registry():
            blob = _front_end_fused(a, config, with_entropy=True)
            if blob is not None:
                return blob                               # all nine steps on the device
        return _walk(todo, "execute", a, config, _hot_run(todo) if fused else None, _hot_forward)
    except jpegx.JpegxError as exc:
        raise _bad_rle(exc)


def decompress_band_u8(compression_result, config):
    """decompress_band for callers that want the displayable uint8 samples (what Jpeg.decompress turns the
    band into anyway, pipeline/__init__.py:119-122): skips the int64 array the reference's API returns --
    for a 4096x4096 band that conversion alone costs more than the whole device pipeline."""
    import jpegx
    a = compression_result
    job = _decode_job_8(config) if _is_coded(a) else None
    band = None if job is None else _none_on_refusal(jpegx.decompress_plane, a, *job)
    if band is not None:
        return band[:config.height, :config.width]
    if not _accelerated(config) and _stock_registry():
        try:
            plane, done = _decode_n(a, config, "u8")
        except jpegx.JpegxError as exc:
            raise _bad_rle(exc)
        if done:
            return plane
        if plane is not None:
            # the clamp was fused into the inverse; the geometry steps on uint8: crop the DCT padding, replicate, crop
            bs = config.block_size
            (rows, cols), _, pooled, _ = geometry.band_geometry(config)
            plane = plane[:pooled[0], :pooled[1]]
            if bs != 1:
                plane = np.repeat(np.repeat(plane, bs, axis=0), bs, axis=1)
            return np.ascontiguousarray(plane[:rows, :cols])
    return decompress_band(compression_result, config).astype(np.uint8)


def decompress_band(compression_result, config):
    """Run every registered step backwards (pipeline/__init__.py:79-88)."""
    import jpegx
    a = compression_result
    # dct_size 8: all nine steps inverted on the device, entropy decoding included; only the samples come back
    job = _decode_job_8(config) if _is_coded(a) else None
    band = None if job is None else _none_on_refusal(jpegx.decompress_plane_i64, a, *job, config.height, config.width)
    if band is not None:
        return band if band.dtype == np.dtype(int) else band.astype(int)
    fused = _accelerated(config)
    todo = list(reversed(step_classes))
    try:
        if fused and _stock_registry():
            if isinstance(a, (bytes, bytearray)):
                # not a well-formed stream, or one the device job does not take: the host parser of libjpegx says exactly
                # what is wrong (steps 8, 7)
                hb, wb = _blocks(config)
                a = jpegx.entropy_decode(a, hb * wb).reshape(hb, wb, 64)
            else:
                a = _walk(todo[:2], "invert", a, config)
            band = _back_end_fused(a, config)
            if band is not None:
                return band
            todo = todo[2:]
        if not fused and _stock_registry():
            band, done = _decode_n(a, config, "int")
            if done:                                # all nine steps inverted in one device job: this is the band
                return band if band.dtype == np.dtype(int) else band.astype(int)
            if band is not None:
                return _walk(todo[5:], "invert", band, config)      # Normalization, DCTPadding, SubSampling, Padding
        at = _hot_run(list(reversed(todo))) if fused else None      # position counted in forward order
        at = None if at is None else len(todo) - 3 - at             # -> index of ZigzagOrder in the reversed list
        return _walk(todo, "invert", a, config, at, _hot_inverse)
    except jpegx.JpegxError as exc:
        raise _bad_rle(exc)


class CompressedData:
    def __init__(self, y, cb, cr):
        self.y = y
        self.cb = cb
        self.cr = cr


class Jpeg:
    """PIL image <-> container bytes (pipeline/__init__.py:98-124)."""

    def __init__(self, config):
        self.config = config

    def compress(self, image):
        nbands = len(image.getbands())
        if nbands != 3:                                      # the reference's `y, cb, cr = image.split()`
            raise ValueError("%s to unpack (expected 3, got %d)" % ("too many values" if nbands > 3 else "not enough values", nbands))
        whole = _compress_pixels(image, self.config)         # the picture's pixels as ONE array, the bands made on the device
        if whole is not None:
            return whole
        whole = _compress_pixels_n(image, self.config)       # the same for dct_size other than 8
        if whole is not None:
            return whole
        arrays = [band_to_array(band) for band in image.split()]
        whole = _compress_image(arrays, self.config)        # the finished container, written band by band from the device
        if whole is not None:
            return whole
        bands = [compress_band(a, self.config) for a in arrays]
        return file_format.generate_data(self.config, CompressedData(*bands))

    def compress_rgb(self, image):
        """The bytes of ``self.compress(image.convert("YCbCr"))`` -- what the command line does with an opened picture
        (compress.py:9, 19-20).  An 8-bit mode-'RGB' picture of the configured size that a picture job admits goes up as
        it is and becomes Pillow's YCbCr on the device, inside the job (jpegx.compress_image_packed / _packed_n with
        colour='rgb'); every other case is literally that line."""
        if getattr(image, "mode", None) == "RGB":
            whole = _compress_pixels(image, self.config, colour="rgb")
            if whole is None:
                whole = _compress_pixels_n(image, self.config, colour="rgb")
            if whole is not None:
                return whole
        return self.compress(image.convert("YCbCr"))

    @staticmethod
    def decompress_rgb(bytestream):
        """A mode-'RGB' image equal to ``Jpeg.decompress(bytestream).convert("RGB")`` -- the command line's way back
        (decompress.py:9-10).  Where a picture job decodes the container, Pillow's conversion runs on the device inside
        it (jpegx.decompress_image_native / decompress_image_n with colour='rgb'); otherwise, and for a stream the device
        refuses, literally that line."""
        from PIL import Image
        config, data = file_format.read_data(bytestream)
        blobs = (data.y, data.cb, data.cr)
        packed = _decompress_image(blobs, config, colour="rgb")
        if packed is None:
            packed = _decompress_image_n(blobs, config, colour="rgb")
        if packed is None:
            return Jpeg.decompress(bytestream).convert("RGB")
        return Image.fromarray(packed, mode="RGB")

    @staticmethod
    def decompress(bytestream):
        from PIL import Image
        config, data = file_format.read_data(bytestream)
        size = (config.height, config.width)
        packed = _decompress_image((data.y, data.cb, data.cr), config)
        if packed is None:
            packed = _decompress_image_n((data.y, data.cb, data.cr), config)      # dct_size other than 8: one device job
        if packed is None:
            packed = np.dstack([decompress_band_u8(b, config).reshape(size) for b in (data.y, data.cb, data.cr)])
        return Image.fromarray(packed, mode="YCbCr")


def _picture_size(image, config):
    """(rows, cols) of a picture that the picture jobs take whole -- three bands (CompressedData holds three), mode YCbCr,
    RGB, LAB or HSV, of the configured size -- else None."""
    try:
        bands = image.getbands()
    except Exception:
        return None
    if len(bands) != 3 or image.mode not in ("YCbCr", "RGB", "LAB", "HSV") \
            or (config.height, config.width) != (image.height, image.width):
        return None
    return image.height, image.width


def _colour_kw(colour):
    """The picture jobs' ``colour`` keyword where a road sets it; the roads of before call their entries as they always did."""
    return {} if colour is None else {"colour": colour}


def _picture_pixels(image):
    """The interleaved uint8 pixels (rows, cols, 3) of a picture _picture_size took, C-contiguous, else None.  The costly
    part of the vetting (14 ms for 4096 x 4096), so the roads ask for it last."""
    pixels = np.asarray(image)
    return np.ascontiguousarray(pixels) if pixels.dtype == np.uint8 and pixels.ndim == 3 else None


def _compress_pixels(image, config, colour=None):
    """Jpeg.compress without `image.split()`: for a 4096 x 4096 picture PIL needs 25 ms to split the bands and hand each
    over as an array, 14 ms to hand over the interleaved pixels in one piece (np.asarray(image)) -- and the native job
    behind either takes 1.5 ms.  Multi-band 8-bit pictures of any size take this road (the device pads: Padding and
    DCTPadding are a margin fill in the padded device planes); the bytes are those of the per-band road.  None otherwise.
    ``colour``: handed to the job (Jpeg.compress_rgb: 'rgb', the picture becomes Pillow's YCbCr on the device)."""
    import jpegx
    job = _job_config_8(config)
    if job is None or _picture_size(image, config) is None:
        return None
    pixels = _picture_pixels(image)
    if pixels is None:
        return None
    try:
        return jpegx.compress_image_packed(pixels, *job, prefix=file_format.create_header(config), ragged=True, **_colour_kw(colour))
    except jpegx.JpegxError as exc:
        raise _bad_rle(exc)


def _compress_image(arrays, config):
    """The three bands of one picture through ONE native job (jpegx_host_compress_image) that writes the finished
    container: the bytes of file_format.generate_data over three compress_band calls (pipeline/__init__.py:102-110,
    file_format.py:86-93), with the bands alternating between two streams and no concatenation on the host; bands of
    any size, padded on the device.  None when the configuration or the bands do not take that road."""
    import jpegx
    job = _job_config_8(config)
    if job is None or any(a.ndim != 2 or a.size == 0 or a.dtype.kind not in "ui" for a in arrays):
        return None
    try:
        return jpegx.compress_image_native([np.ascontiguousarray(a) for a in arrays], *job,
                                           prefix=file_format.create_header(config), ragged=True)
    except jpegx.JpegxError as exc:
        raise _bad_rle(exc)


def _decompress_image(blobs, config, colour=None):
    """Jpeg.decompress's three decompress_band calls + np.dstack (pipeline/__init__.py:112-124) as ONE native job;
    (height, width, 3) uint8, or None when this road does not apply or the device decoder refuses a stream (the
    per-band road then names the fault).  ``colour``: handed to the job (Jpeg.decompress_rgb: 'rgb', Pillow's RGB pixels)."""
    import jpegx
    job = _decode_job_8(config)
    if job is None or not all(_is_coded(b) for b in blobs):
        return None
    return _none_on_refusal(jpegx.decompress_image_native, blobs, *job, config.height, config.width, **_colour_kw(colour))


def _compress_pixels_n(image, config, colour=None):
    """_compress_pixels for dct_size other than 8: the picture's interleaved pixels through ONE device job that writes the
    finished container (jpegx.compress_image_packed_n) -- no `image.split()`, one upload instead of three, one wait per band
    for its size instead of a whole job -- with the bytes of file_format.generate_data over three compress_band calls.  None:
    the picture is not one the picture jobs take (_picture_size, _picture_pixels) or is empty or holds more than 2^31 - 1
    pixels per band; _compress_job_n says no for DCTN_IMAGE_JOB_MIN_SAMPLES; or the job met an amplitude beyond 15 bits --
    the per-band road then raises the reference's BadRleCodeError with its own text.  Unlike _compress_pixels this road
    refuses a block_size that is no integer.  ``colour``: handed to the job, as in _compress_pixels."""
    size = _picture_size(image, config)
    if size is None or size[0] < 1 or size[1] < 1 or size[0] * size[1] > 2 ** 31 - 1:
        return None
    job = _compress_job_n(config, size[0], size[1], DCTN_IMAGE_JOB_MIN_SAMPLES)
    pixels = None if job is None else _picture_pixels(image)
    if pixels is None:
        return None
    import jpegx
    return _none_on_bad_rle(jpegx.compress_image_packed_n, pixels, *job, prefix=file_format.create_header(config), **_colour_kw(colour))


def _decompress_image_n(blobs, config, colour=None):
    """_decompress_image for dct_size other than 8: three decompress_band_u8 calls and the np.dstack as ONE device job
    (jpegx.decompress_image_n); (height, width, 3) uint8.  None: _decompress_job_n says no for
    DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES, or the device refused a band's stream: the per-band road then names the fault.
    ``colour``: handed to the job, as in _decompress_image."""
    job = _decompress_job_n(config, blobs, DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES)
    if job is None:
        return None
    import jpegx
    return _none_on_refusal(jpegx.decompress_image_n, blobs, *job, **_colour_kw(colour))


# ---------------------------------------------------------------------------------------------------------------------
# many bands of one shape at once
# ---------------------------------------------------------------------------------------------------------------------
# compress_bands / decompress_bands_u8 take the batch road (jpegx.batch_compress_n / batch_decompress_n for dct_size other
# than 8, jpegx.batch_compress / batch_decompress for dct_size 8: one upload, one launch chain and one download for the whole
# stack) from this many bands on; None: the road is off and both functions are a loop over the per-band functions.  Never
# below 2: one band is what the per-band functions are for.  All three constants are read when the functions are called.
# Measured (profiles/batch_codec_n.json; bands of 64 x 64 at N 4 and N 16, the batch road against the loop,
# alternating call by call on one MI355X): with 2 bands the batch loses three of four comparisons (compressing 0.21-0.22 ms
# against 0.17-0.18 ms: its two status reads and three allocations against two pooled jobs), with 4 it wins all four
# (0.22-0.23 against 0.37-0.38 ms compressing, 0.15-0.26 against 0.45-0.46 ms decompressing), and so at 8 and 16 (2.1-8.3x),
# 64 (10-19x) and 4096 bands (47-55x).  The smallest measured count with no loss at or above it.
DCTN_BATCH_MIN_PLANES = 4

# ... and only for planes of at most this many samples ENTERING STEP 4 / LEAVING THE INVERSE (H * W of one band after both
# paddings, like the DCTN_*_MIN_SAMPLES constants); None: no upper limit.  The batch pays its launches and copies once, which
# is what many SMALL bands gain from; it also stacks the bands on the host and moves the stack through pageable memory in one
# piece, while the per-band jobs stream through the pool's pinned staging, and that is what large bands lose by.  Measured
# (the same record and profiles/batch_codec_n_run1.json, two runs): compressing, the batch is 13-55x faster than the loop on
# 4096 planes of 4096 samples and 256 of 14 400, and 1.4-1.9x SLOWER on 256 planes of 262 144 samples in both runs; on 16 planes
# of 489 600 and 12 M samples it was 2.5-5.1x slower in one run and faster in the other, in which the loop itself took 4-22x
# longer (a shared host).  Decompressing, it is 1.3-51x faster up to 262 144 samples in both runs and lost at one
# configuration each at 489 600 and 12 M samples in the first.  Each constant is the largest measured plane with no loss at
# or below it in either run.
DCTN_BATCH_COMPRESS_MAX_SAMPLES = 14400
DCTN_BATCH_DECOMPRESS_MAX_SAMPLES = 262144


def _batch_gate(count, samples, most):
    """What the three constants above mean, for ``count`` bands whose planes hold ``samples`` samples each; ``most`` is
    the direction's DCTN_BATCH_*_MAX_SAMPLES as the caller reads it from this module."""
    gate = DCTN_BATCH_MIN_PLANES
    return gate is not None and count >= max(gate, 2) and (most is None or samples <= most)


def _stacked_u8(bands):
    """The bands as one uint8 array [n][rows][cols], or None: they are not all real 2-D non-empty integer bands of one
    shape with samples in 0..255."""
    arrays = [b if isinstance(b, np.ndarray) else np.asarray(b) for b in bands]
    shape = arrays[0].shape
    if len(shape) != 2 or 0 in shape or any(a.shape != shape or a.dtype.kind not in "ui" for a in arrays):
        return None
    if any(a.dtype != np.uint8 and (a.min() < 0 or a.max() > 255) for a in arrays):
        return None
    return np.stack([a.astype(np.uint8, copy=False) for a in arrays])


def _compress_batch(bands, config):
    """The byte strings of the batch road, or None: the gate, the bands or the configuration do not admit it, or libjpegx
    refused or failed -- the per-band loop then names the band and the fault."""
    most = DCTN_BATCH_COMPRESS_MAX_SAMPLES
    if not _batch_gate(len(bands), 0, most) or not _stock_registry() or not _device_usable():
        return None
    shape = np.shape(bands[0])
    if len(shape) != 2 or 0 in shape:
        return None
    rows, cols = shape
    eight = _accelerated(config)
    job = _job_config_8(config) if eight else _compress_job_n(config, rows, cols, 0)
    if job is None:
        return None
    if eight and (job[0] not in (1, 2, 4) or rows % (8 * job[0]) or cols % (8 * job[0])):
        return None                                     # the shape and block_size limits of jpegx.batch_compress
    h, w = (rows // int(job[0]), cols // int(job[0])) if eight else _blocked_shape(rows, cols, job[0], job[1])
    if not _batch_gate(len(bands), h * w, most) or h * w * len(bands) > 2 ** 31 - 1:
        return None
    stack = _stacked_u8(bands)                          # the costly part of the vetting: last
    if stack is None:
        return None
    import jpegx
    return _none_on_refusal(jpegx.batch_compress if eight else jpegx.batch_compress_n, stack, *job)


def compress_bands(bands, config):
    """[compress_band(b, config) for b in bands], byte for byte.  At least DCTN_BATCH_MIN_PLANES 8-bit bands of one shape
    whose planes hold at most DCTN_BATCH_COMPRESS_MAX_SAMPLES samples, under a configuration the device jobs admit (_job_sizes / _job_mode; dct_size 8: _job_config_8 within the shape and
    block_size limits of jpegx.batch_compress) go to the device as ONE batch; everything else, and every refusal of the
    batch -- a BadRleCodeError included, so that the failing band is named as before -- is that loop."""
    bands = list(bands)
    blobs = _compress_batch(bands, config) if bands else None
    return blobs if blobs is not None else [compress_band(b, config) for b in bands]


def _decompress_batch(blobs, config):
    """uint8 [n][height][width] by the batch road, or None (see _compress_batch)."""
    most = DCTN_BATCH_DECOMPRESS_MAX_SAMPLES
    if not _batch_gate(len(blobs), 0, most) or not _stock_registry() or not _device_usable() or not all(_is_coded(b) for b in blobs):
        return None
    import jpegx
    if _accelerated(config):
        job = _decode_job_8(config)
        if job is None or not _batch_gate(len(blobs), job[0] * job[1], most):
            return None
        planes = _none_on_refusal(jpegx.batch_decompress, blobs, *job, out="u8")
        return None if planes is None else planes[:, :config.height, :config.width]
    job = _decompress_job_n(config, blobs, 0)
    if job is None:
        return None
    h, w = _blocked_shape(*job[:4])
    if not _batch_gate(len(blobs), h * w, most) or h * w * len(blobs) > 2 ** 31 - 1:
        return None
    return _none_on_refusal(jpegx.batch_decompress_n, blobs, *job)


def decompress_bands_u8(compression_results, config):
    """[decompress_band_u8(r, config) for r in compression_results], sample for sample: the batch road under the conditions
    of compress_bands (coded bytes in place of 8-bit bands; DCTN_BATCH_DECOMPRESS_MAX_SAMPLES; a whole divisor, as the decoding
    jobs ask), else that loop."""
    results = list(compression_results)
    stack = _decompress_batch(results, config) if results else None
    return list(stack) if stack is not None else [decompress_band_u8(r, config) for r in results]


# ---------------------------------------------------------------------------------------------------------------------
# many pictures of one size at once
# ---------------------------------------------------------------------------------------------------------------------
# compress_pictures / decompress_pictures_u8 take the batch road (jpegx.batch_compress_pictures_n /
# batch_decompress_pictures_n, dct_size other than 8; dct_size 8 has its own entries and gates, DCT8_PICTURE_BATCH_* below:
# one upload, one launch chain and one download for the whole stack, the
# colour conversion, the split into bands and the np.dstack inside the device's gather and scatter) from this many pictures
# on; None: the road is off and the functions are a loop over Jpeg.compress / compress_rgb / decompress / decompress_rgb.
# Never below 2: one picture is what those are for.  All three constants are read when the functions are called.
# Measured (profiles/batch_pictures_n.json and, a second run of the same code, _run2.json; figures of the first,
# the second agrees on every verdict here; pictures of 64 x 64 and 128 x 128 at N 4 and N 16, with colour
# 'rgb' and without, the batch road against the loop, alternating call by call on one MI355X, 12 rounds): ONE picture through
# the batch loses compressing at 128 x 128 (0.22 against 0.17 ms in all four comparisons: the picture job of the loop is one
# pooled job, the batch two status reads and three allocations) and wins at 64 x 64 (0.23 against 0.30-0.36 ms); with 2 pictures
# it wins all sixteen comparisons (0.23-0.25 against 0.34-0.75 ms compressing, 0.18-0.27 against 0.40-0.77 ms decompressing), and
# so at 4, 8, 16 (1.4-13x) and 64 pictures (4.1-22x).  The smallest measured count with no loss at or above it.
DCTN_PICTURE_BATCH_MIN_PICTURES = 2

# ... and only for planes of at most this many samples ENTERING STEP 4 / LEAVING THE INVERSE (H * W of one band of one
# picture after both paddings, like DCTN_BATCH_*_MAX_SAMPLES); None: no upper limit.  As with the band batch, the batch pays
# its launches and copies once and stacks the pictures on the host (np.stack) and moves the stack through pageable memory in
# one piece, while the picture jobs of the loop stream through the pool's pinned staging.
# Measured (the same two records): compressing, the batch is 23-27x faster than the loop on 4096 pictures of 4096 samples a
# plane and 7.4-9.3x on 256 of 14 400 in both runs; on 256 pictures of 262 144 samples it was 1.03-1.27x faster in the first run and,
# with colour 'rgb', 1.08-1.11x SLOWER in the second (93-101 against 86-91 ms); on 16 pictures of 489 600 samples it is 1.1-1.3x
# slower in both (259-299 against 214-231 ms) and on 16 of 12 M 2.2-4.3x slower (251-495 against 108-132 ms).  Decompressing, it is
# 1.9-46x faster up to 489 600 samples in both runs; on 16 pictures of 12 M samples it lost one comparison of four in the first run
# (210 against 201 ms at N 16 with colour 'rgb') and none in the second (1.1-2.2x).  Each constant is the largest measured picture
# size with no loss at or below it in either run.
DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES = 14400
DCTN_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES = 489600


def _picture_batch_gate(count, samples, most):
    """What the three constants above mean, for ``count`` pictures whose planes hold ``samples`` samples each; ``most`` is
    the direction's DCTN_PICTURE_BATCH_*_MAX_SAMPLES as the caller reads it from this module."""
    gate = DCTN_PICTURE_BATCH_MIN_PICTURES
    return gate is not None and count >= max(gate, 2) and (most is None or samples <= most)


# dct_size 8 has a picture batch of its own (jpegx.batch_compress_pictures / batch_decompress_pictures: every block_size
# 1..255 and every picture size, the padding inside the device's gather) behind its OWN three gates, with the meaning of the
# DCTN_PICTURE_BATCH_* constants above and read when the functions are called.  The first ships as None -- the road is off and
# dct_size 8 is the loop, as it was (tests/test_picture_batch_dispatch.py pins that with only the DCTN_* gates set; the precedent
# is DCTN_ENTROPY_MIN_SAMPLES) -- and callers with many small pictures opt in by setting it: 2 is the measured value.
# Measured (profiles/batch_pictures_8.json and _run2.json, the batch road against the loop alternating call by
# call on one MI355X, block_size 4 and 1 with qtable, with colour 'rgb' and without, two runs): ONE picture loses compressing
# (0.22-0.26 against 0.16-0.18 ms at 64 x 64 and 128 x 128: the loop's one pooled picture job against two status reads and three
# allocations) and wins decompressing; with 2 pictures the batch wins all sixteen comparisons of either run (0.25-0.32 against
# 0.31-0.40 ms compressing, 0.17-0.22 against 0.49-0.65 ms back), with 4 by 1.8-5.4x, with 64 by 5.1-40x.  Compressing, it is
# 8.5-14x faster than the loop on 4096 pictures of 256 and of 4096 samples a plane and 1.03-1.24x on 256 pictures of 16 384; on 256
# of 262 144 each run has one loss (78.4 against 75.2 ms, 83.9 against 80.7 ms), and on 16 pictures of 752 000 and 12 M samples it
# loses 1.3-2.6x in both (np.stack and one pageable copy of 576 MB against the pooled picture jobs).  Decompressing, it wins
# everything measured in both runs: 24-88x on the 4096 pictures, 1.7-9.5x on the 256, 10-15x on 16 of 752 000 samples and
# 1.07-1.8x on 16 of 12 M.  Each _MAX_SAMPLES constant is the largest measured plane with no loss at or below it in either run;
# they take effect once DCT8_PICTURE_BATCH_MIN_PICTURES is set.
DCT8_PICTURE_BATCH_MIN_PICTURES = None
DCT8_PICTURE_BATCH_COMPRESS_MAX_SAMPLES = 16384
DCT8_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES = 12000000


def _picture_batch_gate_8(count, samples, most):
    """_picture_batch_gate for dct_size 8: ``most`` is the direction's DCT8_PICTURE_BATCH_*_MAX_SAMPLES as the caller reads it."""
    gate = DCT8_PICTURE_BATCH_MIN_PICTURES
    return gate is not None and count >= max(gate, 2) and (most is None or samples <= most)


def _stacked_pixels(images, config, colour):
    """The pictures as one uint8 array [n][rows][cols][3], or None: they are not all pictures the picture jobs take
    (_picture_size: three bands, one of its four modes, the configured size -- so all of one size; _picture_pixels) or, with
    colour 'rgb', not all of mode RGB.  One array [n][rows][cols][3] is n such pictures as it is."""
    if isinstance(images, np.ndarray):
        if images.ndim != 4 or images.dtype != np.uint8 or images.shape[1:] != (config.height, config.width, 3):
            return None
        return np.ascontiguousarray(images)
    if any(_picture_size(im, config) is None or (colour is not None and im.mode != "RGB") for im in images):
        return None
    pixels = [_picture_pixels(im) for im in images]     # the costly part of the vetting: last
    return None if any(p is None for p in pixels) else np.stack(pixels)


def _compress_picture_batch(images, config, colour):
    """The containers of the batch road, or None: the gate, the pictures or the configuration do not admit it, or libjpegx
    refused or failed -- the loop then names the picture and the fault.  dct_size 8 (the accelerated configuration) goes by
    _job_config_8, jpegx.padded_shape and the DCT8_* gates to jpegx.batch_compress_pictures, every other size by
    _compress_job_n, _blocked_shape and the DCTN_* gates to jpegx.batch_compress_pictures_n."""
    eight = _accelerated(config)
    gate = _picture_batch_gate_8 if eight else _picture_batch_gate
    most = DCT8_PICTURE_BATCH_COMPRESS_MAX_SAMPLES if eight else DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES
    count = len(images)
    if not gate(count, 0, most) or not _stock_registry() or not _device_usable():
        return None
    rows, cols = config.height, config.width
    if not isinstance(rows, (int, np.integer)) or not isinstance(cols, (int, np.integer)) or rows < 1 or cols < 1 \
            or rows * cols > 2 ** 31 - 1:
        return None
    import jpegx
    job = _job_config_8(config) if eight else _compress_job_n(config, rows, cols, 0)
    if job is None:
        return None
    shape = _none_on_refusal(jpegx.padded_shape, rows, cols, job[0]) if eight else _blocked_shape(rows, cols, job[0], job[1])
    if shape is None or not gate(count, shape[0] * shape[1], most) or 3 * count * shape[0] * shape[1] > 2 ** 31 - 1:
        return None
    stack = _stacked_pixels(images, config, colour)
    if stack is None:
        return None
    blobs = _none_on_refusal(jpegx.batch_compress_pictures if eight else jpegx.batch_compress_pictures_n, stack, *job, **_colour_kw(colour))
    if blobs is None:
        return None
    header = file_format.create_header(config)          # file_format.generate_data: the header, then <L length + bytes per band
    return [header + b"".join(file_format.pack_long(len(b)) + b for b in picture) for picture in blobs]


def _as_images(images, colour):
    """The pictures as the loop takes them: PIL images as they are, the slices of an array as mode YCbCr (RGB with colour 'rgb')."""
    if not isinstance(images, np.ndarray):
        return list(images)
    from PIL import Image
    return [Image.fromarray(a, mode="YCbCr" if colour is None else "RGB") for a in images]


def _check_colour(colour):
    if colour is not None and colour != "rgb":
        raise ValueError("colour must be None or 'rgb', got %r" % (colour,))


def compress_pictures(images, config, colour=None):
    """[Jpeg(config).compress(im) for im in images], byte for byte; with colour='rgb', [Jpeg(config).compress_rgb(im) ...].
    ``images``: a sequence of PIL images, or one uint8 array [n][rows][cols][3] taken as n pictures of mode YCbCr (RGB with
    colour='rgb').  At least DCTN_PICTURE_BATCH_MIN_PICTURES pictures that the picture jobs take (_picture_size,
    _picture_pixels; all of the configured size; with colour='rgb' all of mode RGB) whose planes hold at most
    DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES samples, under a configuration the device jobs admit (_compress_job_n: dct_size
    other than 8) go to the device as ONE batch; everything else, and every refusal of the batch -- a BadRleCodeError included,
    so that the failing picture is named as before -- is that loop.  dct_size 8 has the same road (_job_config_8: every
    block_size 1..255 and every picture size; jpegx.batch_compress_pictures) behind gates of its own,
    DCT8_PICTURE_BATCH_MIN_PICTURES and DCT8_PICTURE_BATCH_COMPRESS_MAX_SAMPLES; the first ships as None, so dct_size 8 is the
    loop until a caller sets it."""
    _check_colour(colour)
    if not isinstance(images, np.ndarray):
        images = list(images)
    whole = _compress_picture_batch(images, config, colour) if len(images) else None
    if whole is not None:
        return whole
    codec = Jpeg(config)
    return [codec.compress(im) if colour is None else codec.compress_rgb(im) for im in _as_images(images, colour)]


def _container_bands(container, header):
    """The three coded bands of a container that starts with ``header``, or None: it is no bytes object, carries another
    header or does not hold three whole length-prefixed bands."""
    if not isinstance(container, (bytes, bytearray)) or not container.startswith(header):
        return None
    bands, at = [], len(header)
    for _ in range(3):
        if at + 4 > len(container):
            return None
        size = file_format.unpack_long(container[at:at + 4])
        if at + 4 + size > len(container):
            return None
        bands.append(bytes(container[at + 4:at + 4 + size]))
        at += 4 + size
    return bands


def _decompress_picture_batch(containers, colour):
    """uint8 [n][height][width][3] by the batch road, or None (see _compress_picture_batch): all containers carry one and
    the same header and coded bands, and _decompress_job_n -- for dct_size 8 _decode_job_8 -- admits the configuration."""
    count = len(containers)
    if not (_picture_batch_gate(count, 0, None) or _picture_batch_gate_8(count, 0, None)) or not _stock_registry() or not _device_usable():
        return None                                     # neither road's count gate admits them: nothing is parsed
    first = containers[0]
    if not isinstance(first, (bytes, bytearray)) or len(first) < 2:
        return None
    header = bytes(first[:file_format.unpack_integer(first[:2])])
    blobs = [_container_bands(c, header) for c in containers]
    if any(b is None for b in blobs):
        return None
    try:
        config = file_format.get_header(header)
    except Exception:
        return None                                     # the loop names the fault
    import jpegx
    if _accelerated(config):
        most = DCT8_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES
        job = _decode_job_8(config) if _picture_batch_gate_8(count, 0, most) else None
        if job is None or not all(_is_coded(b) for picture in blobs for b in picture):
            return None
        bs, mode, param = job[2:]
        shape = _none_on_refusal(jpegx.padded_shape, config.height, config.width, bs)
        if shape is None or not _picture_batch_gate_8(count, shape[0] * shape[1], most) or 3 * count * shape[0] * shape[1] > 2 ** 31 - 1:
            return None
        return _none_on_refusal(jpegx.batch_decompress_pictures, blobs, config.height, config.width, bs, mode, param, **_colour_kw(colour))
    most = DCTN_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES
    if not _picture_batch_gate(count, 0, most):
        return None
    job = _decompress_job_n(config, [b for picture in blobs for b in picture], 0)
    if job is None:
        return None
    h, w = _blocked_shape(*job[:4])
    if not _picture_batch_gate(count, h * w, most) or 3 * count * h * w > 2 ** 31 - 1:
        return None
    return _none_on_refusal(jpegx.batch_decompress_pictures_n, blobs, *job, **_colour_kw(colour))


def decompress_pictures_u8(containers, colour=None):
    """[np.asarray(Jpeg.decompress(c)) for c in containers] as uint8 arrays (height, width, 3), sample for sample; with
    colour='rgb', of Jpeg.decompress_rgb(c).  The batch road under the conditions of compress_pictures (containers that all
    carry one and the same header and coded bands in place of the pictures; DCTN_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES; a
    whole divisor, as the decoding jobs ask; dct_size 8: _decode_job_8 and DCT8_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES), else that
    loop, which names the container and the fault."""
    _check_colour(colour)
    containers = list(containers)
    stack = _decompress_picture_batch(containers, colour) if containers else None
    if stack is not None:
        return list(stack)
    return [np.asarray(Jpeg.decompress(c) if colour is None else Jpeg.decompress_rgb(c)) for c in containers]


def decompress_pictures(containers, colour=None):
    """decompress_pictures_u8 as PIL images of mode YCbCr (RGB with colour='rgb')."""
    from PIL import Image
    return [Image.fromarray(a, mode="YCbCr" if colour is None else "RGB") for a in decompress_pictures_u8(containers, colour)]


# ---------------------------------------------------------------------------------------------------------------------
# many pictures of unequal sizes at once: each under the same settings at its own size
# ---------------------------------------------------------------------------------------------------------------------
# compress_picture_set / decompress_picture_set_u8 send the pictures that the picture jobs admit to the device as ONE set
# (jpegx.batch_compress_picture_set_n / batch_decompress_picture_set_n, dct_size other than 8: one flat upload, one launch chain
# and one download whatever the sizes) from this many admitted pictures on; None: the road is off and the functions are a loop
# over Jpeg.compress / compress_rgb / decompress / decompress_rgb with a Configuration of each picture's own size.  Never below
# 2: one picture is what those are for.  All three constants are read when the functions are called.
# Measured (profiles/batch_picture_set_n.json and, a second run of the same code, _run2.json; figures of the first,
# the second agrees on every verdict here; pictures with sides between 64 and 128 at N 4 and N 16, with colour 'rgb' and
# without, the set road against the loop, alternating call by call on one MI355X, 12 rounds): even ONE picture through the set
# won all eight comparisons of either run (0.29-0.30 against 0.52-0.78 ms compressing, 0.23-0.31 against 0.28-0.35 ms
# decompressing: the loop's picture jobs start at 16 384 samples a plane, most of these planes are smaller); with 2 pictures it wins
# 2.7-3.8x / 1.6-2.0x, with 4 5.6-7.3x / 1.9-3.7x, with 16 9.2-11.8x / 5.4-5.9x, with 64 17-21x / 11-13x.  The smallest count with no
# loss at or above it is the smallest the constant may take.
DCTN_PICTURE_SET_MIN_PICTURES = 2

# ... and only when the LARGEST plane of the set (H * W of one band of one picture after both paddings) holds at most this
# many samples; None: no upper limit.  The set pays its launches and copies once, and copies all pixels into one flat array
# that moves through pageable memory in one piece, while the picture jobs of the loop stream through the pool's pinned staging.
# Measured (the same two records): compressing, the set is 18-23x faster than the loop on 4096 pictures with sides 48..96 (planes
# of at most 9216 samples) and 7.4-10x on 256 with sides 384..640 at bs 5 N 24 (at most 20 736 samples) in both runs; on the same
# 256 pictures at bs 1 (up to 399 360 samples) it is 1.2-1.4x faster at N 4 and lost at N 16 in both runs (100-106 against 96-97 ms,
# 87.3 against 86.8 ms); on 16 pictures near 3000 x 4000 it is 2.4-4.2x slower at 489 600 and at 12 M samples.  Decompressing, it
# won every comparison of either run: 12-17x on the 4096 pictures, 2.0-41x on the 256, 1.8-9.6x on the 16 (planes of up to
# 12 032 000 samples).  Each constant is the largest measured plane with no loss at or below it in either run.
DCTN_PICTURE_SET_COMPRESS_MAX_SAMPLES = 20736
DCTN_PICTURE_SET_DECOMPRESS_MAX_SAMPLES = 12032000


def _picture_set_gate(count, samples, most):
    """What the three constants above mean, for ``count`` admitted pictures whose largest plane holds ``samples`` samples."""
    gate = DCTN_PICTURE_SET_MIN_PICTURES
    return gate is not None and count >= max(gate, 2) and (most is None or samples <= most)


# dct_size 8 has a picture set of its own (jpegx.batch_compress_picture_set / batch_decompress_picture_set: every block_size
# 1..255, the qtable quantiser included; block_size 1, 2, 4 through the raw uint8 block strip and the sized uint8 forward kernel)
# behind its OWN three gates, with the meaning of the DCTN_PICTURE_SET_* constants above and read when the functions are
# called.  The first ships as None -- the road is off and dct_size 8 is the loop, as it was (tests/test_picture_set_dispatch.py
# pins that with only the DCTN_* gates set; the precedent is DCT8_PICTURE_BATCH_MIN_PICTURES) -- and callers with many small
# pictures opt in by setting it: 4 is the measured value.
# Measured (profiles/batch_picture_set_8.json and, a second run of the same code, _run2.json; the set road
# against the loop alternating call by call on one MI355X, colour 'rgb', qtable, block_size 4 and 1, 3 rounds, both size gates
# lifted): with 2 pictures of sides 64..128 the set lost compressing once in four comparisons (0.382 against 0.379 ms at
# block_size 1 in the second run; 0.34-0.35 against 0.35-0.37 ms in the others) and won decompressing 7.3-8.1x; with 4 it wins
# 1.77-2.06x / 8.0-8.6x, with 16 3.9-4.1x / 16-23x, with 64 4.4-5.3x / 22-29x; 4096 pictures of sides 48..96 go 5.7-6.3x /
# 19-28x faster (101-127 against 634-751 ms, 101-148 against 2800-2870 ms).  Compressing 256 pictures of sides 384..640 the
# set LOSES in both runs at block_size 4 (102-108 against 77-79 ms; planes of up to 25 600 samples) and at block_size 1 (115-120
# against 101-103 ms; up to 404 480 samples): one flat pageable copy against the pooled picture jobs.  Compressing 16 pictures
# near 3000 x 4000 it wins at block_size 4 (286-287 against 304-365 ms; 752 000 samples) and loses 6.5-6.9x at block_size 1
# (734-753 against 109-112 ms; 11 976 000 samples).  Decompressing, it won every comparison of either run from 2 pictures on:
# 8.8-45x on the 256 pictures, 18-23x (block_size 4) and 2.6-3.0x (block_size 1) on the 16 large ones.  Each _MAX_SAMPLES
# constant is the largest measured plane with no loss at or below it in either run, from 4 pictures on.  They take effect once
# DCT8_PICTURE_SET_MIN_PICTURES is set.
DCT8_PICTURE_SET_MIN_PICTURES = None
DCT8_PICTURE_SET_COMPRESS_MAX_SAMPLES = 15360
DCT8_PICTURE_SET_DECOMPRESS_MAX_SAMPLES = 11976000


def _picture_set_gate_8(count, samples, most):
    """_picture_set_gate for dct_size 8: ``most`` is the direction's DCT8_PICTURE_SET_*_MAX_SAMPLES as the caller reads it."""
    gate = DCT8_PICTURE_SET_MIN_PICTURES
    return gate is not None and count >= max(gate, 2) and (most is None or samples <= most)


def _sized(config, rows, cols):
    """``config`` with the picture's own width and height, as cli.py makes one per picture."""
    return Configuration(width=cols, height=rows, block_size=config.block_size, dct_size=config.dct_size, transform=config.transform,
                         quantization=config.quantization)


def _compress_picture_set(images, config, colour):
    """{index: container} of the pictures that went to the device as one set; empty where the gates, the configuration or
    libjpegx say no -- the loop then names the picture and the fault.  dct_size 8 (the accelerated configuration) goes by
    _job_config_8, jpegx.padded_shape and the DCT8_* gates to jpegx.batch_compress_picture_set, every other size by
    _compress_job_n, _blocked_shape and the DCTN_* gates to jpegx.batch_compress_picture_set_n."""
    eight = _accelerated(config)
    gate = _picture_set_gate_8 if eight else _picture_set_gate
    most = DCT8_PICTURE_SET_COMPRESS_MAX_SAMPLES if eight else DCTN_PICTURE_SET_COMPRESS_MAX_SAMPLES
    if not gate(len(images), 0, most) or not _stock_registry() or not _device_usable():
        return {}
    if eight and not isinstance(config.block_size, (int, np.integer)):
        return {}                                       # the table takes whole block sizes; 2.0 is the loop's
    import jpegx
    admitted, job = [], None                            # (index, rows, cols)
    for at, im in enumerate(images):
        try:
            rows, cols = im.height, im.width
        except Exception:
            continue
        if not isinstance(rows, (int, np.integer)) or not isinstance(cols, (int, np.integer)) or rows < 1 or cols < 1 or rows * cols > 2 ** 31 - 1:
            continue
        sized = _sized(config, rows, cols)
        if _picture_size(im, sized) is None or (colour is not None and im.mode != "RGB"):
            continue
        this = _job_config_8(sized) if eight else _compress_job_n(sized, rows, cols, 0)
        if this is None:
            continue
        job = this                                      # (block_size, [dct_size,] mode, param): the same for every picture
        admitted.append((at, rows, cols))
    if not admitted:
        return {}
    if eight:
        shapes = [_none_on_refusal(jpegx.padded_shape, rows, cols, job[0]) for _, rows, cols in admitted]
        if any(s is None for s in shapes):
            return {}
    else:
        shapes = [_blocked_shape(rows, cols, job[0], job[1]) for _, rows, cols in admitted]
    if not gate(len(admitted), max(h * w for h, w in shapes), most) or 3 * sum(h * w for h, w in shapes) > 2 ** 31 - 1:
        return {}
    pixels = [_picture_pixels(images[at]) for at, _, _ in admitted]      # the costly part of the vetting: last
    keep = [k for k, p in enumerate(pixels) if p is not None]
    if len(keep) != len(pixels):
        admitted, pixels = [admitted[k] for k in keep], [pixels[k] for k in keep]
        if not gate(len(admitted), 0, None):
            return {}
    blobs = _none_on_refusal(jpegx.batch_compress_picture_set if eight else jpegx.batch_compress_picture_set_n, pixels, *job, **_colour_kw(colour))
    if blobs is None:
        return {}
    out = {}
    for (at, rows, cols), picture in zip(admitted, blobs):
        header = file_format.create_header(_sized(config, rows, cols))   # file_format.generate_data: the header, then <L length + bytes per band
        out[at] = header + b"".join(file_format.pack_long(len(b)) + b for b in picture)
    return out


def compress_picture_set(images, config, colour=None):
    """[Jpeg(config_p).compress(im) for im in images], byte for byte, where config_p is ``config`` with the picture's own width
    and height (``config``'s own are not read); with colour='rgb', compress_rgb.  The pictures that the picture jobs admit
    (_picture_size, _picture_pixels, _compress_job_n with the picture's size -- so planes of at least DCTN_MIN_SAMPLES samples,
    dct_size other than 8; with colour='rgb' of mode RGB) go to the device as ONE set when there are at least
    DCTN_PICTURE_SET_MIN_PICTURES of them and the largest plane holds at most DCTN_PICTURE_SET_COMPRESS_MAX_SAMPLES samples; every
    other picture, and every picture after a refusal of the set -- a BadRleCodeError included -- goes through the loop, which
    names it.  Results come back in input order.  dct_size 8 has the same road (_job_config_8: every block_size 1..255;
    jpegx.batch_compress_picture_set) behind gates of its own, DCT8_PICTURE_SET_MIN_PICTURES and
    DCT8_PICTURE_SET_COMPRESS_MAX_SAMPLES; the first ships as None, so dct_size 8 is the loop until a caller sets it."""
    _check_colour(colour)
    images = list(images)
    done = _compress_picture_set(images, config, colour) if images else {}
    out = []
    for at, im in enumerate(images):
        if at in done:
            out.append(done[at])
        else:
            codec = Jpeg(_sized(config, im.height, im.width))
            out.append(codec.compress(im) if colour is None else codec.compress_rgb(im))
    return out


def _decompress_picture_set(containers, colour):
    """{index: uint8 pixels} of the containers that went to the device as one set (see _compress_picture_set): containers whose
    headers differ in width and height alone, with coded bands, under a configuration _decompress_job_n -- for dct_size 8
    _decode_job_8 -- admits, each kind behind its own gates."""
    count = len(containers)
    if not (_picture_set_gate(count, 0, None) or _picture_set_gate_8(count, 0, None)) or not _stock_registry() or not _device_usable():
        return {}                                       # neither road's count gate admits them: nothing is parsed
    admitted, blobs, rest, job, eight = [], [], None, None, False
    for at, box in enumerate(containers):
        if not isinstance(box, (bytes, bytearray)) or len(box) < 6:
            continue
        header = bytes(box[:file_format.unpack_integer(box[:2])])
        if len(header) < 6 or (rest is not None and header[:2] + header[6:] != rest):
            continue
        bands = _container_bands(box, header)
        if bands is None:
            continue
        try:
            sized = file_format.get_header(header)
        except Exception:
            continue                                    # the loop names the fault
        if _accelerated(sized):                         # the rest of the header is shared: one kind per set
            if not _picture_set_gate_8(count, 0, None) or not isinstance(sized.block_size, (int, np.integer)):
                continue
            this = _decode_job_8(sized)
            if this is None or not all(_is_coded(b) for b in bands):
                continue
            this = (sized.height, sized.width) + tuple(this[2:])
        else:
            if not _picture_set_gate(count, 0, None):
                continue
            this = _decompress_job_n(sized, bands, 0)
            if this is None:
                continue
        if rest is None:
            rest, job, eight = header[:2] + header[6:], this[2:], _accelerated(sized)
        admitted.append((at, this[0], this[1]))
        blobs.append(bands)
    if not admitted:
        return {}
    import jpegx
    gate = _picture_set_gate_8 if eight else _picture_set_gate
    most = DCT8_PICTURE_SET_DECOMPRESS_MAX_SAMPLES if eight else DCTN_PICTURE_SET_DECOMPRESS_MAX_SAMPLES
    if eight:
        shapes = [_none_on_refusal(jpegx.padded_shape, rows, cols, job[0]) for _, rows, cols in admitted]
        if any(s is None for s in shapes):
            return {}
    else:
        shapes = [_blocked_shape(rows, cols, job[0], job[1]) for _, rows, cols in admitted]
    if not gate(len(admitted), max(h * w for h, w in shapes), most) or 3 * sum(h * w for h, w in shapes) > 2 ** 31 - 1:
        return {}
    entry = jpegx.batch_decompress_picture_set if eight else jpegx.batch_decompress_picture_set_n
    back = _none_on_refusal(entry, blobs, [(rows, cols) for _, rows, cols in admitted], *job, **_colour_kw(colour))
    if back is None:
        return {}
    return {at: a for (at, _, _), a in zip(admitted, back)}


def decompress_picture_set_u8(containers, colour=None):
    """[np.asarray(Jpeg.decompress(c)) for c in containers] as uint8 arrays (height_p, width_p, 3), sample for sample; with
    colour='rgb', of Jpeg.decompress_rgb(c).  The containers may differ in width and height and in nothing else of the header:
    those that share the rest of the first admitted one's header, hold coded bands and pass _decompress_job_n go to the device
    as ONE set under the gates of compress_picture_set (DCTN_PICTURE_SET_DECOMPRESS_MAX_SAMPLES); every other container, and all
    of them after a refusal of the set, go through the loop, which names the container and the fault."""
    _check_colour(colour)
    containers = list(containers)
    done = _decompress_picture_set(containers, colour) if containers else {}
    return [done[at] if at in done else np.asarray(Jpeg.decompress(c) if colour is None else Jpeg.decompress_rgb(c))
            for at, c in enumerate(containers)]


def decompress_picture_set(containers, colour=None):
    """decompress_picture_set_u8 as PIL images of mode YCbCr (RGB with colour='rgb')."""
    from PIL import Image
    return [Image.fromarray(a, mode="YCbCr" if colour is None else "RGB") for a in decompress_picture_set_u8(containers, colour)]


# ---------------------------------------------------------------------------------------------------------------------
# what a divisor costs in bytes, and compressing to a byte budget
# ---------------------------------------------------------------------------------------------------------------------
# probe_picture_sizes takes the device road (jpegx.batch_probe_pictures_n: one upload, one gather and one forward pass per
# group of pictures, every candidate divisor quantised and sized from the coefficients in LDS, one download of the sums) from
# this many divisors on; None: the road is off and the function is the loop over Jpeg.compress.  Read when the function is
# called.  Never below 1.
# Measured (profiles/probe_sizes_n.json and, a second run of the same code, _run2.json; 1 and 8 pictures of
# 64 x 64 and 512 x 512 at N 4 and N 16, the probe against the loop alternating call by call on one MI355X): with ONE divisor
# the probe loses on one 512 x 512 picture in both runs (0.50-0.54 against 0.36 ms: the loop's pooled picture job against three
# allocations and a pageable copy) and wins the other comparisons; with 2 divisors it wins all of them in both runs (1.26-34x),
# with 4 by 2.4-50x, with 16 by 7.9-151x.  On device buffers the probe is 1.6-1.9x faster than 2 sizes-only compressions at
# every measured shape (4096 pictures of 64 x 64, 256 of 512 x 512, 16 of 3000 x 4000; N 4, 16, 24) and 0.85-1.16x with one
# candidate.  The smallest measured count with no loss at or above it; no plane size lost at every count, so there is no size
# gate beyond DCTN_MIN_SAMPLES.
DCTN_PROBE_MIN_CANDIDATES = 2
# dct_size 8 has a size probe of its own (jpegx.batch_probe_pictures: csrc/jpegx_probe_8.hip, the float64 tier of the 8x8 roads
# with the stream left out, so its sizes are the roads' sizes, exact rounding ties included) behind a gate of its OWN, with the
# meaning of the constant above and read when the function is called.  It ships as None -- the road is off and dct_size 8 is the
# loop, as it was (tests/test_probe_dispatch.py pins that with only the DCTN_* gates set; the precedent is
# DCT8_PICTURE_BATCH_MIN_PICTURES) -- and a caller opts in by setting it.
# Measured (microbench/probe_8.py, profiles/probe_8.json and, a second run of the same code, _run2.json; 1 and 8
# pictures of 64 x 64 and 512 x 512 at block_size 4 and 1, the probe against the loop alternating call by call on one MI355X):
# with ONE divisor the probe loses on one 512 x 512 picture at block_size 1 (0.44 against 0.37 and 0.31 ms) and wins the
# other comparisons; from 2 divisors on it won every comparison of both runs (1.4-11x with 2, 8.3-47x with 16).  By the
# rule of the constant above -- the smallest measured count with no loss at or above it in either run -- this gate would stand at 2.
DCT8_PROBE_MIN_CANDIDATES = None


class TargetSizeError(ValueError):
    """No candidate divisor brings the picture within the byte budget."""


def _checked_divisors(config, divisors):
    """The candidate divisors as plain Python numbers; ValueError for a configuration that is not 'divide' and for a divisor
    that is not a whole positive number (_whole_divisor: the device jobs restore such a one as the reference does)."""
    if getattr(config.quantization, "name", None) != "divide":
        raise ValueError("the size probe varies the divisor: config.quantization must be 'divide', got %r"
                         % (getattr(config.quantization, "name", None),))
    out = []
    for d in divisors:
        whole = isinstance(d, (int, float, np.integer, np.floating)) and not isinstance(d, (bool, np.bool_)) \
            and np.isfinite(d) and d > 0 and _whole_divisor(("divide", float(d)))
        if not whole:
            raise ValueError("a candidate divisor must be a whole positive number, got %r" % (d,))
        out.append(d.item() if isinstance(d, np.generic) else d)
    return out


def _divide_config(config, divisor):
    """``config`` with QuantizationMethod('divide', divisor=divisor)."""
    return Configuration(width=config.width, height=config.height, block_size=config.block_size, dct_size=config.dct_size,
                         transform=config.transform, quantization=QuantizationMethod("divide", divisor=divisor))


def _compress_one(image, config, colour):
    codec = Jpeg(config)
    return codec.compress(image) if colour is None else codec.compress_rgb(image)


def _probe_loop(images, config, divisors, colour):
    """The literal loop: len(Jpeg(config_j).compress(image_i)), -1 where it raises the reference's BadRleCodeError."""
    import util
    images = _as_images(images, colour)
    out = np.empty((len(images), len(divisors)), dtype=np.int64)
    for j, d in enumerate(divisors):
        cfg = _divide_config(config, d)
        for i, im in enumerate(images):
            try:
                out[i, j] = len(_compress_one(im, cfg, colour))
            except util.BadRleCodeError:
                out[i, j] = -1
    return out


def _probe_job(images, config, divisors, colour, gate_n, gate_8):
    """(the pictures as _stacked_pixels gives them, the entry's arguments between them and the mode, dct_size 8?) for the two
    probe roads, or None: the gate, the configuration or the pictures do not admit the road.  ``gate_n`` and ``gate_8`` are the
    function's DCTN_* and DCT8_* constants as it reads them from this module.  dct_size 8 (the accelerated configuration) goes by
    _job_config_8, the quantiser 'divide', a usable device and jpegx.padded_shape to the entries without n, (block_size,);
    every other size by _job_sizes, _blocked_shape and dctn_on_device to the _n entries, (block_size, dct_size)."""
    eight = _accelerated(config)
    gate = gate_8 if eight else gate_n
    count = len(images)
    if gate is None or len(divisors) < max(gate, 1) or count < 1 or not _stock_registry():
        return None
    rows, cols = config.height, config.width
    if not isinstance(rows, (int, np.integer)) or not isinstance(cols, (int, np.integer)) or rows < 1 or cols < 1 \
            or rows * cols > 2 ** 31 - 1:
        return None
    if eight:
        job = _job_config_8(config)
        # _job_config_8 lets a block_size such as 2.0 through; the container's header does not (the loop raises), so neither
        # does this road: an integer, as _job_sizes asks of the other sizes
        if job is None or job[1] != "divide" or not isinstance(job[0], (int, np.integer)) or not _device_usable():
            return None
        import jpegx
        head = (int(job[0]),)
        shape = _none_on_refusal(jpegx.padded_shape, rows, cols, head[0])
        if shape is None:
            return None
        h, w = shape
    else:
        head = _job_sizes(config)                        # transform 'DCT', dct_size 2..32 but 8, a usable device
        if head is None:
            return None
        h, w = _blocked_shape(rows, cols, *head)
        if not dctn_on_device(config, h * w):
            return None
    if 3 * count * h * w > 2 ** 31 - 1:
        return None
    stack = _stacked_pixels(images, config, colour)
    return None if stack is None else (stack, head, eight)


def _probe_device(images, config, divisors, colour):
    """The sizes from jpegx.batch_probe_pictures_n -- at dct_size 8 from jpegx.batch_probe_pictures --, or None: the gate, the
    configuration or the pictures do not admit the road (_probe_job), or libjpegx refused or failed."""
    job = _probe_job(images, config, divisors, colour, DCTN_PROBE_MIN_CANDIDATES, DCT8_PROBE_MIN_CANDIDATES)
    if job is None:
        return None
    stack, head, eight = job
    import jpegx
    entry = jpegx.batch_probe_pictures if eight else jpegx.batch_probe_pictures_n
    out = np.empty((len(stack), len(divisors)), dtype=np.int64)
    for at in range(0, len(divisors), jpegx.PROBE_MAX_CANDIDATES):
        some = divisors[at:at + jpegx.PROBE_MAX_CANDIDATES]
        got = _none_on_refusal(entry, stack, *head, "divide", [float(d) for d in some], **_colour_kw(colour))
        if got is None:
            return None
        coded, bad = got
        # file_format.generate_data: the header, whose JSON changes length with the divisor's digits, then <L length + bytes per band
        heads = np.array([len(file_format.create_header(_divide_config(config, d))) for d in some], dtype=np.int64)
        part = coded.sum(axis=1).astype(np.int64) + heads[None, :] + 3 * 4
        part[bad.any(axis=1)] = -1
        out[:, at:at + len(some)] = part
    return out


def probe_picture_sizes(images, config, divisors, colour=None):
    """int64 [len(images)][len(divisors)]: entry [i][j] is len(Jpeg(config_j).compress(images[i])) -- with colour='rgb', of
    compress_rgb -- where config_j is ``config`` with QuantizationMethod('divide', divisor=divisors[j]); -1 where that call
    raises BadRleCodeError.  The header and the 12 bytes of length prefixes are counted.  ``images`` as compress_pictures takes
    them.  ValueError for a configuration that is not 'divide' and for a divisor that is not a whole positive number.
    With at least DCTN_PROBE_MIN_CANDIDATES divisors, dct_size other than 8 with transform 'DCT', the stock steps, a usable
    device, pictures that _stacked_pixels accepts and planes of at least DCTN_MIN_SAMPLES samples, all divisors are sized on the
    device in one pass per 32 of them (jpegx.batch_probe_pictures_n); everything else, and every refusal, is the loop.
    dct_size 8 has the same road (_job_config_8, jpegx.batch_probe_pictures) behind a gate of its own,
    DCT8_PROBE_MIN_CANDIDATES, which ships as None: dct_size 8 is the loop until a caller sets it."""
    _check_colour(colour)
    divisors = _checked_divisors(config, divisors)
    if not isinstance(images, np.ndarray):
        images = list(images)
    sizes = _probe_device(images, config, divisors, colour) if len(divisors) else None
    return sizes if sizes is not None else _probe_loop(images, config, divisors, colour)


def _geometric(lo, hi, probes):
    """``probes`` whole numbers spaced geometrically from lo to hi inclusive, deduplicated and ascending."""
    if probes < 2 or lo == hi:
        return sorted({lo, hi})
    ratio = float(hi) / float(lo)
    return sorted({lo, hi} | {min(hi, max(lo, int(round(lo * ratio ** (i / (probes - 1.0)))))) for i in range(1, probes - 1)})


def _between(g, f, probes):
    """Up to ``probes`` of the whole numbers strictly between g and f, evenly spaced by index; all of them if that many or fewer."""
    m = f - g - 1
    if m <= probes:
        return list(range(g + 1, f))
    if probes < 2:
        return [g + 1 + (m - 1) // 2]
    return sorted({g + 1 + (i * (m - 1)) // (probes - 1) for i in range(probes)})


def _fits(size, max_bytes):
    return size != -1 and size <= max_bytes


def compress_to_size(image, config, max_bytes, colour=None, lo=1, hi=4096, probes=16, rounds=3):
    """(container, divisor): ``image`` compressed under ``config`` with the smallest 'divide' divisor the search below finds
    whose container holds at most ``max_bytes`` bytes; the container is Jpeg(config_divisor).compress(image) (compress_rgb with
    colour='rgb').  The search is deterministic and costs 1 + ``rounds`` calls of probe_picture_sizes at most:
      1. candidates: ``probes`` whole numbers spaced geometrically from ``lo`` to ``hi`` inclusive;
      2. f = the smallest candidate whose size is neither -1 (BadRleCodeError) nor above max_bytes -- none: TargetSizeError;
         g = the candidate just below f, or lo - 1;
      3. while rounds remain and whole numbers lie strictly between g and f: up to ``probes`` of them, evenly spaced, are
         probed; f becomes the smallest of them that fits (it stays if none does), g the probed number just below the new f (the
         old g if there is none);
      4. compress with f; RuntimeError if the container's length is not the probed one.
    Sizes need not fall monotonically with the divisor: f is the smallest FITTING number the search has seen above a number
    that does not fit, not a global minimum."""
    _check_colour(colour)
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (lo, hi, probes, rounds)) \
            or lo < 1 or hi < lo or probes < 1 or rounds < 0:
        raise ValueError("compress_to_size: lo, hi, probes and rounds must be whole numbers with 1 <= lo <= hi, probes >= 1, rounds >= 0")
    lo, hi, probes, rounds = int(lo), int(hi), int(probes), int(rounds)
    seen = {}                                            # divisor -> probed size

    def probe(candidates):
        sizes = probe_picture_sizes([image], config, candidates, colour)[0]
        seen.update((d, int(s)) for d, s in zip(candidates, sizes))

    candidates = _geometric(lo, hi, probes)
    probe(candidates)
    fitting = [d for d in candidates if _fits(seen[d], max_bytes)]
    if not fitting:
        coded = [(s, d) for d, s in seen.items() if s != -1]
        if not coded:
            raise TargetSizeError("no divisor in %d..%d codes the picture at all (BadRleCodeError at every candidate)" % (lo, hi))
        raise TargetSizeError("no divisor in %d..%d brings the picture within %d bytes: the smallest size seen is %d bytes, at divisor %d"
                              % ((lo, hi, max_bytes) + min(coded)))
    f = fitting[0]
    g = max([d for d in candidates if d < f], default=lo - 1)
    for _ in range(rounds):
        inner = _between(g, f, probes)
        if not inner:
            break
        probe(inner)
        fitting = [d for d in inner if _fits(seen[d], max_bytes)]
        if fitting:
            f = fitting[0]
        g = max([d for d in inner if d < f], default=g)
    container = _compress_one(image, _divide_config(config, f), colour)
    if len(container) != seen[f]:
        raise RuntimeError("compress_to_size: divisor %d was probed at %d bytes, its container holds %d" % (f, seen[f], len(container)))
    return container, f


def compress_pictures_to_size(images, config, max_bytes, divisors, colour=None):
    """(containers, chosen): every picture compressed with the smallest divisor of the ascending ladder ``divisors`` (at most
    32 rungs) that brings its container within ``max_bytes`` bytes; chosen[i] is picture i's divisor and containers[i] equals
    Jpeg(config_chosen[i]).compress(images[i]) (compress_rgb with colour='rgb'), byte for byte.  ONE probe_picture_sizes call
    sizes the whole batch on every rung; the pictures of a rung are then one compress_pictures call.  TargetSizeError names
    the first picture that fits no rung."""
    _check_colour(colour)
    ladder = _checked_divisors(config, divisors)
    if not 1 <= len(ladder) <= 32 or any(b <= a for a, b in zip(ladder, ladder[1:])):
        raise ValueError("compress_pictures_to_size: divisors must be 1..32 ascending rungs")
    if not isinstance(images, np.ndarray):
        images = list(images)
    sizes = probe_picture_sizes(images, config, ladder, colour)
    rung = []
    for i, row in enumerate(sizes):
        fitting = [j for j, s in enumerate(row) if _fits(int(s), max_bytes)]
        if not fitting:
            coded = [(int(s), ladder[j]) for j, s in enumerate(row) if s != -1]
            raise TargetSizeError("picture %d fits no rung within %d bytes%s" % (
                i, max_bytes, ": its smallest size is %d bytes, at divisor %d" % min(coded) if coded else " (BadRleCodeError at every rung)"))
        rung.append(fitting[0])
    containers = [None] * len(rung)
    for j in sorted(set(rung)):
        members = [i for i, r in enumerate(rung) if r == j]
        group = images[members] if isinstance(images, np.ndarray) else [images[i] for i in members]
        for i, c in zip(members, compress_pictures(group, _divide_config(config, ladder[j]), colour)):
            containers[i] = c
    return containers, [ladder[j] for j in rung]


# ---------------------------------------------------------------------------------------------------------------------
# what a divisor costs in quality, and compressing to a PSNR floor
# ---------------------------------------------------------------------------------------------------------------------
# probe_picture_distortion takes the device road (jpegx.batch_probe_distortion_pictures_n: one upload, two gathers and one pass
# of the distortion kernel per group of pictures, every candidate divisor quantised, restored, inverted and compared from the
# coefficients in LDS, one download of the sums) from this many divisors on; None: the road is off and the function is the
# loop over Jpeg.compress and Jpeg.decompress.  Read when the function is called.  Never below 1.
# Measured (profiles/probe_distortion_n.json and, a second run of the same code, _run2.json; 1 and 8 pictures
# of 64 x 64 and 512 x 512 at N 4 and N 16, the probe against the loop alternating call by call on one MI355X): the probe won
# every comparison of both runs, with ONE divisor already (0.12-0.13 against 0.59-0.61 ms on one 64 x 64 picture, 0.74-0.82
# against 5.7-6.0 ms on one 512 x 512 picture, 2.5-2.6 against 38-40 ms on eight: 4.7-28x), with 2 by 9-49x, with 16 by 52-310x:
# the loop pays a compression, a decompression and a NumPy comparison per divisor.  On device buffers, against K bare
# forward-plus-inverse kernel pairs without gather, way back or comparison (a lower bound no caller of pipeline has), one
# candidate loses (0.39-0.78x) and the probe wins from 2 on at block_size 1 (1.04-1.22x; 2.0-2.7x at 32) and from 4-16 on at bs
# 5 N 24.  The smallest measured count with no loss against the loop at or above it; no plane size lost at any count, so there
# is no size gate beyond DCTN_MIN_SAMPLES.
DCTN_DISTORTION_MIN_CANDIDATES = 1
# The same at dct_size 8 (jpegx.batch_probe_distortion_pictures), behind a gate of its own that ships as None: the road is off
# and dct_size 8 is the loop, as it was (tests/test_distortion_dispatch.py pins that) until a caller sets it.  Measured (DESIGN.md
# 4.27, profiles/probe_8.json and _run2.json, the shapes of DCT8_PROBE_MIN_CANDIDATES): the probe won every comparison against
# the loop, 3.1-17x with one divisor and 23-178x with 16; by the rule of the constant above the gate would stand at 1.
DCT8_DISTORTION_MIN_CANDIDATES = None


class TargetQualityError(ValueError):
    """No candidate divisor keeps the picture at or above the PSNR floor."""


def _distortion_loop(images, config, divisors, colour):
    """The literal loop: per band the squared differences between the picture as the codec is handed it and
    Jpeg(config_j).decompress(Jpeg(config_j).compress(picture)), -1 where compressing raises the reference's BadRleCodeError."""
    import util
    images = _as_images(images, colour)
    out = np.empty((len(images), 3, len(divisors)), dtype=np.int64)
    for i, im in enumerate(images):
        x = im if colour is None else im.convert("YCbCr")
        ref = np.asarray(x).astype(np.int64)
        for j, d in enumerate(divisors):
            codec = Jpeg(_divide_config(config, d))
            try:
                back = np.asarray(codec.decompress(codec.compress(x))).astype(np.int64)
            except util.BadRleCodeError:
                out[i, :, j] = -1
                continue
            out[i, :, j] = ((back - ref) ** 2).sum(axis=(0, 1))
    return out


def _distortion_device(images, config, divisors, colour):
    """The sums from jpegx.batch_probe_distortion_pictures_n -- at dct_size 8 from jpegx.batch_probe_distortion_pictures --, or
    None: the gate, the configuration or the pictures do not admit the road (_probe_job), or libjpegx refused or failed."""
    job = _probe_job(images, config, divisors, colour, DCTN_DISTORTION_MIN_CANDIDATES, DCT8_DISTORTION_MIN_CANDIDATES)
    if job is None:
        return None
    stack, head, eight = job
    import jpegx
    entry = jpegx.batch_probe_distortion_pictures if eight else jpegx.batch_probe_distortion_pictures_n
    out = np.empty((len(stack), 3, len(divisors)), dtype=np.int64)
    for at in range(0, len(divisors), jpegx.PROBE_MAX_CANDIDATES):
        some = divisors[at:at + jpegx.PROBE_MAX_CANDIDATES]
        got = _none_on_refusal(entry, stack, *head, "divide", [float(d) for d in some], **_colour_kw(colour))
        if got is None:
            return None
        sse, bad = got
        part = np.asarray(sse).astype(np.int64)
        # Jpeg.compress raises for the whole picture when any band does
        part[np.broadcast_to(np.asarray(bad).any(axis=1, keepdims=True), part.shape)] = -1
        out[:, :, at:at + len(some)] = part
    return out


def probe_picture_distortion(images, config, divisors, colour=None):
    """int64 [len(images)][3][len(divisors)]: entry [i][b][j] is the sum over the picture's pixels of
    (band b of Jpeg(config_j).decompress(Jpeg(config_j).compress(x_i)) - band b of x_i) ** 2, where config_j is ``config`` with
    QuantizationMethod('divide', divisor=divisors[j]) and x_i is picture i as the codec is handed it -- with colour='rgb' that
    is images[i].convert('YCbCr'): the error is measured in the coded bands, where compress_rgb equals compress of the converted
    picture.  -1 (in all three bands) where compressing raises BadRleCodeError.  ``images`` as compress_pictures takes them.
    ValueError for a configuration that is not 'divide' and for a divisor that is not a whole positive number.
    With at least DCTN_DISTORTION_MIN_CANDIDATES divisors, dct_size other than 8 with transform 'DCT', the stock steps, a usable
    device, pictures that _stacked_pixels accepts and planes of at least DCTN_MIN_SAMPLES samples, all divisors are measured on
    the device in one pass per 32 of them (jpegx.batch_probe_distortion_pictures_n); everything else, and every refusal, is the
    loop.  dct_size 8 has the same road (_job_config_8, jpegx.batch_probe_distortion_pictures) behind a gate of its own,
    DCT8_DISTORTION_MIN_CANDIDATES, which ships as None: dct_size 8 is the loop until a caller sets it."""
    _check_colour(colour)
    divisors = _checked_divisors(config, divisors)
    if not isinstance(images, np.ndarray):
        images = list(images)
    sse = _distortion_device(images, config, divisors, colour) if len(divisors) else None
    return sse if sse is not None else _distortion_loop(images, config, divisors, colour)


def _psnr_of(sse, rows, cols):
    """float64 [pictures][K] from int64 sums [pictures][bands][K]: 10 log10(255^2 * bands * rows * cols / sum over the bands); inf at
    zero error, nan where an entry is -1."""
    sse = np.asarray(sse)
    total = sse.sum(axis=1).astype(np.float64)
    peak = 255.0 ** 2 * sse.shape[1] * rows * cols
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = np.where(total > 0, 10.0 * np.log10(peak / np.where(total > 0, total, 1.0)), np.inf)
    psnr[(sse < 0).any(axis=1)] = np.nan
    return psnr


def probe_picture_psnr(images, config, divisors, colour=None):
    """float64 [len(images)][len(divisors)]: the PSNR of every picture under every divisor over its three coded bands,
    10 * log10(255^2 * 3 * rows * cols / sum over the bands of probe_picture_distortion); inf where nothing is lost, nan where
    the picture cannot be coded (an entry of -1)."""
    return _psnr_of(probe_picture_distortion(images, config, divisors, colour), config.height, config.width)


def _meets(psnr, min_psnr):
    return not np.isnan(psnr) and psnr >= min_psnr


def compress_to_quality(image, config, min_psnr, colour=None, lo=1, hi=4096, probes=16, rounds=3):
    """(container, divisor, psnr): ``image`` compressed under ``config`` with the largest 'divide' divisor the search below finds
    whose PSNR (probe_picture_psnr) is at least ``min_psnr`` dB; the container is Jpeg(config_divisor).compress(image)
    (compress_rgb with colour='rgb').  compress_to_size's search mirrored; it is deterministic and costs 1 + ``rounds`` calls of
    probe_picture_psnr at most:
      1. candidates: ``probes`` whole numbers spaced geometrically from ``lo`` to ``hi`` inclusive;
      2. f = the LARGEST candidate whose PSNR is not nan (BadRleCodeError) and at least min_psnr -- none: TargetQualityError;
         g = the candidate just above f, or hi + 1;
      3. while rounds remain and whole numbers lie strictly between f and g: up to ``probes`` of them, evenly spaced, are
         probed; f becomes the largest of them that meets the floor (it stays if none does), g the probed number just above
         the new f (the old g if there is none);
      4. ONE compression, with f.
    PSNR need not fall monotonically with the divisor: f is the largest number MEETING the floor that the search has seen below
    a number that misses it, not a global maximum."""
    _check_colour(colour)
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (lo, hi, probes, rounds)) \
            or lo < 1 or hi < lo or probes < 1 or rounds < 0:
        raise ValueError("compress_to_quality: lo, hi, probes and rounds must be whole numbers with 1 <= lo <= hi, probes >= 1, rounds >= 0")
    if isinstance(min_psnr, bool) or not isinstance(min_psnr, (int, float, np.integer, np.floating)) or np.isnan(min_psnr):
        raise ValueError("compress_to_quality: min_psnr must be a number of decibels, got %r" % (min_psnr,))
    lo, hi, probes, rounds = int(lo), int(hi), int(probes), int(rounds)
    seen = {}                                            # divisor -> probed PSNR

    def probe(candidates):
        psnr = probe_picture_psnr([image], config, candidates, colour)[0]
        seen.update((d, float(p)) for d, p in zip(candidates, psnr))

    candidates = _geometric(lo, hi, probes)
    probe(candidates)
    meeting = [d for d in candidates if _meets(seen[d], min_psnr)]
    if not meeting:
        coded = [(p, -d) for d, p in seen.items() if not np.isnan(p)]
        if not coded:
            raise TargetQualityError("no divisor in %d..%d codes the picture at all (BadRleCodeError at every candidate)" % (lo, hi))
        best, at = max(coded)
        raise TargetQualityError("no divisor in %d..%d keeps the picture at %.2f dB or above: the best PSNR seen is %.2f dB, at divisor %d"
                                 % (lo, hi, min_psnr, best, -at))
    f = meeting[-1]
    g = min([d for d in candidates if d > f], default=hi + 1)
    for _ in range(rounds):
        inner = _between(f, g, probes)
        if not inner:
            break
        probe(inner)
        meeting = [d for d in inner if _meets(seen[d], min_psnr)]
        if meeting:
            f = meeting[-1]
        g = min([d for d in inner if d > f], default=g)
    return _compress_one(image, _divide_config(config, f), colour), f, seen[f]


def compress_pictures_to_quality(images, config, min_psnr, divisors, colour=None):
    """(containers, chosen): every picture compressed with the largest divisor of the ascending ladder ``divisors`` (at most 32
    rungs) that keeps its PSNR at ``min_psnr`` dB or above; chosen[i] is picture i's divisor and containers[i] equals
    Jpeg(config_chosen[i]).compress(images[i]) (compress_rgb with colour='rgb'), byte for byte, in input order.  ONE
    probe_picture_psnr call measures the whole batch on every rung; the pictures of a rung are then one compress_pictures call.
    TargetQualityError names the first picture that meets the floor on no rung."""
    _check_colour(colour)
    ladder = _checked_divisors(config, divisors)
    if not 1 <= len(ladder) <= 32 or any(b <= a for a, b in zip(ladder, ladder[1:])):
        raise ValueError("compress_pictures_to_quality: divisors must be 1..32 ascending rungs")
    if not isinstance(images, np.ndarray):
        images = list(images)
    psnr = probe_picture_psnr(images, config, ladder, colour)
    rung = []
    for i, row in enumerate(psnr):
        meeting = [j for j, p in enumerate(row) if _meets(p, min_psnr)]
        if not meeting:
            coded = [(float(p), -ladder[j]) for j, p in enumerate(row) if not np.isnan(p)]
            raise TargetQualityError("picture %d meets %.2f dB on no rung%s" % (
                i, min_psnr, ": its best PSNR is %.2f dB, at divisor %d" % (max(coded)[0], -max(coded)[1]) if coded
                else " (BadRleCodeError at every rung)"))
        rung.append(meeting[-1])
    containers = [None] * len(rung)
    for j in sorted(set(rung)):
        members = [i for i, r in enumerate(rung) if r == j]
        group = images[members] if isinstance(images, np.ndarray) else [images[i] for i in members]
        for i, c in zip(members, compress_pictures(group, _divide_config(config, ladder[j]), colour)):
            containers[i] = c
    return containers, [ladder[j] for j in rung]


# ---------------------------------------------------------------------------------------------------------------------
# the same for a SET of pictures of unequal sizes, each under the configuration at its own size (compress_picture_set)
# ---------------------------------------------------------------------------------------------------------------------
# probe_picture_set_sizes takes the device road (jpegx.batch_probe_picture_set_n: one flat upload, per group of pictures one
# gather into the block strip and one pass of the probe's kernel with the planes looked up in the set's table, one download)
# from DCTN_PROBE_MIN_CANDIDATES divisors and this many ADMITTED pictures on; None: the road is off and the function is the
# loop.  Read when the function is called.  Never below 1.
# Measured (profiles/probe_set_n.json and, a second run of the same code, _run2.json; pictures with sides between
# 64 and 128 at N 4 and N 16, 2 and 16 divisors, the set probe against the loop and against one probe_picture_sizes call per
# distinct size, alternating call by call on one MI355X; figures of the first run, the second agrees on every verdict here):
# the set probe beat the loop at every count (6-96x).  With ONE admitted picture it lost to probe_picture_sizes on that
# picture in all four comparisons of either run (0.18 against 0.14 ms with 2 divisors, 0.26 against 0.21-0.23 ms with 16:
# the table and its upload on top of the same work); with 2 pictures of 2 sizes it won all of them (0.20-0.21 against
# 0.26-0.27 ms, 0.34-0.35 against 0.41-0.43 ms), with 4 by 1.4-1.6x, with 16 by 1.8-2.4x, with 64 by 2.1-3.8x.  The smallest count with no
# loss at or above it; no plane size lost at every count, so there is no size gate.  A lone admitted picture is the loop here:
# callers with one picture have probe_picture_sizes.
DCTN_PROBE_SET_MIN_PICTURES = 2


def _probe_set_row(image, config, divisors, colour):
    """One row of the literal loop: len(Jpeg(config_ij).compress(image)) under the configuration at the picture's own size,
    -1 where it raises the reference's BadRleCodeError."""
    import util
    sized = _sized(config, image.height, image.width)
    row = np.empty(len(divisors), dtype=np.int64)
    for j, d in enumerate(divisors):
        try:
            row[j] = len(_compress_one(image, _divide_config(sized, d), colour))
        except util.BadRleCodeError:
            row[j] = -1
    return row


def _admitted_set(images, config, colour, least):
    """(admitted, pixels, job) of the pictures that go to the device as one set -- admitted: (index, rows, cols) per picture,
    pixels: their uint8 arrays, job: (block_size, dct_size, mode, param), the same for every picture -- or None where fewer
    than ``least`` pictures are admitted or the set is too large.  The vetting is _compress_picture_set's without its size
    ceiling; the size probe and the distortion probe over a set share it."""
    admitted, job = [], None                            # (index, rows, cols)
    for at, im in enumerate(images):
        try:
            rows, cols = im.height, im.width
        except Exception:
            continue
        if not isinstance(rows, (int, np.integer)) or not isinstance(cols, (int, np.integer)) or rows < 1 or cols < 1 or rows * cols > 2 ** 31 - 1:
            continue
        sized = _sized(config, rows, cols)
        if _picture_size(im, sized) is None or (colour is not None and im.mode != "RGB"):
            continue
        this = _compress_job_n(sized, rows, cols, 0)
        if this is None:
            continue
        job = this                                      # (block_size, dct_size, mode, param): the same for every picture
        admitted.append((at, rows, cols))
    if len(admitted) < max(least, 1):
        return None
    if 3 * sum(h * w for h, w in (_blocked_shape(rows, cols, job[0], job[1]) for _, rows, cols in admitted)) > 2 ** 31 - 1:
        return None
    pixels = [_picture_pixels(images[at]) for at, _, _ in admitted]      # the costly part of the vetting: last
    keep = [k for k, p in enumerate(pixels) if p is not None]
    if len(keep) != len(pixels):
        admitted, pixels = [admitted[k] for k in keep], [pixels[k] for k in keep]
        if len(admitted) < max(least, 1):
            return None
    return admitted, pixels, job


def _probe_set_device(images, config, divisors, colour):
    """{index: int64 row of sizes} of the pictures that were sized on the device as one set; empty where the gates, the
    configuration or libjpegx say no.  The vetting is _admitted_set's."""
    gate, least = DCTN_PROBE_MIN_CANDIDATES, DCTN_PROBE_SET_MIN_PICTURES
    if gate is None or least is None or len(divisors) < max(gate, 1) or len(images) < max(least, 1) \
            or not _stock_registry() or not _device_usable():
        return {}
    import jpegx
    vetted = _admitted_set(images, config, colour, least)
    if vetted is None:
        return {}
    admitted, pixels, job = vetted
    out = np.empty((len(admitted), len(divisors)), dtype=np.int64)
    heads = {}                                           # (rows, cols, divisor) -> the header's length
    for at in range(0, len(divisors), jpegx.PROBE_MAX_CANDIDATES):
        some = divisors[at:at + jpegx.PROBE_MAX_CANDIDATES]
        got = _none_on_refusal(jpegx.batch_probe_picture_set_n, pixels, job[0], job[1], "divide", [float(d) for d in some], **_colour_kw(colour))
        if got is None:
            return {}
        coded, bad = got
        # file_format.generate_data: the header of the picture's OWN configuration, then <L length + bytes per band
        for (_, rows, cols) in admitted:
            for d in some:
                if (rows, cols, d) not in heads:
                    heads[(rows, cols, d)] = len(file_format.create_header(_divide_config(_sized(config, rows, cols), d)))
        lengths = np.array([[heads[(rows, cols, d)] for d in some] for _, rows, cols in admitted], dtype=np.int64)
        part = coded.sum(axis=1).astype(np.int64) + lengths + 3 * 4
        part[bad.any(axis=1)] = -1
        out[:, at:at + len(some)] = part
    return {at: out[k] for k, (at, _, _) in enumerate(admitted)}


def probe_picture_set_sizes(images, config, divisors, colour=None):
    """int64 [len(images)][len(divisors)]: entry [i][j] is len(Jpeg(config_ij).compress(images[i])) -- with colour='rgb', of
    compress_rgb -- where config_ij is ``config`` with picture i's own width and height (``config``'s own are not read) and
    QuantizationMethod('divide', divisor=divisors[j]); -1 where that call raises BadRleCodeError.  The header of config_ij and
    the 12 bytes of length prefixes are counted.  ``images``: a sequence of PIL images, sizes as they come.  ValueError as
    probe_picture_sizes raises it.
    The pictures that compress_picture_set admits (_picture_size, _compress_job_n with the picture's own size, _picture_pixels;
    with colour='rgb' of mode RGB; no ceiling on the plane) are sized on the device as ONE set, 32 divisors to a pass
    (jpegx.batch_probe_picture_set_n), when there are at least DCTN_PROBE_SET_MIN_PICTURES of them and at least
    DCTN_PROBE_MIN_CANDIDATES divisors; every other picture, and all of them after a refusal, are the loop.  Rows come back
    in input order."""
    _check_colour(colour)
    divisors = _checked_divisors(config, divisors)
    images = list(images)
    done = _probe_set_device(images, config, divisors, colour) if images and divisors else {}
    out = np.empty((len(images), len(divisors)), dtype=np.int64)
    for at, im in enumerate(images):
        out[at] = done[at] if at in done else _probe_set_row(im, config, divisors, colour)
    return out


def compress_picture_set_to_size(images, config, max_bytes, divisors, colour=None):
    """compress_pictures_to_size for a set of pictures of unequal sizes: (containers, chosen), every picture compressed under
    the configuration at its own size with the smallest divisor of the ascending ladder ``divisors`` (at most 32 rungs) that
    brings its container within ``max_bytes`` bytes; containers[i] equals Jpeg(config_i with chosen[i]).compress(images[i])
    (compress_rgb with colour='rgb'), byte for byte.  ONE probe_picture_set_sizes call sizes the set on every rung; the
    pictures of a rung are then one compress_picture_set call.  TargetSizeError names the first picture that fits no rung;
    RuntimeError if a container's length is not the probed one."""
    _check_colour(colour)
    ladder = _checked_divisors(config, divisors)
    if not 1 <= len(ladder) <= 32 or any(b <= a for a, b in zip(ladder, ladder[1:])):
        raise ValueError("compress_picture_set_to_size: divisors must be 1..32 ascending rungs")
    images = list(images)
    sizes = probe_picture_set_sizes(images, config, ladder, colour)
    rung = []
    for i, row in enumerate(sizes):
        fitting = [j for j, s in enumerate(row) if _fits(int(s), max_bytes)]
        if not fitting:
            coded = [(int(s), ladder[j]) for j, s in enumerate(row) if s != -1]
            raise TargetSizeError("picture %d fits no rung within %d bytes%s" % (
                i, max_bytes, ": its smallest size is %d bytes, at divisor %d" % min(coded) if coded else " (BadRleCodeError at every rung)"))
        rung.append(fitting[0])
    containers = [None] * len(rung)
    for j in sorted(set(rung)):
        members = [i for i, r in enumerate(rung) if r == j]
        for i, c in zip(members, compress_picture_set([images[i] for i in members], _divide_config(config, ladder[j]), colour)):
            if len(c) != int(sizes[i][j]):
                raise RuntimeError("compress_picture_set_to_size: picture %d was probed at %d bytes under divisor %s, its container holds %d"
                                   % (i, int(sizes[i][j]), ladder[j], len(c)))
            containers[i] = c
    return containers, [ladder[j] for j in rung]


# ---------------------------------------------------------------------------------------------------------------------
# probe_picture_set_distortion takes the device road (jpegx.batch_probe_distortion_picture_set_n: one flat upload, per group
# of pictures the two gathers onto the block strip and one pass of the distortion kernel with a block's plane, place and band
# size looked up in the set's table, one download) from DCTN_DISTORTION_MIN_CANDIDATES divisors and this many ADMITTED pictures
# on; None: the road is off and the function is the loop.  Read when the function is called.  Never below 1.
# Measured (profiles/probe_distortion_set_n.json and, a second run of the same code, _run2.json; pictures with
# sides between 64 and 128 at N 4 and N 16, 1, 2 and 16 divisors, the set probe against the loop and against one
# probe_picture_distortion call per distinct size, alternating call by call on one MI355X; both runs agree on every verdict):
# the set probe beat the loop at every count (6-7x with one picture and one divisor, 480-550x with 64 and 16).  Against
# probe_picture_distortion per size: with ONE admitted picture it lost all six comparisons of either run (0.17-0.26 against
# 0.14-0.25 ms: the table and its upload on top of the same work); with 2 pictures of 2 sizes it won all of them (0.19-0.27
# against 0.24-0.41 ms); with 4 pictures of 3 sizes it LOST with 1 and 2 divisors in both runs (0.45-0.49 against 0.39-0.42 ms)
# and lay within 4 % either way with 16; with 16 pictures it won by 2.4-3.0x, with 64 by 4.5-5.5x.  The smallest measured count
# with no loss at or above it.  Between 2 and 15 admitted pictures callers who know their sizes repeat have
# probe_picture_distortion; the loop, which this gate falls back to there, is the slowest of the three.
DCTN_DISTORTION_SET_MIN_PICTURES = 16


def _distortion_set_row(image, config, divisors, colour):
    """One row of the literal loop: _distortion_loop of the one picture under the configuration at its own size."""
    return _distortion_loop([image], _sized(config, image.height, image.width), divisors, colour)[0]


def _distortion_set_device(images, config, divisors, colour):
    """{index: int64 [3][K] sums} of the pictures that were measured on the device as one set; empty where the gates, the
    configuration or libjpegx say no.  The vetting is _admitted_set's, as the size probe's over a set."""
    gate, least = DCTN_DISTORTION_MIN_CANDIDATES, DCTN_DISTORTION_SET_MIN_PICTURES
    if gate is None or least is None or len(divisors) < max(gate, 1) or len(images) < max(least, 1) \
            or not _stock_registry() or not _device_usable():
        return {}
    import jpegx
    vetted = _admitted_set(images, config, colour, least)
    if vetted is None:
        return {}
    admitted, pixels, job = vetted
    out = np.empty((len(admitted), 3, len(divisors)), dtype=np.int64)
    for at in range(0, len(divisors), jpegx.PROBE_MAX_CANDIDATES):
        some = divisors[at:at + jpegx.PROBE_MAX_CANDIDATES]
        got = _none_on_refusal(jpegx.batch_probe_distortion_picture_set_n, pixels, job[0], job[1], "divide", [float(d) for d in some],
                               **_colour_kw(colour))
        if got is None:
            return {}
        sse, bad = got
        part = np.asarray(sse).astype(np.int64)
        # Jpeg.compress raises for the whole picture when any band does
        part[np.broadcast_to(np.asarray(bad).any(axis=1, keepdims=True), part.shape)] = -1
        out[:, :, at:at + len(some)] = part
    return {at: out[k] for k, (at, _, _) in enumerate(admitted)}


def probe_picture_set_distortion(images, config, divisors, colour=None):
    """int64 [len(images)][3][len(divisors)]: entry [i][b][j] is what probe_picture_distortion gives for picture i alone under
    ``config`` with the picture's own width and height (``config``'s own are not read) and divisor divisors[j]: the sum over the
    picture's pixels of the squared differences in coded band b; -1 (in all three bands) where compressing raises
    BadRleCodeError.  ``images``: a sequence of PIL images, sizes as they come.  ValueError as probe_picture_distortion raises it.
    The pictures that compress_picture_set admits (probe_picture_set_sizes' vetting; planes of at least DCTN_MIN_SAMPLES samples)
    are measured on the device as ONE set, 32 divisors to a pass (jpegx.batch_probe_distortion_picture_set_n), when there are
    at least DCTN_DISTORTION_SET_MIN_PICTURES of them and at least DCTN_DISTORTION_MIN_CANDIDATES divisors; every other picture,
    and all of them after a refusal, are the loop.  Rows come back in input order."""
    _check_colour(colour)
    divisors = _checked_divisors(config, divisors)
    images = list(images)
    done = _distortion_set_device(images, config, divisors, colour) if images and divisors else {}
    out = np.empty((len(images), 3, len(divisors)), dtype=np.int64)
    for at, im in enumerate(images):
        out[at] = done[at] if at in done else _distortion_set_row(im, config, divisors, colour)
    return out


def probe_picture_set_psnr(images, config, divisors, colour=None):
    """float64 [len(images)][len(divisors)]: probe_picture_psnr for a set, every picture's PSNR over its three coded bands with
    its OWN rows * cols: inf where nothing is lost, nan where the picture cannot be coded."""
    images = list(images)
    sse = probe_picture_set_distortion(images, config, divisors, colour)
    out = np.empty((len(images), sse.shape[2]), dtype=np.float64)
    for at, im in enumerate(images):
        out[at] = _psnr_of(sse[at:at + 1], im.height, im.width)[0]
    return out


def compress_picture_set_to_quality(images, config, min_psnr, divisors, colour=None):
    """compress_pictures_to_quality for a set of pictures of unequal sizes: (containers, chosen), every picture compressed under
    the configuration at its own size with the largest divisor of the ascending ladder ``divisors`` (at most 32 rungs) that
    keeps its PSNR at ``min_psnr`` dB or above; containers[i] equals Jpeg(config_i with chosen[i]).compress(images[i])
    (compress_rgb with colour='rgb'), byte for byte, in input order.  ONE probe_picture_set_psnr call measures the set on every
    rung; the pictures of a rung are then one compress_picture_set call.  TargetQualityError names the first picture that meets
    the floor on no rung."""
    _check_colour(colour)
    ladder = _checked_divisors(config, divisors)
    if not 1 <= len(ladder) <= 32 or any(b <= a for a, b in zip(ladder, ladder[1:])):
        raise ValueError("compress_picture_set_to_quality: divisors must be 1..32 ascending rungs")
    images = list(images)
    psnr = probe_picture_set_psnr(images, config, ladder, colour)
    rung = []
    for i, row in enumerate(psnr):
        meeting = [j for j, p in enumerate(row) if _meets(p, min_psnr)]
        if not meeting:
            coded = [(float(p), -ladder[j]) for j, p in enumerate(row) if not np.isnan(p)]
            raise TargetQualityError("picture %d meets %.2f dB on no rung%s" % (
                i, min_psnr, ": its best PSNR is %.2f dB, at divisor %d" % (max(coded)[0], -max(coded)[1]) if coded
                else " (BadRleCodeError at every rung)"))
        rung.append(meeting[-1])
    containers = [None] * len(rung)
    for j in sorted(set(rung)):
        members = [i for i, r in enumerate(rung) if r == j]
        for i, c in zip(members, compress_picture_set([images[i] for i in members], _divide_config(config, ladder[j]), colour)):
            containers[i] = c
    return containers, [ladder[j] for j in rung]
