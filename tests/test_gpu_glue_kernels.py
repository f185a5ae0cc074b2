"""GPU: the small device entries that join the 8x8 road's kernels together, called directly on device pointers with
every kind of argument include/jpegx.h lets them take -- not only the one combination the host jobs pass.
jpegx_deinterleave_u8 / jpegx_interleave_u8 (1..4 bands, ragged widths, loose and odd packed pitches, packed bases at
odd addresses), jpegx_mean_pool_f64 (both element types, block sizes 1..1024, loose pitches), the stand-alone stage
entries with input and output rows further apart than they are long and by different amounts, and the run-time
replication of jpegx_inverse_fused_u8_inflated.  Every comparison is exact against a few lines of numpy or the CPU oracle
(the fp32 DCT pair keeps the criterion of tests/test_gpu_parity.py), and every output is fenced (tests/fenced.py)."""
import ctypes
import functools

import numpy as np
import pytest

import adversarial_zz as az
import oracle
from conftest import MODES
from fenced import Fenced, device_inverse, pitched, plane_pointers, rows_mask, rows_of

pytestmark = pytest.mark.gpu


def ru4(n):
    return (n + 3) & ~3


class created_stream:
    def __init__(self, gpu):
        self.gpu, self.handle = gpu, ctypes.c_void_p()

    def __enter__(self):
        self.gpu.check(self.gpu.lib().jpegx_stream_create(ctypes.byref(self.handle)), "jpegx_stream_create")
        return self.handle

    def __exit__(self, *exc):
        self.gpu.check(self.gpu.lib().jpegx_stream_synchronize(self.handle))
        self.gpu.check(self.gpu.lib().jpegx_stream_destroy(self.handle))


# ---- interleave / deinterleave --------------------------------------------------------------------------------------
# one pixel; fewer than four; one quad; a quad and a tail; around the 1024 columns one block of 256 threads takes; several
# blocks with a tail
PIXEL_SHAPES = [(1, 1), (2, 3), (3, 4), (2, 5), (3, 7), (1, 1023), (2, 1024), (2, 1025), (1, 1029), (5, 2052)]
BASE_OFFSETS = (0, 1, 2)


def packed_pitches(cols, nb):
    """Tight; the next multiple of 4 strictly above it (3 bands: whole dwords and the tail's bytes in one row); odd."""
    tight = cols * nb
    return (tight, (tight // 4 + 1) * 4, tight + 1)


def plane_pitches(cols):
    return (ru4(cols), ru4(cols) + 12)


def pixel_cases(nb):
    for rows, cols in PIXEL_SHAPES:
        for packed in packed_pitches(cols, nb):
            for base in BASE_OFFSETS:
                for pitch in plane_pitches(cols):
                    yield rows, cols, packed, base, pitch


def pixels_of(rows, cols, nb):
    """Random bytes, different in every band."""
    return np.random.default_rng(rows * 10007 + cols * 13 + nb).integers(0, 256, (rows, cols, nb), dtype=np.uint8)


def plane_layout(nb, rows, pitch):
    """Byte offsets of nb planes inside one allocation: 4-byte but not 16-byte aligned, a gap of canaries between two."""
    offs, off = [], 4
    for _ in range(nb):
        while off % 16 == 0:
            off += 4
        offs.append(off)
        off += rows * pitch + 4
    return offs, off


def interleave_from(gpu, ptrs, nb, rows, cols, pitch, out_pitch, base, stream=None, what=""):
    """jpegx_interleave_u8 of device planes into a fenced packed span `base` bytes off alignment: exactly cols * nb
    bytes of every row may be written.  Returns them as (rows, cols, nb)."""
    out = Fenced(gpu, rows * out_pitch, offset=base)
    try:
        gpu.check(gpu.lib().jpegx_interleave_u8(plane_pointers(ptrs), nb, rows, cols, pitch, out.ptr, out_pitch, stream), "jpegx_interleave_u8")
        span = out.download(rows_mask(out.nbytes, rows, out_pitch, cols * nb), what)
        return rows_of(span, rows, out_pitch, cols * nb).reshape(rows, cols, nb)
    finally:
        out.free()


def check_deinterleave(gpu, nb, rows, cols, packed, base, pitch, stream=None):
    what = ("deinterleave", nb, rows, cols, packed, base, pitch)
    x = pixels_of(rows, cols, nb)
    src = Fenced(gpu, rows * packed, offset=base)
    offs, total = plane_layout(nb, rows, pitch)
    dst = Fenced(gpu, total)
    try:
        src.upload(pitched(x.reshape(rows, cols * nb), packed))
        ptrs = [dst.ptr + o for o in offs]
        assert all(p % 4 == 0 and p % 16 != 0 for p in ptrs) and src.ptr % 4 == base
        gpu.check(gpu.lib().jpegx_deinterleave_u8(src.ptr, packed, nb, rows, cols, plane_pointers(ptrs), pitch, stream), "jpegx_deinterleave_u8")
        # a plane row may be written up to cols rounded up to 4 (include/jpegx.h); what lies behind cols is not asserted
        written = np.zeros(total, bool)
        for o in offs:
            written |= rows_mask(total, rows, pitch, ru4(cols), o)
        span = dst.download(written, what)
        for k, o in enumerate(offs):
            assert np.array_equal(rows_of(span, rows, pitch, cols, start=o), x[..., k]), (what, "band %d" % k)
        # and back: the planes as they lie on the device, through the other entry, into a span of the same kind
        back = interleave_from(gpu, ptrs, nb, rows, cols, pitch, packed, base, stream, what + ("and back",))
        assert np.array_equal(back, x), (what, "and back")
    finally:
        src.free()
        dst.free()


def check_interleave(gpu, nb, rows, cols, packed, base, pitch, stream=None):
    what = ("interleave", nb, rows, cols, packed, base, pitch)
    rng = np.random.default_rng(rows * 7919 + cols * 17 + nb)
    offs, total = plane_layout(nb, rows, pitch)
    host = rng.integers(0, 256, total, dtype=np.uint8)            # the slack of the planes holds random bytes too
    bands = [rows_of(host, rows, pitch, cols, start=o) for o in offs]
    src = Fenced(gpu, total)
    try:
        src.upload(host)
        got = interleave_from(gpu, [src.ptr + o for o in offs], nb, rows, cols, pitch, packed, base, stream, what)
        assert np.array_equal(got, np.dstack(bands)), what
    finally:
        src.free()


@pytest.mark.parametrize("nbands", [1, 2, 3, 4])
def test_deinterleave_every_width_pitch_and_base(gpu, nbands):
    for case in pixel_cases(nbands):
        check_deinterleave(gpu, nbands, *case)


@pytest.mark.parametrize("nbands", [1, 2, 3, 4])
def test_interleave_every_width_pitch_and_base(gpu, nbands):
    for case in pixel_cases(nbands):
        check_interleave(gpu, nbands, *case)


def test_pixel_entries_on_a_created_stream(gpu):
    with created_stream(gpu) as stream:
        check_deinterleave(gpu, 3, 2, 1025, 3076, 0, 1028 + 12, stream)
        check_interleave(gpu, 3, 2, 1025, 3076, 0, 1028 + 12, stream)
        check_interleave(gpu, 4, 3, 7, 29, 1, 8, stream)


# ---- jpegx_mean_pool_f64 --------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1), (3, 255), (2, 256), (2, 257), (5, 600)]       # W on either side of the 256-thread row split
POOL_CONTENTS = ["random", "all255", "zeros", "ones"]


def pool_band(content, H, W, bs, seed):
    if content == "random":
        return np.random.default_rng(seed).integers(0, 256, (H * bs, W * bs), dtype=np.uint8)
    if content == "all255":                                          # the largest sum a tile can have
        return np.full((H * bs, W * bs), 255, np.uint8)
    band = np.zeros((H * bs, W * bs), np.uint8)
    if content == "ones":                                            # every tile sums to 1: no multiple of bs * bs
        band[::bs, ::bs] = 1
    return band


def check_mean_pool(gpu, band, bs, elem_size, in_extra, out_extra):
    H, W = band.shape[0] // bs, band.shape[1] // bs
    what = ("mean_pool", elem_size, bs, H, W, in_extra, out_extra)
    want = band.reshape(H, bs, W, bs).astype(np.int64).sum((1, 3)) / float(bs * bs)
    pitch, opitch = W * bs + in_extra, W + out_extra
    samples = band if elem_size == 1 else band.astype(np.float32)
    src, out = Fenced(gpu, H * bs * pitch * elem_size), Fenced(gpu, H * opitch * 8)
    try:
        src.upload(pitched(samples, pitch))
        gpu.check(gpu.lib().jpegx_mean_pool_f64(src.ptr, elem_size, H, W, pitch, bs, out.ptr, opitch, None), "jpegx_mean_pool_f64")
        span = out.download(rows_mask(out.nbytes, H, opitch * 8, W * 8), what)
        got = rows_of(span, H, opitch * 8, W * 8, np.float64)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), what
    finally:
        src.free()
        out.free()


@pytest.mark.parametrize("elem_size", [1, 4])
@pytest.mark.parametrize("bs", [1, 2, 3, 5, 7, 16, 255])
def test_mean_pool_every_block_size_and_pitch(gpu, bs, elem_size):
    shapes = POOL_SHAPES if bs < 255 else [(1, 1), (2, 3)]
    for H, W in shapes:
        for content in POOL_CONTENTS:
            band = pool_band(content, H, W, bs, H * 1000 + W + bs)
            if content == "ones" and bs > 1:
                assert np.all(band.reshape(H, bs, W, bs).sum((1, 3), dtype=np.int64) % (bs * bs) != 0)
            for in_extra in (0, 13):
                for out_extra in (0, 3):
                    check_mean_pool(gpu, band, bs, elem_size, in_extra, out_extra)


@pytest.mark.parametrize("elem_size", [1, 4])
def test_mean_pool_block_size_1024(gpu, elem_size):
    for content in ("random", "all255"):
        check_mean_pool(gpu, pool_band(content, 1, 2, 1024, 5), 1024, elem_size, 13, 3)


def test_mean_pool_last_legal_row_of_the_grid(gpu):
    check_mean_pool(gpu, pool_band("random", 65535, 1, 1, 6), 1, 1, 13, 3)


# ---- the stand-alone stage entries, rows further apart than they are long ---------------------------------------------
# 1 block; 6 blocks in two block rows; 65 blocks: a partial group of the 8-blocks-per-wave float64 kernels and a partial
# wave of the lane-per-block fp32 ones
STAGE_SHAPES = [(8, 8), (16, 24), (8, 520)]
IN_EXTRA, OUT_EXTRA = 8, 16          # different on purpose: taking one pitch for the other shows


def run_stage(gpu, a, call, in_pitch, out_shape, out_pitch, out_dtype=None, what=""):
    """`a` (rows, n) to the device with rows in_pitch elements apart, call(d_in, d_out), and the fenced output
    (out_shape, rows out_pitch elements apart) back."""
    a = np.ascontiguousarray(a)
    out_dtype = np.dtype(out_dtype or a.dtype)
    rows, n = out_shape
    src, out = Fenced(gpu, a.shape[0] * in_pitch * a.itemsize), Fenced(gpu, rows * out_pitch * out_dtype.itemsize)
    try:
        src.upload(pitched(a, in_pitch))
        gpu.check(call(src.ptr, out.ptr), str(what))
        esz = out_dtype.itemsize
        span = out.download(rows_mask(out.nbytes, rows, out_pitch * esz, n * esz), what)
        return rows_of(span, rows, out_pitch * esz, n * esz, out_dtype)
    finally:
        src.free()
        out.free()


def plane_stage(gpu, a, fn, *mid, tail=(), what=""):
    """An entry of the form fn(d_in, H, W, pitch, *mid, d_out, out_pitch, *tail, stream) on a pitched plane."""
    H, W = a.shape
    call = lambda di, do: fn(di, H, W, W + IN_EXTRA, *mid, do, W + OUT_EXTRA, *tail, None)
    return run_stage(gpu, a, call, W + IN_EXTRA, (H, W), W + OUT_EXTRA, what=what)


def samples_of(shape, seed=0):
    return np.random.default_rng(100 + seed).integers(-128, 128, shape).astype(np.float64)


@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_dct_f64_entries_with_two_pitches(gpu, shape):
    L = gpu.lib()
    a = samples_of(shape)
    c = oracle.dct_plane(a)
    assert np.array_equal(plane_stage(gpu, a, L.jpegx_dct8x8_f64, what=("dct_f64", shape)), c)
    q = oracle.quant_plane(c, "divide", 3.0)                       # coefficients that do not bring the samples back
    assert np.array_equal(plane_stage(gpu, q, L.jpegx_idct8x8_f64, tail=(1,), what=("idct_f64 rounded", shape)), oracle.idct_plane(q))
    assert np.array_equal(plane_stage(gpu, q, L.jpegx_idct8x8_f64, tail=(0,), what=("idct_f64", shape)), oracle.idct_plane(q, rounded=False))


@pytest.mark.parametrize("suffix,mode,param", MODES)
def test_quantize_and_restore_entries_with_two_pitches(gpu, suffix, mode, param):
    L = gpu.lib()
    for shape in STAGE_SHAPES:
        c = oracle.dct_plane(samples_of(shape, 1))
        q = oracle.quant_plane(c, mode, param)
        got = plane_stage(gpu, c, L.jpegx_quantize_f64, gpu.mode_of(mode), float(param), what=("quantize", mode, shape))
        assert np.array_equal(got, q), (mode, shape)
        got = plane_stage(gpu, q, L.jpegx_restore_f64, gpu.mode_of(mode), float(param), what=("restore", mode, shape))
        assert np.array_equal(got, oracle.restore_plane(q, mode, param)), (mode, shape)
    # the table index follows the position in the block, not in the row: the columns of a qtable plane differ
    assert len(np.unique(oracle.quant_plane(np.full((8, 8), 1000.0), "qtable"))) > 8


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64, np.complex128])
def test_zigzag_entries_with_a_pitch(gpu, dtype):
    L = gpu.lib()
    esz = np.dtype(dtype).itemsize
    rng = np.random.default_rng(esz)
    for H, W in STAGE_SHAPES:
        a = rng.integers(-1000, 1000, (H, W)).astype(dtype)
        if dtype == np.complex128:
            a = a + 1j * rng.integers(-1000, 1000, (H, W))
            want = oracle.zigzag_plane(a.real) + 1j * oracle.zigzag_plane(a.imag)
        else:
            want = oracle.zigzag_plane(a).astype(dtype)
        n = H * W
        z = run_stage(gpu, a, lambda di, do: L.jpegx_zigzag(di, H, W, W + IN_EXTRA, esz, do, None), W + IN_EXTRA, (1, n), n,
                      what=("zigzag", esz, H, W))
        assert np.array_equal(z.reshape(H // 8, W // 8, 64), want), (esz, H, W)
        back = run_stage(gpu, z, lambda di, do: L.jpegx_unzigzag(di, H, W, esz, do, W + OUT_EXTRA, None), n, (H, W), W + OUT_EXTRA,
                         what=("unzigzag", esz, H, W))
        assert np.array_equal(back, a), (esz, H, W)
        if dtype != np.complex128:
            assert np.array_equal(back, oracle.unzigzag_plane(want).astype(dtype))


@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_dct_f32_entries_with_two_pitches(gpu, shape):
    """The criterion of test_dct_f32_within_1e4_of_reference (tests/test_gpu_parity.py), with its numbers."""
    L = gpu.lib()
    h, w = shape
    pre = samples_of(shape, 2)
    ref = oracle.dct_plane(pre)
    got32 = plane_stage(gpu, pre.astype(np.float32), L.jpegx_dct8x8_f32, what=("dct_f32", shape))
    got = got32.astype(np.float64)
    blockmax = np.abs(ref).reshape(h // 8, 8, w // 8, 8).max(axis=(1, 3))
    tol = 1e-4 * np.maximum(1.0, blockmax)
    err = np.abs(got - ref).reshape(h // 8, 8, w // 8, 8).max(axis=(1, 3))
    assert np.all(err <= tol), float((err / tol).max())
    back = plane_stage(gpu, got32, L.jpegx_idct8x8_f32, what=("idct_f32", shape))
    assert np.allclose(back, pre, atol=2e-3)


# ---- run-time replication of jpegx_inverse_fused_u8_inflated ----------------------------------------------------------
REPL_SHAPES = [(1, 1), (1, 65), (2, 3)]


REPL_MODE, REPL_PARAM = "divide", 0.125      # full_range amplitudes of +-16383 come back as samples within some +-1000


@functools.lru_cache(maxsize=None)
def clamping_stream(shape):
    """full_range blocks restored to samples of a spread of a few hundred: about half below 0, a quarter above 255 and
    the rest spread over 0..255, so that a sample taken from the wrong place shows.  Shared; left unchanged."""
    zz = az.plane(az.make("full_range", shape[0] * shape[1]), shape[0])
    raw = oracle.inverse_i16(zz, REPL_MODE, REPL_PARAM)
    assert (raw < 0).any() and (raw > 255).any() and np.unique(np.clip(raw, 0, 255)).size > 16
    return zz, np.clip(raw, 0, 255)


def check_replication(gpu, shape, bs, flags=0):
    zz, u8 = clamping_stream(shape)
    want = np.repeat(np.repeat(u8, bs, 0), bs, 1)
    for pitch_extra in (0, 8):
        got = device_inverse(gpu, zz, REPL_MODE, REPL_PARAM, "u8", flags, inflate=bs, pitch_extra=pitch_extra)
        assert got.shape == want.shape
        bad = np.flatnonzero((got != want).ravel())
        assert bad.size == 0, "x%d %s pitch +%d flags %#x: %d samples differ, the first at %s" % (
            bs, shape, pitch_extra, flags, bad.size, np.unravel_index(bad[0], got.shape))


@pytest.mark.parametrize("bs", [6, 7, 9, 12, 17, 31, 64])
def test_run_time_replication_factors(gpu, bs):
    for shape in REPL_SHAPES:
        check_replication(gpu, shape, bs)
        if bs == 9:
            for flags in (gpu.F_TUNE_NO_NT, gpu.F_TUNE_XCD_CONTIG):
                check_replication(gpu, shape, bs, flags)


def test_run_time_replication_factor_255(gpu):
    check_replication(gpu, (1, 2), 255)
