"""GPU: jpegx_inflate_crop_u8 (csrc/jpegx_band_n.hip) -- DCTPadding.invert, SubSampling.invert and Padding.invert as one
scatter -- against np.repeat(np.repeat(plane[:P0, :P1], bs, 0), bs, 1)[:rows, :cols], exactly.  Planes are random bytes at
a pitch wider than the pooled row, with random poison in every column and row that the statement never reads (a kernel
that reads one shows it in the result).  Each case runs with a tight output pitch, with five bytes of slack per row behind
a sentinel fill and a guard span, from an output base 1 and 8 bytes behind a 16-byte boundary (the byte-wise path, and the
aligned path inside one row), and through the explicit-device twin."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (rows, cols, bs): one sample; a whole source byte wider than a chunk; one row, one column; around one 16-byte chunk at
# bs 1; around two chunks at bs 2; whole tiles; ragged both ways; a tile as wide as a chunk and one byte wider; the largest bs
CASES = [(1, 1, 1), (1, 1, 255), (1, 50, 3), (45, 1, 7), (5, 15, 1), (5, 16, 1), (5, 17, 1), (33, 31, 2), (33, 32, 2), (64, 96, 4),
         (53, 77, 5), (100, 136, 3), (37, 300, 16), (40, 529, 17), (3, 600, 255), (300, 2, 255)]
SENTINEL, GUARD = 0xC3, 256


@functools.lru_cache(maxsize=None)
def _case(rows, cols, bs):
    """(the plane with its poison, P0, P1, the expected band): built once, shared, read-only."""
    rng = np.random.default_rng(rows * 1000003 + cols * 1009 + bs)
    p0, p1 = -(-rows // bs), -(-cols // bs)
    plane = rng.integers(0, 256, (p0 + 3, p1 + 7)).astype(np.uint8)      # rows and columns beyond P0 x P1: poison
    want = np.repeat(np.repeat(plane[:p0, :p1], bs, 0), bs, 1)[:rows, :cols].copy()
    plane.setflags(write=False)
    want.setflags(write=False)
    return plane, p0, p1, want


def _run(gpu, rows, cols, bs, out_pitch, offset=0, device=None):
    """The entry on device buffers of the test's own.  Returns (band, slack, front guard, back guard)."""
    plane, p0, p1, _ = _case(rows, cols, bs)
    L = gpu.lib()
    span = rows * out_pitch
    size = GUARD + offset + span + GUARD
    din, dout = gpu.DeviceBuffer(plane.nbytes), gpu.DeviceBuffer(size)
    try:
        assert dout.ptr % 16 == 0
        din.upload(plane)
        dout.upload(np.full(size, SENTINEL, np.uint8))
        at = GUARD + offset
        if device is None:
            gpu.check(L.jpegx_inflate_crop_u8(din.ptr, plane.shape[1], rows, cols, bs, dout.ptr + at, out_pitch, None), "jpegx_inflate_crop_u8")
        else:
            gpu.check(L.jpegx_inflate_crop_u8_on(device, din.ptr, plane.shape[1], rows, cols, bs, dout.ptr + at, out_pitch, None),
                      "jpegx_inflate_crop_u8_on")
        buf = dout.download((size,), np.uint8)
        body = buf[at:at + span].reshape(rows, out_pitch)
        return body[:, :cols], body[:, cols:], buf[:at], buf[at + span:]
    finally:
        din.free()
        dout.free()


def _check(got, want, what):
    band, slack, front, back = got
    assert np.array_equal(band, want), what
    assert np.all(slack == SENTINEL), "%s: the pitch slack was written" % (what,)
    assert np.all(front == SENTINEL) and np.all(back == SENTINEL), "%s: bytes outside the band were written" % (what,)


@pytest.mark.parametrize("rows,cols,bs", CASES)
def test_tight_pitch(gpu, rows, cols, bs):
    _check(_run(gpu, rows, cols, bs, cols), _case(rows, cols, bs)[3], "tight")


@pytest.mark.parametrize("rows,cols,bs", CASES)
def test_slack_and_guard_come_back_unchanged(gpu, rows, cols, bs):
    _check(_run(gpu, rows, cols, bs, cols + 5), _case(rows, cols, bs)[3], "pitch cols + 5")


@pytest.mark.parametrize("rows,cols,bs", CASES)
def test_output_base_off_the_16_byte_boundary(gpu, rows, cols, bs):
    want = _case(rows, cols, bs)[3]
    for offset in (1, 8):
        for pitch in (cols, cols + 5, (cols + 15) // 16 * 16):
            _check(_run(gpu, rows, cols, bs, pitch, offset), want, "offset %d pitch %d" % (offset, pitch))


@pytest.mark.parametrize("rows,cols,bs", CASES)
def test_explicit_device_twin(gpu, rows, cols, bs):
    _check(_run(gpu, rows, cols, bs, cols + 5, 0, device=0), _case(rows, cols, bs)[3], "_on")


def test_python_wrapper(gpu):
    for rows, cols, bs in ((53, 77, 5), (5, 17, 1), (3, 600, 255)):
        plane, _, _, want = _case(rows, cols, bs)
        got = gpu.inflate_crop_u8(plane, bs, rows, cols)
        assert got.dtype == np.uint8 and got.shape == (rows, cols) and np.array_equal(got, want)
        assert np.array_equal(gpu.inflate_crop_u8(plane[:, ::1][:-1, :-2], bs, rows, cols), want)      # another pitch, still large enough
