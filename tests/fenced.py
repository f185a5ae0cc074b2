"""Fenced device outputs for the tests that call a device entry directly: allocate, fill with 0xA5, call, download
the whole allocation and require every byte the entry has no business writing to hold 0xA5 still -- the slack between
the rows, the bytes in front of an offset base and the bytes behind the last row.  A plain helper module of the suite."""
import ctypes

import numpy as np

CANARY = 0xA5
GUARD = 256          # bytes kept in front of and behind every fenced span; a multiple of 16


class Fenced:
    """A device allocation of GUARD + offset + nbytes + GUARD bytes, all 0xA5; `ptr` is the address handed to the
    entry, GUARD + offset bytes into the allocation (the allocation itself is 256-byte aligned)."""

    def __init__(self, gpu, nbytes, offset=0):
        self.gpu, self.nbytes, self.front = gpu, int(nbytes), GUARD + int(offset)
        self.buf = gpu.DeviceBuffer(self.front + self.nbytes + GUARD)
        self.ptr = self.buf.ptr + self.front
        gpu.check(gpu.lib().jpegx_memset(self.buf.ptr, CANARY, self.buf.nbytes, None), "jpegx_memset")
        gpu.check(gpu.lib().jpegx_device_synchronize())

    def upload(self, array, offset=0):
        """Bytes of `array` to ptr + offset (what a test puts into a span the entry reads)."""
        a = np.ascontiguousarray(array)
        assert 0 <= offset and offset + a.nbytes <= self.nbytes
        self.buf.upload(a, offset=self.front + offset)

    def download(self, written=None, what=""):
        """The span's nbytes as uint8 after a device-wide synchronize.  `written`: bool mask over the span of the bytes
        the entry may have written; every other byte of the span and both guards must still hold the canary."""
        self.gpu.check(self.gpu.lib().jpegx_device_synchronize())
        raw = self.buf.download((self.buf.nbytes,), np.uint8)
        span = raw[self.front:self.front + self.nbytes]
        assert np.all(raw[:self.front] == CANARY), "%s: bytes in front of the base were written" % (what,)
        assert np.all(raw[self.front + self.nbytes:] == CANARY), "%s: bytes behind the last row were written" % (what,)
        if written is not None:
            bad = np.flatnonzero((span != CANARY) & ~written)
            assert bad.size == 0, "%s: %d bytes outside the output were written, the first at byte %d" % (what, bad.size, bad[0])
        return span

    def free(self):
        self.buf.free()


def rows_mask(nbytes, rows, pitch, row_bytes, start=0):
    """Bool mask over nbytes: True for `row_bytes` bytes of each of `rows` rows `pitch` bytes apart, from `start`."""
    m = np.zeros(nbytes, bool)
    for y in range(rows):
        m[start + y * pitch:start + y * pitch + row_bytes] = True
    return m


def rows_of(span, rows, pitch, row_bytes, dtype=np.uint8, start=0):
    """The rows of a downloaded span as a (rows, row_bytes / itemsize) array of dtype (a copy)."""
    assert start + rows * pitch <= span.size
    return np.ascontiguousarray(span[start:start + rows * pitch].reshape(rows, pitch)[:, :row_bytes]).view(dtype)


def pitched(array, pitch, fill=77):
    """`array` (rows, n) laid out with rows `pitch` elements apart, as one flat array of rows * pitch elements; the
    slack holds `fill`, a value unlike the data: an entry that reads it by mistake computes something else."""
    a = np.ascontiguousarray(array)
    rows, n = a.shape
    assert pitch >= n
    out = np.full(rows * pitch, fill, a.dtype)
    out.reshape(rows, pitch)[:, :n] = a
    return out


def device_inverse(gpu, zz, mode, param, out, flags=0, inflate=None, pitch_extra=0):
    """jpegx_inverse_fused (inflate None) or jpegx_inverse_fused_u8_inflated on device buffers, the output prefilled
    with 0xA5; the bytes between the rows, in front of the plane and behind it must still hold it.  pitch_extra:
    elements on top of the aligned row."""
    dtype = np.dtype({"f32": np.float32, "i16": np.int16, "u8": np.uint8}[out])
    esz, bs = dtype.itemsize, (inflate or 1)
    h, w = zz.shape[0] * 8, zz.shape[1] * 8
    pitch = (w * bs * esz + 15) // 16 * 16 // esz + pitch_extra
    dzz, dout = gpu.DeviceBuffer(zz.nbytes), Fenced(gpu, h * bs * pitch * esz)
    try:
        dzz.upload(np.ascontiguousarray(zz, np.int16))
        if inflate is None:
            gpu.inverse_fused_device(dzz.ptr, h, w, dout.ptr, mode, param, flags, out_type={"f32": gpu.OUT_F32, "i16": gpu.OUT_I16, "u8": gpu.OUT_U8}[out], out_pitch=pitch)
        else:
            gpu.check(gpu.lib().jpegx_inverse_fused_u8_inflated(dzz.ptr, h, w, gpu.mode_of(mode), float(param), flags, bs, dout.ptr, pitch, None),
                      "jpegx_inverse_fused_u8_inflated")
        res = dout.download(what="inverse").view(dtype).reshape(h * bs, pitch)
    finally:
        dzz.free()
        dout.free()
    assert np.all(res[:, w * bs:].view(np.uint8) == CANARY), "bytes between the rows were written"
    return res[:, :w * bs]


def plane_pointers(ptrs):
    """A host array of device pointers, the d_planes argument of the interleave entries."""
    return (ctypes.c_void_p * len(ptrs))(*ptrs)
