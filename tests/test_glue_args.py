"""The device glue entries of the 8x8 road (jpegx_deinterleave_u8, jpegx_interleave_u8, jpegx_mean_pool_f64): every bad
argument is refused with its documented code and a telling word in jpegx_last_error(), before a device is needed and
without a byte written.  The "device" pointers here are host spans filled with 0xA5 that must hold it afterwards.
CPU only; tests/test_gpu_glue_kernels.py runs what these entries accept."""
import ctypes

INVALID, UNSUPPORTED = -1, -4


class Spans:
    """Host memory standing in for device spans: a 256-byte aligned address, all 0xA5."""

    def __init__(self, nbytes=4096):
        self.buf = ctypes.create_string_buffer(b"\xA5" * (nbytes + 256), nbytes + 256)
        self.p = (ctypes.addressof(self.buf) + 255) & ~255

    def untouched(self):
        return self.buf.raw == b"\xA5" * len(self.buf.raw)


def _planes(*ptrs):
    return (ctypes.c_void_p * 4)(*ptrs)


def test_deinterleave_refuses_bad_arguments():
    import jpegx
    L = jpegx.lib()
    s = Spans()
    p = s.p
    good = _planes(p + 1024, p + 1536, p + 2048, p + 2560)
    err = lambda: L.jpegx_last_error()
    call = lambda **kw: L.jpegx_deinterleave_u8(*[kw.get(k, d) for k, d in (
        ("src", p), ("in_pitch", 30), ("nbands", 3), ("rows", 2), ("cols", 10), ("planes", good), ("pitch", 12), ("stream", None))])
    assert call(src=None) == INVALID and b"null" in err()
    assert call(planes=None) == INVALID and b"null" in err()
    assert call(nbands=0) == INVALID and b"planes" in err()
    assert call(nbands=5) == INVALID and b"planes" in err()
    assert call(rows=0) == INVALID and b"rows" in err()
    assert call(rows=65536) == INVALID and b"65535 rows" in err()
    assert call(cols=0) == INVALID and b"cols" in err()
    assert call(pitch=13) == INVALID and b"multiple of 4" in err()
    assert call(pitch=14) == INVALID and b"pitch" in err()
    assert call(pitch=8) == INVALID and b"rounded up to 4" in err()             # roundup4(10) is 12
    assert call(in_pitch=29) == INVALID and b"packed pitch" in err()
    assert call(nbands=4, in_pitch=39) == INVALID and b"packed pitch" in err()
    assert call(planes=_planes(p + 1024, None, p + 2048, None)) == INVALID and b"aligned" in err()
    for off in (1, 2, 3):
        assert call(planes=_planes(p + 1024, p + 1536, p + 2048 + off, None)) == INVALID and b"4-byte aligned" in err()
    assert call(nbands=1, in_pitch=10, planes=_planes(p + 1026, None, None, None)) == INVALID and b"aligned" in err()
    assert s.untouched()


def test_interleave_refuses_bad_arguments():
    import jpegx
    L = jpegx.lib()
    s = Spans()
    p = s.p
    good = _planes(p + 1024, p + 1536, p + 2048, p + 2560)
    err = lambda: L.jpegx_last_error()
    call = lambda **kw: L.jpegx_interleave_u8(*[kw.get(k, d) for k, d in (
        ("planes", good), ("nbands", 3), ("rows", 2), ("cols", 10), ("pitch", 12), ("out", p), ("out_pitch", 30), ("stream", None))])
    assert call(out=None) == INVALID and b"null" in err()
    assert call(planes=None) == INVALID and b"null" in err()
    assert call(nbands=0) == INVALID and b"planes" in err()
    assert call(nbands=5) == INVALID and b"planes" in err()
    assert call(rows=0) == INVALID and b"rows" in err()
    assert call(rows=65536) == INVALID and b"65535 rows" in err()
    assert call(cols=0) == INVALID and b"cols" in err()
    assert call(pitch=13) == INVALID and b"multiple of 4" in err()
    assert call(pitch=14) == INVALID and b"pitch" in err()
    assert call(pitch=8) == INVALID and b"rounded up to 4" in err()
    assert call(out_pitch=29) == INVALID and b"packed pitch" in err()
    assert call(nbands=2, out_pitch=19) == INVALID and b"packed pitch" in err()
    assert call(planes=_planes(p + 1024, None, p + 2048, None)) == INVALID and b"aligned" in err()
    for off in (1, 2, 3):
        assert call(planes=_planes(p + 1024 + off, p + 1536, p + 2048, None)) == INVALID and b"4-byte aligned" in err()
    assert s.untouched()


def test_mean_pool_refuses_bad_arguments():
    import jpegx
    L = jpegx.lib()
    s = Spans()
    p = s.p
    err = lambda: L.jpegx_last_error()
    call = lambda **kw: L.jpegx_mean_pool_f64(*[kw.get(k, d) for k, d in (
        ("src", p), ("elem", 1), ("H", 2), ("W", 5), ("pitch", 15), ("bs", 3), ("out", p + 2048), ("out_pitch", 5), ("stream", None))])
    assert call(src=None) == INVALID and b"null" in err()
    assert call(out=None) == INVALID and b"null" in err()
    assert call(bs=0) == INVALID and b"block_size" in err()
    assert call(bs=4097, pitch=5 * 4097) == INVALID and b"block_size" in err()
    assert call(bs=-3) == INVALID and b"block_size" in err()
    assert call(H=0) == INVALID and b"shape" in err()
    assert call(W=0) == INVALID and b"shape" in err()
    assert call(pitch=14) == INVALID and b"pitch" in err()
    assert call(out_pitch=4) == INVALID and b"pitch" in err()
    assert call(H=65536) == UNSUPPORTED and b"65535" in err()
    assert call(elem=2) == UNSUPPORTED and b"elem_size" in err()
    assert call(elem=8) == UNSUPPORTED and b"elem_size" in err()
    assert L.jpegx_mean_pool_f64_on(0, None, 1, 2, 5, 15, 3, p + 2048, 5, None) != 0
    assert s.untouched()
