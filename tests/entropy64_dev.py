"""The 8x8 entropy stage's device entries on device pointers, for tests/test_gpu_entropy_adversarial.py: the public road
(jpegx_entropy_sizes / _emit), the production road's internal entries (sizes with half_info, the scan on its own, the
two-lanes-per-block emitter and its guarded twin) and the forward kernels that size their own blocks.  The internal
entries are not part of include/jpegx.h; their ctypes signatures are set here.  Every device output -- workspace,
coefficient stream, coded bytes -- lives in a fenced allocation (tests/fenced.py)."""
import ctypes

import numpy as np

import fenced

_vp, _ll, _int, _uint, _dbl, _sz, _pd = (ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_uint, ctypes.c_double,
                                         ctypes.c_size_t, ctypes.c_ssize_t)
INTERNAL = {
    "jpegx_internal_entropy_views": ([_vp, _ll] + [ctypes.POINTER(_vp)] * 3, None),
    "jpegx_internal_entropy_sizes_half": ([_vp, _ll, _vp, _vp], _int),
    "jpegx_internal_entropy_scan": ([_ll, _vp, _vp], _int),
    "jpegx_internal_entropy_emit2": ([_vp, _ll, _vp, _vp, _vp], _int),
    "jpegx_internal_entropy_emit2_guarded": ([_vp, _ll, _vp, _vp, _sz, _vp], _int),
    "jpegx_internal_forward_u8_sized": ([_vp, _int, _int, _pd, _int, _int, _dbl, _uint, _vp, _vp, _vp, _vp, _vp], _int),
    "jpegx_internal_forward_f32_sized": ([_vp, _int, _int, _pd, _int, _dbl, _uint, _vp, _vp, _vp, _vp, ctypes.POINTER(_int), _vp], _int),
}


def hooks(gpu):
    L = gpu.lib()
    for name, (argtypes, restype) in INTERNAL.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, restype
    return L


class Workspace:
    """A fenced entropy workspace for streams of up to `nblocks` blocks.  Nothing here clears it between uses (refill()
    puts the canary back where a test wants no earlier result to stand in for a missing write)."""

    def __init__(self, gpu, nblocks):
        self.gpu, self.L = gpu, hooks(gpu)
        self.cap = int(nblocks)
        self.mem = fenced.Fenced(gpu, self.L.jpegx_entropy_workspace_bytes(self.cap))
        self.ptr = self.mem.ptr

    def refill(self):
        self.gpu.check(self.L.jpegx_memset(self.mem.buf.ptr, fenced.CANARY, self.mem.buf.nbytes, None), "jpegx_memset")
        self.gpu.check(self.L.jpegx_device_synchronize())

    def views(self, nblocks):
        assert nblocks <= self.cap
        bb, wb, hb = _vp(), _vp(), _vp()
        self.L.jpegx_internal_entropy_views(self.ptr, nblocks, ctypes.byref(bb), ctypes.byref(wb), ctypes.byref(hb))
        for p in (bb, wb, hb):
            assert self.ptr <= p.value and p.value + 4 * nblocks <= self.ptr + self.mem.nbytes
        return bb.value, wb.value, hb.value

    def sizes(self, dzz, nblocks):
        """The public road: sizes and scans in one entry."""
        self.gpu.check(self.L.jpegx_entropy_sizes(dzz, nblocks, self.ptr, None), "jpegx_entropy_sizes")

    def sizes_half(self, dzz, nblocks):
        self.gpu.check(self.L.jpegx_internal_entropy_sizes_half(dzz, nblocks, self.ptr, None), "entropy_sizes_half")

    def scan(self, nblocks):
        self.gpu.check(self.L.jpegx_internal_entropy_scan(nblocks, self.ptr, None), "entropy_scan")

    def total_rc(self):
        total = ctypes.c_ulonglong(0)
        rc = self.L.jpegx_entropy_total(self.ptr, ctypes.byref(total), None)
        return rc, int(total.value)

    def block_sizes(self, nblocks):
        out = np.empty(nblocks, np.uint32)
        self.gpu.check(self.L.jpegx_entropy_block_sizes(self.ptr, nblocks, out.ctypes.data, None), "jpegx_entropy_block_sizes")
        return out

    def half_info(self, nblocks):
        self.gpu.check(self.L.jpegx_device_synchronize())
        hb = self.views(nblocks)[2]
        return self.mem.buf.download((nblocks,), np.uint32, offset=hb - self.mem.buf.ptr)

    def check_fences(self, what="workspace"):
        self.mem.download(what=what)

    def free(self):
        self.mem.free()


class Stream:
    """An int16 (nblocks, 64) stream on the device."""

    def __init__(self, gpu, zz):
        z = np.ascontiguousarray(zz, dtype=np.int16)
        self.nblocks = z.size // 64
        self.buf = gpu.DeviceBuffer(z.nbytes)
        self.buf.upload(z)
        self.ptr = self.buf.ptr

    def free(self):
        self.buf.free()


def emit(gpu, entry, dzz, nblocks, ws, nbytes, offset=0, cap=None):
    """One emit into a fenced span of nbytes that starts `offset` bytes behind a 16-byte boundary: entry "emit" (one lane
    per block), "emit2" (two lanes) or "guarded" (emit2 with the capacity `cap`).  Returns the span's bytes; the fences
    are checked on the way."""
    L = hooks(gpu)
    out = fenced.Fenced(gpu, nbytes, offset)
    try:
        assert out.ptr % 16 == offset % 16
        if entry == "emit":
            rc = L.jpegx_entropy_emit(dzz, nblocks, ws.ptr, out.ptr, None)
        elif entry == "emit2":
            rc = L.jpegx_internal_entropy_emit2(dzz, nblocks, ws.ptr, out.ptr, None)
        else:
            rc = L.jpegx_internal_entropy_emit2_guarded(dzz, nblocks, ws.ptr, out.ptr, cap, None)
        gpu.check(rc, entry)
        return out.download(what="%s at offset %d" % (entry, offset)).tobytes()
    finally:
        out.free()


def untouched(blob):
    return blob == bytes([fenced.CANARY]) * len(blob)


def forward_sized(gpu, plane, ws, mode, param, flags=0, bs=1):
    """jpegx_internal_forward_f32_sized (float32 plane) or _u8_sized (uint8 plane, pooled bs x bs) into a fenced stream
    and the views of `ws`: (stream int16 (hb, wb, 64), the fenced device stream -- the caller frees it --, sized)."""
    L = hooks(gpu)
    a = np.ascontiguousarray(plane)
    hh, ww = a.shape
    H, W = hh // bs, ww // bs
    nblocks = (H // 8) * (W // 8)
    din, dzz = gpu.DeviceBuffer(a.nbytes), fenced.Fenced(gpu, nblocks * 128)
    try:
        din.upload(a)
        bb, wb, hb = ws.views(nblocks)
        sized = _int(-1)
        if a.dtype == np.float32:
            assert bs == 1
            rc = L.jpegx_internal_forward_f32_sized(din.ptr, H, W, ww, gpu.mode_of(mode), float(param), flags, dzz.ptr, bb, wb, hb,
                                                    ctypes.byref(sized), None)
        else:
            assert a.dtype == np.uint8
            rc = L.jpegx_internal_forward_u8_sized(din.ptr, H, W, ww, bs, gpu.mode_of(mode), float(param), flags, dzz.ptr, bb, wb, hb, None)
            sized = _int(1)
        gpu.check(rc, "forward_sized")
        zz = dzz.download(what="forward_sized stream").view(np.int16).reshape(H // 8, W // 8, 64).copy()
        return zz, dzz, sized.value
    except BaseException:
        dzz.free()
        raise
    finally:
        din.free()
