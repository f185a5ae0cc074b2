"""What the GPU tests of the distortion probe share: a stack of 8-bit bands on the device with its float64 planes and its
moments, jpegx_probe_distortion_n between canaries, and the road the probe stands for, run once per candidate --
jpegx_forward_fused_n, jpegx_inverse_fused_n with the uint8 clamp, jpegx_inflate_crop_stacked_u8, then NumPy's sum of squared
differences against the bands."""
import numpy as np

MODES = {"none": 0, "discard": 1, "divide": 2}
BAD = np.uint64(1 << 63)
CANARY = np.uint64(0xC0FFEE0DDBA11AD5)


class Stack:
    """bands uint8 [nplanes][rows][cols], every band pooled bs x bs and transformed in n x n blocks.  pad, mpad: elements added
    to the pitch of the planes and of the moments; the planes' gap holds 1e300, which would flag everything if it were read."""

    def __init__(self, gpu, bands, bs, n, pad=0, mpad=0):
        bands = np.ascontiguousarray(bands, dtype=np.uint8)
        self.gpu, self.L, self.bs, self.n, self.bands = gpu, gpu.lib(), bs, n, bands
        self.nplanes, self.rows, self.cols = bands.shape
        self.h, self.w = gpu.band_shape_n(self.rows, self.cols, bs, n)
        self.pitch, self.mpitch = self.w + pad, self.w + mpad
        self.bpp = (self.h // n) * (self.w // n)
        tall = self.nplanes * self.h
        self.dbands = gpu.DeviceBuffer(bands.nbytes)
        self.dbands.upload(bands)
        self.dplanes = gpu.DeviceBuffer(tall * self.pitch * 8)
        self.dplanes.upload(np.full((tall, self.pitch), 1e300))
        self.dmom = gpu.DeviceBuffer(tall * self.mpitch * 8)
        self.dmom.upload(np.full((tall, self.mpitch), np.uint64(0xFFFFFFFFFFFFFFFF)))
        gpu.band_planes_stacked_n_device(self.dbands.ptr, self.nplanes, self.rows, self.cols, bs, n, self.dplanes.ptr, out_pitch=self.pitch)
        gpu.band_moments_packed_stacked_n_device(self.dbands.ptr, self.nplanes, 1, self.rows, self.cols, bs, n, self.dmom.ptr, out_pitch=self.mpitch)
        gpu.check(self.L.jpegx_stream_synchronize(None))
        self.dzz = self.du8 = self.dback = None

    def moments(self):
        """uint64 [nplanes][H][W] as the gather wrote them."""
        return self.dmom.download((self.nplanes * self.h, self.mpitch), np.uint64)[:, :self.w].reshape(self.nplanes, self.h, self.w)

    def probe(self, mode, params, device=None):
        k = len(params)
        count = self.nplanes * k
        dtot = self.gpu.DeviceBuffer((count + 4) * 8)
        fill = np.full(count + 4, np.uint64(0xDEADBEEFDEADBEEF))        # garbage where the totals go
        fill[:2] = fill[-2:] = CANARY
        dtot.upload(fill)
        self.gpu.probe_distortion_n_device(self.dplanes.ptr, self.dmom.ptr, self.nplanes, self.h, self.w, self.n, self.bs, self.rows, self.cols,
                                           mode, params, dtot.ptr + 16, pitch=self.pitch, mpitch=self.mpitch, device=device)
        self.gpu.check(self.L.jpegx_stream_synchronize(None))
        raw = dtot.download((count + 4,), np.uint64)
        dtot.free()
        assert (raw[:2] == CANARY).all() and (raw[-2:] == CANARY).all()
        raw = raw[2:-2].reshape(self.nplanes, k)
        return (raw & ~BAD).astype(np.int64), (raw & BAD) != 0

    def road(self, mode, params):
        """(sse int64 [nplanes][K], bad bool [nplanes][K]) by the existing entries, once per candidate."""
        g, L, n = self.gpu, self.L, self.n
        tall = self.nplanes * self.h
        if self.dzz is None:
            self.dzz = g.DeviceBuffer(tall * self.w * 4)
            self.du8 = g.DeviceBuffer(tall * self.w)
            self.dback = g.DeviceBuffer(self.bands.nbytes)
        sse = np.empty((self.nplanes, len(params)), np.int64)
        bad = np.empty((self.nplanes, len(params)), bool)
        ref = self.bands.astype(np.int64)
        for q, param in enumerate(params):
            g.check(L.jpegx_forward_fused_n(self.dplanes.ptr, tall, self.w, self.pitch, n, MODES[mode], float(param), self.dzz.ptr, None),
                    "jpegx_forward_fused_n")
            g.check(L.jpegx_inverse_fused_n(self.dzz.ptr, tall, self.w, n, MODES[mode], float(param), g.F_CLAMP_U8, self.du8.ptr, self.w, None),
                    "jpegx_inverse_fused_n")
            g.inflate_crop_stacked_u8_device(self.du8.ptr, self.nplanes, self.h, self.w, self.rows, self.cols, self.bs, self.dback.ptr)
            g.check(L.jpegx_stream_synchronize(None))
            back = self.dback.download(self.bands.shape, np.uint8).astype(np.int64)
            zz = self.dzz.download((self.nplanes, self.h * self.w), np.int32).astype(np.int64)
            sse[:, q] = ((back - ref) ** 2).sum(axis=(1, 2))
            bad[:, q] = (np.abs(zz) > 16383).any(axis=1)
        return sse, bad

    def check(self, mode, params, want=None, label=""):
        """The probe against (sse, bad) -- the road's when none is given -- exactly, twice in a row; returns what the probe gave."""
        got, got_bad = self.probe(mode, params)
        want, want_bad = self.road(mode, params) if want is None else want
        print("%s N %d bs %d %s %s: sse %s bad %s" % (label, self.n, self.bs, mode, list(params), got[:4].tolist(), got_bad[:4].tolist()))
        assert np.array_equal(got_bad, want_bad), (label, self.n, self.bs, params, np.argwhere(got_bad != want_bad)[:8].tolist())
        same = (got == want) | want_bad
        assert same.all(), (label, self.n, self.bs, params, np.argwhere(~same)[:8].tolist(), got[~same][:8].tolist(), want[~same][:8].tolist())
        again, again_bad = self.probe(mode, params)
        assert np.array_equal(again_bad, got_bad) and np.array_equal(again[~got_bad], got[~got_bad])
        return got, got_bad

    def free(self):
        for b in (self.dbands, self.dplanes, self.dmom, self.dzz, self.du8, self.dback):
            if b is not None:
                b.free()
