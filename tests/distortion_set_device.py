"""What the GPU tests of the distortion probe over a set share: a set of 8-bit pictures on the device with its table, its
float64 block strip (jpegx_picture_set_blocks_n) and its moments (jpegx_picture_set_moments_n) -- the moments strip pre-filled
with 0xFF.. and the strip with 1e300, both between margins that keep their fill, so an unwritten or over-read word shows --,
jpegx_probe_distortion_set_n between canaries over garbage totals, and the yardstick: the road the probe stands for, run once
per candidate -- jpegx_forward_fused_n on the strip, jpegx_inverse_fused_n with the uint8 clamp, jpegx_picture_set_pixels_u8,
then NumPy's sum of squared differences against the pixels; the flag from |zz| > 16383 per plane.  A helper module of the
suite; the `gpu` module reaches it as an argument."""
import numpy as np

import picture_set_model as model

BAD = np.uint64(1 << 63)
CANARY = np.uint64(0xC0FFEE0DDBA11AD5)
GARBAGE = np.uint64(0xDEADBEEFDEADBEEF)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
MODES = {"none": 0, "discard": 1, "divide": 2}
MARGIN = 64                                              # words either side of the two strips
ANY = "any"                                              # check(expect_bad=ANY): the flags are the yardstick's, whichever they are


def sizes_for(shapes, n, bs=1, crops=None):
    """Picture sizes (rows, cols) whose bands are planes of hb x wb blocks at block_size bs; crops: (rows, cols) taken off the
    last block of each, below n * bs."""
    crops = crops or [(0, 0)] * len(shapes)
    out = []
    for (hb, wb), (cr, cc) in zip(shapes, crops):
        assert 0 <= cr < n * bs and 0 <= cc < n * bs
        out.append((hb * n * bs - cr, wb * n * bs - cc))
    return out


class PictureSet:
    """pictures: a list of uint8 [rows_p][cols_p][nb].  layout: a picture_set_model.Layout (offsets and pitches with slack), or
    None for the pictures back to back.  strip: a float64 strip to put in place of the gathered one (content made for a
    kernel test); the moments stay those of the pixels."""

    def __init__(self, gpu, pictures, bs, n, colour=0, layout=None, strip=None):
        self.gpu, self.L, self.bs, self.n, self.colour = gpu, gpu.lib(), bs, n, colour
        self.pictures = [np.ascontiguousarray(p, dtype=np.uint8) for p in pictures]
        self.sizes = [p.shape[:2] for p in self.pictures]
        self.nbands = self.pictures[0].shape[2]
        self.npictures = len(self.pictures)
        if layout is None:
            flat = np.concatenate([p.reshape(-1) for p in self.pictures])
            self.table = gpu.picture_set_table(self.sizes, self.nbands, bs, n)
        else:
            flat = layout.pack(self.pictures, 0x5A)
            self.table = gpu.picture_set_table(self.sizes, self.nbands, bs, n, offsets=layout.offsets, pitches=layout.pitches)
        self.layout = layout
        self.first = self.table.plane_first.astype(np.int64)          # nplanes + 1
        self.nplanes, self.nblk = len(self.first) - 1, int(self.first[-1])
        self.words = self.nblk * n * n
        self.dpx = gpu.DeviceBuffer(flat.nbytes)
        self.dpx.upload(flat)
        self.dtab = gpu.DeviceBuffer(self.table.nbytes)
        self.dtab.upload(self.table.blob.view(np.uint8)[:self.table.nbytes])
        self.dstrip = gpu.DeviceBuffer((self.words + 2 * MARGIN) * 8)
        self.dmom = gpu.DeviceBuffer((self.words + 2 * MARGIN) * 8)
        self.dzz = self.du8 = self.dback = None
        self.gather()
        if strip is not None:
            assert strip.shape == (self.nblk * n, n) and strip.dtype == np.float64
            whole = np.full(self.words + 2 * MARGIN, 1e300)
            whole[MARGIN:-MARGIN] = strip.reshape(-1)
            self.dstrip.upload(whole)

    def counts(self):
        return np.diff(self.first)

    def at(self, p0):
        """Byte offset of picture p0's first block inside either strip (the margin counted)."""
        return (MARGIN + int(self.first[p0 * self.nbands]) * self.n * self.n) * 8

    def gather(self, p0=0, k=None, device=None):
        """Both gathers of pictures p0 .. p0 + k - 1 into freshly filled strips; returns (strip float64, moments uint64, at): the
        two buffers with their margins and the word at which the range's first block was put -- its place in the whole strip,
        one word later where that place is not 16-byte aligned (odd N), as the gathers ask."""
        k = self.npictures - p0 if k is None else k
        place = self.at(p0) + (self.at(p0) & 8)
        self.dstrip.upload(np.full(self.words + 2 * MARGIN, 1e300))
        self.dmom.upload(np.full(self.words + 2 * MARGIN, ONES))
        self.gpu.picture_set_blocks_n_device(self.dpx.ptr, self.table, self.dtab.ptr, p0, k, self.dstrip.ptr + place, self.colour, device=device)
        self.gpu.picture_set_moments_n_device(self.dpx.ptr, self.table, self.dtab.ptr, p0, k, self.dmom.ptr + place, self.colour, device=device)
        self.gpu.check(self.L.jpegx_stream_synchronize(None))
        return self.dstrip.download((self.words + 2 * MARGIN,), np.float64), self.dmom.download((self.words + 2 * MARGIN,), np.uint64), place // 8

    def probe(self, mode, params, p0=0, k=None, device=None):
        """(sse int64, bad) [k * nbands][K] of pictures p0 .. p0 + k - 1, from totals that held garbage, between canaries."""
        k = self.npictures - p0 if k is None else k
        nk = len(params)
        count = k * self.nbands * nk
        dtot = self.gpu.DeviceBuffer((count + 4) * 8)
        try:
            fill = np.full(count + 4, GARBAGE)
            fill[:2] = fill[-2:] = CANARY
            dtot.upload(fill)
            self.gpu.probe_distortion_set_n_device(self.dstrip.ptr + self.at(p0), self.dmom.ptr + self.at(p0), self.table, self.dtab.ptr, p0, k,
                                                   MODES[mode], [float(v) for v in params], dtot.ptr + 16, device=device)
            self.gpu.check(self.L.jpegx_stream_synchronize(None))
            raw = dtot.download((count + 4,), np.uint64)
        finally:
            dtot.free()
        assert (raw[:2] == CANARY).all() and (raw[-2:] == CANARY).all(), "the probe wrote outside its rows of the totals"
        raw = raw[2:-2].reshape(k * self.nbands, nk)
        return (raw & ~BAD).astype(np.int64), (raw & BAD) != 0

    def reference_pixels(self):
        """What the decoded pixels are compared with: the pictures, with colour their model YCbCr."""
        return [model.model_of(p, self.colour).astype(np.int64) for p in self.pictures]

    def road(self, mode, params):
        """(sse int64 [nplanes][K], bad bool [nplanes][K]) of the whole set by the existing entries, once per candidate.  The
        scatter runs WITHOUT the colour conversion back: the error is measured in the coded bands."""
        g, L, n = self.gpu, self.L, self.n
        tall = self.nblk * n
        nout = sum(r * c * self.nbands for r, c in self.sizes)
        plain = g.picture_set_table(self.sizes, self.nbands, self.bs, n)          # the decoded pictures back to back
        if self.dzz is None:
            self.dzz = g.DeviceBuffer(self.words * 4)
            self.du8 = g.DeviceBuffer(self.words)
            self.dback = g.DeviceBuffer(nout)
            self.dplain = g.DeviceBuffer(plain.nbytes)
            self.dplain.upload(plain.blob.view(np.uint8)[:plain.nbytes])
        sse = np.empty((self.nplanes, len(params)), np.int64)
        bad = np.empty((self.nplanes, len(params)), bool)
        ref = self.reference_pixels()
        ends = np.concatenate([[0], np.cumsum([r * c * self.nbands for r, c in self.sizes])])
        for q, param in enumerate(params):
            g.check(L.jpegx_forward_fused_n(self.dstrip.ptr + MARGIN * 8, tall, n, n, n, MODES[mode], float(param), self.dzz.ptr, None),
                    "jpegx_forward_fused_n")
            g.check(L.jpegx_inverse_fused_n(self.dzz.ptr, tall, n, n, MODES[mode], float(param), g.F_CLAMP_U8, self.du8.ptr, n, None),
                    "jpegx_inverse_fused_n")
            g.picture_set_pixels_u8_device(self.du8.ptr, plain, self.dplain.ptr, 0, self.npictures, self.dback.ptr, 0)
            g.check(L.jpegx_stream_synchronize(None))
            flat = self.dback.download((nout,), np.uint8).astype(np.int64)
            top = np.abs(self.dzz.download((self.nblk, n * n), np.int32).astype(np.int64)).max(axis=1)
            for p, (r, c) in enumerate(self.sizes):
                back = flat[ends[p]:ends[p + 1]].reshape(r, c, self.nbands)
                sse[p * self.nbands:(p + 1) * self.nbands, q] = ((back - ref[p]) ** 2).sum(axis=(0, 1))
            bad[:, q] = np.maximum.reduceat(top, self.first[:-1]) > 16383
        return sse, bad

    def check(self, mode, params, p0=0, k=None, expect_bad=None, want=None, label=""):
        """The probe of pictures p0 .. p0 + k - 1 equals the yardstick's rows of those pictures, twice in a row; no cell is
        flagged unless expect_bad lists the (plane of the set, candidate) cells that must be, and exactly those.  want: (sse,
        bad) [nplanes][K] of the whole set from elsewhere in place of the yardstick."""
        k = self.npictures - p0 if k is None else k
        rows = slice(p0 * self.nbands, (p0 + k) * self.nbands)
        got, got_bad = self.probe(mode, params, p0, k)
        want, want_bad = (a[rows] for a in (self.road(mode, params) if want is None else want))
        print("%s N %d bs %d %s %s pictures %d..%d: sse %s bad %s" % (label, self.n, self.bs, mode, list(params)[:6], p0, p0 + k - 1,
                                                                      got[:3].tolist(), np.argwhere(got_bad)[:4].tolist()))
        where = np.argwhere(got_bad != want_bad)
        assert where.size == 0, "N %d %s %r: flags differ at (plane, candidate) %s" % (self.n, mode, list(params), where[:8].tolist())
        flagged = [[int(p) + rows.start, int(q)] for p, q in np.argwhere(got_bad)]
        if expect_bad is not ANY:
            assert flagged == sorted([list(c) for c in (expect_bad or [])]), (self.n, mode, list(params), flagged)
        ok = ~want_bad
        where = np.argwhere((got != want) & ok)
        assert where.size == 0, "N %d bs %d %s %r pictures %d..%d: %d sums differ, first (plane, candidate) %s: got %s for %s" % (
            self.n, self.bs, mode, list(params), p0, p0 + k - 1, len(where), where[:4].tolist(), [int(got[tuple(i)]) for i in where[:4]],
            [int(want[tuple(i)]) for i in where[:4]])
        again, again_bad = self.probe(mode, params, p0, k)
        assert np.array_equal(again_bad, got_bad) and np.array_equal(again[ok], got[ok]), "N %d: two calls in a row differ" % self.n
        return got

    def free(self):
        for b in (self.dpx, self.dtab, self.dstrip, self.dmom, self.dzz, self.du8, self.dback, getattr(self, "dplain", None)):
            if b is not None:
                b.free()
