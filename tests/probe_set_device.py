"""What the GPU tests of jpegx_probe_sizes_set_n share: a float64 block strip with its picture-set table on the device, the
probe between canaries, and the yardstick -- the road the probe stands for, run once per candidate on the same strip:
jpegx_forward_fused_n (the strip is a plane of width N), jpegx_entropy_sizes_n, jpegx_entropy_block_sizes, and the per-block
sizes summed over each plane's block range from the table.  A helper module of the suite; the `gpu` module reaches it as an
argument."""
import numpy as np

BAD = np.uint64(1 << 63)
CANARY = np.uint64(0xC0FFEE0DDBA11AD5)
GARBAGE = np.uint64(0xDEADBEEFDEADBEEF)
MODES = {"none": 0, "discard": 1, "divide": 2}


def strip_of(plane, n):
    """A plane [hb * n][wb * n] as its blocks, row-major, one under the other: [hb * wb * n][n]."""
    hb, wb = plane.shape[0] // n, plane.shape[1] // n
    return plane.reshape(hb, n, wb, n).transpose(0, 2, 1, 3).reshape(hb * wb * n, n)


def sizes_for(counts, n):
    """Picture sizes (rows, cols) whose bands are planes of `counts` blocks at block_size 1: one row of blocks each."""
    return [(n, c * n) for c in counts]


class SetStrip:
    """strip [nblk * n][n] float64 of a set whose pictures have the sizes given (block_size 1), on the device with its table."""

    def __init__(self, gpu, strip, sizes, nbands, n):
        self.gpu, self.L, self.n, self.nbands = gpu, gpu.lib(), n, nbands
        self.table = gpu.picture_set_table(sizes, nbands, 1, n)
        self.npictures = len(sizes)
        self.first = self.table.plane_first.astype(np.int64)          # nplanes + 1
        self.nplanes, self.nblk = len(self.first) - 1, int(self.first[-1])
        assert strip.shape == (self.nblk * n, n) and strip.dtype == np.float64
        self.strip = np.ascontiguousarray(strip)
        self.din = gpu.DeviceBuffer(self.strip.nbytes)
        self.din.upload(self.strip)
        self.dtab = gpu.DeviceBuffer(self.table.nbytes)
        self.dtab.upload(self.table.blob.view(np.uint8)[:self.table.nbytes])
        self.dzz = gpu.DeviceBuffer(self.nblk * n * n * 4)
        self.dws = gpu.DeviceBuffer(self.L.jpegx_entropy_workspace_bytes_n(self.nblk, n * n))
        self._yard = {}

    def counts(self):
        return np.diff(self.first)

    def probe(self, mode, params, p0=0, k=None, device=None):
        """(sizes, bad) [k * nbands][K] of pictures p0 .. p0 + k - 1, from totals that held garbage, between canaries."""
        k = self.npictures - p0 if k is None else k
        nk = len(params)
        count = k * self.nbands * nk
        dtot = self.gpu.DeviceBuffer((count + 4) * 8)
        try:
            fill = np.full(count + 4, GARBAGE)
            fill[:2] = fill[-2:] = CANARY
            dtot.upload(fill)
            at = int(self.first[p0 * self.nbands]) * self.n * self.n * 8
            self.gpu.probe_sizes_set_n_device(self.din.ptr + at, self.table, self.dtab.ptr, p0, k, MODES[mode], [float(v) for v in params],
                                              dtot.ptr + 16, device=device)
            self.gpu.check(self.L.jpegx_stream_synchronize(None))
            raw = dtot.download((count + 4,), np.uint64)
        finally:
            dtot.free()
        assert (raw[:2] == CANARY).all() and (raw[-2:] == CANARY).all(), "the probe wrote outside its rows of the totals"
        raw = raw[2:-2].reshape(k * self.nbands, nk)
        return raw & ~BAD, (raw & BAD) != 0

    def yardstick(self, mode, params):
        """(sizes, bad) [nplanes][K] of the whole set; one candidate's column is computed once and kept."""
        nn = self.n * self.n
        sizes, bad = np.empty((self.nplanes, len(params)), np.uint64), np.empty((self.nplanes, len(params)), bool)
        per_block = np.empty(self.nblk, np.uint32)
        for q, param in enumerate(params):
            key = (mode, float(param))
            if key not in self._yard:
                self.gpu.check(self.L.jpegx_forward_fused_n(self.din.ptr, self.nblk * self.n, self.n, self.n, self.n, MODES[mode], float(param),
                                                            self.dzz.ptr, None), "jpegx_forward_fused_n")
                self.gpu.check(self.L.jpegx_entropy_sizes_n(self.dzz.ptr, self.nblk, nn, self.dws.ptr, None), "jpegx_entropy_sizes_n")
                self.gpu.check(self.L.jpegx_entropy_block_sizes(self.dws.ptr, self.nblk, per_block.ctypes.data, None))
                top = np.abs(self.dzz.download((self.nblk, nn), np.int32).astype(np.int64)).max(axis=1)
                before = np.concatenate([[0], np.cumsum(per_block, dtype=np.uint64)])
                col = before[self.first[1:]] - before[self.first[:-1]]
                flag = np.maximum.reduceat(top, self.first[:-1]) > 16383
                self._yard[key] = (col, flag)
            sizes[:, q], bad[:, q] = self._yard[key]
        return sizes, bad

    def check(self, mode, params, p0=0, k=None, expect_bad=None, want=None):
        """The probe of pictures p0 .. p0 + k - 1 equals the yardstick's rows of those pictures, twice in a row; no cell is
        flagged unless expect_bad lists the (plane of the set, candidate) cells that must be, and exactly those.  want: (sizes,
        bad) [nplanes][K] of the whole set from elsewhere (an oracle) in place of the yardstick."""
        k = self.npictures - p0 if k is None else k
        rows = slice(p0 * self.nbands, (p0 + k) * self.nbands)
        got, got_bad = self.probe(mode, params, p0, k)
        want, want_bad = (a[rows] for a in (self.yardstick(mode, params) if want is None else want))
        where = np.argwhere(got_bad != want_bad)
        assert where.size == 0, "N %d %s %r: flags differ at (plane, candidate) %s" % (self.n, mode, list(params), where[:8].tolist())
        flagged = [[int(p) + rows.start, int(q)] for p, q in np.argwhere(got_bad)]
        assert flagged == sorted([list(c) for c in (expect_bad or [])]), (self.n, mode, list(params), flagged)
        ok = ~want_bad
        where = np.argwhere((got != want) & ok)
        assert where.size == 0, "N %d %s %r pictures %d..%d: %d sizes differ, first (plane, candidate) %s: got %s for %s" % (
            self.n, mode, list(params), p0, p0 + k - 1, len(where), where[:4].tolist(), [int(got[tuple(i)]) for i in where[:4]],
            [int(want[tuple(i)]) for i in where[:4]])
        again, again_bad = self.probe(mode, params, p0, k)
        assert np.array_equal(again_bad, got_bad) and np.array_equal(again[ok], got[ok]), "N %d: two calls in a row differ" % self.n
        return got

    def free(self):
        for b in (self.din, self.dtab, self.dzz, self.dws):
            b.free()
