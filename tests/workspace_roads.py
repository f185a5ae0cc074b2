"""The six batch roads (planes / pictures / sets, each at dct_size 8 and at any other) as one shape of job for the fenced-
workspace modules: a job knows its pixels or coefficient streams, what the product-free oracles make of them
(codec_oracle.py at 8 x 8, codec_oracle_n.py elsewhere, colour_model.py for RGB) and how to call its family's entries
with EXACTLY the arguments the job has.  A plain helper module of the suite.

The run-time-N roads agree with their oracle bit for bit only off the rounding ties, so their pixels are built as
codec_oracle_n.make_band builds them (multiples of a step, constant on the pooling tiles) and every job asserts the distance
of every coefficient and sample from a tie on the oracle's values alone (TieError: the builder takes the next seed)."""
import numpy as np
import pytest

import codec_oracle as o8
import codec_oracle_n as on
import colour_model
import oracle
from fenced import CANARY, Fenced
from workspace_fence import FencedWorkspace

FREE_MARGIN = 100.0          # as tests/test_codec_oracle_n.py: a tie-free value keeps this many tau from m + 1/2


class TieError(AssertionError):
    pass


def max_block_bytes(n):
    return (23 * n * n + 15) // 8


def model_of(picture, colour):
    return colour_model.rgb_to_ycbcr(picture) if colour else picture


class Road:
    """One job.  pictures: uint8 [rows][cols][nbands] each (a plane or band is a picture of one band).  kind: "planes",
    "pictures" or "set".  group: group_planes (planes, pictures) or group_samples (set).  coefficients: per plane an integer
    array (hb, wb, n * n) -- then the job is a decoding job only, its streams the oracle's coding of them."""

    def __init__(self, kind, pictures, bs, n, mode, param, colour=0, group=0, coefficients=None, elem=1):
        self.kind, self.bs, self.n, self.mode, self.param, self.colour, self.group, self.elem = kind, bs, n, mode, float(param), colour, group, elem
        self.pictures = [np.ascontiguousarray(p, np.uint8) for p in pictures]
        self.k, self.nb = len(self.pictures), self.pictures[0].shape[2]
        self.sizes = [p.shape[:2] for p in self.pictures]
        self.nplanes = self.k * self.nb
        assert kind == "set" or len(set(self.sizes)) == 1
        assert kind != "planes" or (self.nb == 1 and not colour)
        self.forward = coefficients is None
        if self.forward:
            self.blobs = [self._compress(model_of(p, colour)[:, :, b]) for p in self.pictures for b in range(self.nb)]
        else:
            self.blobs = [oracle.rle_bytestream(np.asarray(z).astype(np.int16)) for z in coefficients]
        assert len(self.blobs) == self.nplanes
        self.off = np.zeros(self.nplanes + 1, np.uint64)
        self.off[1:] = np.cumsum([len(b) for b in self.blobs])
        self.total = int(self.off[-1])
        self.stream = b"".join(self.blobs)
        self.decoded, self.decoded_bands = [], []
        for p, (rows, cols) in enumerate(self.sizes):
            bands = [self._decompress(self.blobs[p * self.nb + b], rows, cols) for b in range(self.nb)]
            self.decoded_bands += bands
            px = np.dstack(bands).astype(np.uint8)
            self.decoded.append(colour_model.ycbcr_to_rgb(px) if colour else px)
        self.table = self.d_table = None

    # ---- the oracles -------------------------------------------------------------------------------------------------
    def _compress(self, band):
        if self.n == 8:
            return o8.compress_reference(band, self.bs, self.mode, self.param)
        f = on.Forward(band, self.bs, self.n, self.mode, self.param)
        if not f.distance >= FREE_MARGIN * f.tau:
            raise TieError("a coefficient %g from a tie" % f.distance)
        return f.blob()

    def _decompress(self, blob, rows, cols):
        if self.n == 8:
            return o8.decompress_reference(blob, rows, cols, self.bs, self.mode, self.param)
        inv = on.Inverse(blob, rows, cols, self.bs, self.n, self.mode, self.param)
        if not np.all(inv.off >= FREE_MARGIN * inv.tau_inv):
            raise TieError("a decoded sample on a tie")
        return inv.band

    def blocks(self):
        """Blocks of every plane."""
        out = []
        for rows, cols in self.sizes:
            hb, wb = o8.blocks_of(rows, cols, self.bs) if self.n == 8 else on.blocks_of(rows, cols, self.bs, self.n)
            out += [hb * wb] * self.nb
        return out

    def longest_block(self):
        """(bytes of the longest block of the oracle's streams, the most non-zero coefficients a block of them holds)."""
        top = full = 0
        for blob, nblk in zip(self.blobs, self.blocks()):
            zz = oracle.rle_decode(blob, nblk, n=self.n * self.n).reshape(nblk, self.n * self.n)
            top = max([top] + [len(oracle.rle_bytestream(b[None].astype(np.int16))) for b in zz])
            full = max(full, int(np.count_nonzero(zz, axis=1).max()))
        return top, full

    # ---- the job's arguments ---------------------------------------------------------------------------------------------
    def shape(self):
        rows, cols = self.sizes[0]
        if self.kind == "planes":
            if self.n == 8:
                hb, wb = o8.blocks_of(rows, cols, self.bs)
                return (self.nplanes, hb * 8, wb * 8)
            return (self.nplanes, rows, cols, self.bs, self.n)
        return (self.k, self.nb, rows, cols, self.bs) + (() if self.n == 8 else (self.n,))

    def planes_8(self):
        """(nplanes, H, W) of the 8 x 8 plane batch behind the picture entries: what _status and _emit take."""
        hb, wb = o8.blocks_of(*self.sizes[0], self.bs)
        return (self.nplanes, hb * 8, wb * 8)

    def prepare(self, gpu):
        """Sets: the table (host arithmetic, no device)."""
        if self.kind == "set" and self.table is None:
            self.table = gpu.picture_set_table(self.sizes, self.nb, self.bs, self.n)
        return self

    def open(self, gpu):
        """Sets: the table and its device copy."""
        self.prepare(gpu)
        if self.kind == "set" and self.d_table is None:
            self.d_table = gpu.DeviceBuffer(self.table.blob.nbytes)
            self.d_table.upload(self.table.blob)
        return self

    def close(self):
        if self.d_table is not None:
            self.d_table.free()
            self.d_table = None

    def compress_align(self):
        return 16

    def decompress_align(self):
        return 256 if self.n == 8 else 16

    def compress_workspace_bytes(self, gpu):
        s, g = self.prepare(gpu).shape(), self.group
        if self.kind == "set":
            return (gpu.batch_set_workspace_bytes if self.n == 8 else gpu.batch_set_workspace_bytes_n)(self.table, g)
        if self.kind == "planes":
            return gpu.batch_workspace_bytes(*s) if self.n == 8 else gpu.batch_workspace_bytes_n(*s, g)
        if self.n == 8:
            return gpu.batch_pictures_workspace_bytes(*s, g)
        return gpu.batch_workspace_bytes_n(self.nplanes, *s[2:], g)

    def decompress_workspace_bytes(self, gpu, nbytes=None):
        s, g = self.prepare(gpu).shape(), self.group
        nbytes = self.total if nbytes is None else nbytes
        if self.kind == "set":
            return (gpu.batch_decompress_set_workspace_bytes if self.n == 8 else gpu.batch_decompress_set_workspace_bytes_n)(nbytes, self.table, g)
        if self.kind == "planes":
            return gpu.batch_decompress_workspace_bytes(nbytes, *s) if self.n == 8 else gpu.batch_decompress_workspace_bytes_n(nbytes, *s, g)
        if self.n == 8:
            return gpu.batch_decompress_pictures_workspace_bytes(nbytes, *s)
        return gpu.batch_decompress_pictures_workspace_bytes_n(nbytes, *s, g)

    # ---- device buffers ----------------------------------------------------------------------------------------------------
    def source(self):
        """The bytes the compress entry reads: pictures back to back; 8 x 8 planes at a pitch of whole 16 bytes."""
        if self.kind == "planes" and self.n == 8:
            rows, cols = self.sizes[0]
            assert rows % (8 * self.bs) == 0 and cols % (8 * self.bs) == 0
            self.pitch = (cols + 15) // 16 * 16 if self.elem == 1 else (cols + 3) // 4 * 4
            a = np.zeros((self.k * rows, self.pitch), np.uint8 if self.elem == 1 else np.float32)
            a[:, :cols] = np.concatenate([p[:, :, 0] for p in self.pictures])
            return a.view(np.uint8).reshape(-1)
        return np.concatenate([p.reshape(-1) for p in self.pictures])

    def compress(self, gpu, din, ws, dout, cap):
        s, g, m = self.shape(), self.group, (self.mode, self.param)
        if self.kind == "set":
            fn = gpu.batch_compress_picture_set_device if self.n == 8 else gpu.batch_compress_picture_set_n_device
            fn(din, self.table, self.d_table.ptr, ws, dout, cap, *m, self.colour, g)
        elif self.kind == "planes" and self.n == 8:
            flags = gpu.F_PIXEL_INPUT if self.elem == 4 else 0
            gpu.batch_compress_device(din, self.elem, *s, ws, dout, cap, *m, flags, pitch=self.pitch, block_size=self.bs)
        elif self.kind == "planes":
            gpu.batch_compress_n_device(din, *s, ws, dout, cap, *m, g)
        elif self.n == 8:
            gpu.batch_compress_pictures_device(din, *s, ws, dout, cap, g, *m, self.colour)
        else:
            gpu.batch_compress_pictures_n_device(din, *s, ws, dout, cap, g, *m, self.colour)

    def status(self, gpu, ws):
        g = self.group
        if self.kind == "set":
            return (gpu.batch_compress_status_set if self.n == 8 else gpu.batch_compress_status_set_n)(ws, self.table, g)
        if self.n == 8:
            return gpu.batch_compress_status(ws, *self.planes_8())
        return gpu.batch_compress_status_n(ws, self.nplanes, *self.sizes[0], self.bs, self.n, g)

    def emit(self, gpu, ws, dout, cap):
        g = self.group
        if self.kind == "set":
            fn = gpu.batch_emit_set_device if self.n == 8 else gpu.batch_emit_set_n_device
            fn(ws, self.table, self.d_table.ptr, dout, cap, g)
        elif self.n == 8:
            gpu.batch_emit_device(ws, *self.planes_8(), dout, cap)
        else:
            gpu.batch_emit_n_device(ws, self.nplanes, *self.sizes[0], self.bs, self.n, dout, cap, g)

    def decompress(self, gpu, dbytes, ws, dout, off=None):
        s, g, m = self.shape(), self.group, (self.mode, self.param)
        off = self.off if off is None else off
        if self.kind == "set":
            fn = gpu.batch_decompress_picture_set_device if self.n == 8 else gpu.batch_decompress_picture_set_n_device
            fn(dbytes, off, self.table, self.d_table.ptr, ws, dout, *m, self.colour, g)
        elif self.kind == "planes" and self.n == 8:
            gpu.batch_decompress_device(dbytes, off, *s, ws, dout, self.out_pitch(), self.bs, *m)
        elif self.kind == "planes":
            gpu.batch_decompress_n_device(dbytes, off, *s, ws, dout, None, *m, g)
        elif self.n == 8:
            gpu.batch_decompress_pictures_device(dbytes, off, *s, ws, dout, None, *m, self.colour)
        else:
            gpu.batch_decompress_pictures_n_device(dbytes, off, *s, ws, dout, g, None, *m, self.colour)

    def out_pitch(self):
        """8 x 8 planes come back at a pitch of whole 16 bytes."""
        return (self.sizes[0][1] + 15) // 16 * 16

    def expected(self):
        """The bytes the decompress entry leaves in a destination that held the canary."""
        if self.kind == "planes" and self.n == 8:
            rows, cols = self.sizes[0]
            a = np.full((self.k * rows, self.out_pitch()), CANARY, np.uint8)
            a[:, :cols] = np.concatenate([p[:, :, 0] for p in self.decoded])
            return a.reshape(-1)
        return np.concatenate([p.reshape(-1) for p in self.decoded])


# ---- the runs ------------------------------------------------------------------------------------------------------------------
def compress_on(gpu, job, ws, what=""):
    """Sizes only -> status -> emit into exactly the total -> status -> the whole compress in one go; the oracle's bytes and
    plane index every time; the guards after each step."""
    assert job.forward
    src = job.source()
    din, dout = Fenced(gpu, src.nbytes), Fenced(gpu, job.total)
    try:
        din.upload(src)
        job.compress(gpu, din.ptr, ws.ptr, None, 0)
        rc, total, off = job.status(gpu, ws.ptr)
        assert (rc, total) == (0, job.total) and np.array_equal(off, job.off), (what, rc, total, job.total)
        ws.check(what + ": a sizes-only compress and its status")
        job.emit(gpu, ws.ptr, dout.ptr, job.total)
        rc, total, off = job.status(gpu, ws.ptr)
        assert (rc, total) == (0, job.total) and np.array_equal(off, job.off), what
        assert dout.download(what=what + ": emit").tobytes() == job.stream, what + ": emit"
        ws.check(what + ": emit")
        gpu.check(gpu.lib().jpegx_memset(dout.ptr, CANARY, max(job.total, 1), None), "jpegx_memset")
        job.compress(gpu, din.ptr, ws.ptr, dout.ptr, job.total)
        rc, total, off = job.status(gpu, ws.ptr)
        assert (rc, total) == (0, job.total) and np.array_equal(off, job.off), what
        assert dout.download(what=what + ": compress").tobytes() == job.stream, what + ": compress"
        din.download(what=what + ": the pixels")
        ws.check(what + ": compress")
    finally:
        din.free()
        dout.free()


def decompress_on(gpu, job, ws, what="", stream=None, off=None, refused=False):
    """The oracle's stream (or `stream`) through the decompress entry; refused: None or a pattern the JpegxError must match."""
    stream = job.stream if stream is None else stream
    want = job.expected()
    slack = 16 if job.n == 8 else 0                       # the 8 x 8 decoders read 16 bytes behind the stream
    dbytes, dout = Fenced(gpu, len(stream) + slack), Fenced(gpu, want.nbytes)
    try:
        dbytes.upload(np.frombuffer(stream + bytes(slack), np.uint8))
        if refused is not False:
            with pytest.raises(gpu.JpegxError, match=refused):
                job.decompress(gpu, dbytes.ptr, ws.ptr, dout.ptr, off)
            dout.download(what=what + ": a refused decompress")
        else:
            job.decompress(gpu, dbytes.ptr, ws.ptr, dout.ptr, off)
            got = dout.download(what=what + ": decompress")
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s: %d samples differ from the oracle's, the first at %d" % (what, bad.size, bad[0])
        dbytes.download(what=what + ": the stream")
        ws.check(what + ": decompress")
    finally:
        dbytes.free()
        dout.free()


def both_ways(gpu, job, what):
    """Compress and decompress, each on a workspace of exactly its declared size."""
    job.open(gpu)
    try:
        if job.forward:
            nbytes = job.compress_workspace_bytes(gpu)
            assert nbytes > 0, what
            ws = FencedWorkspace(gpu, nbytes, job.compress_align())
            try:
                compress_on(gpu, job, ws, what)
            finally:
                ws.free()
        nbytes = job.decompress_workspace_bytes(gpu)
        assert nbytes > 0, what
        ws = FencedWorkspace(gpu, nbytes, job.decompress_align())
        try:
            decompress_on(gpu, job, ws, what)
        finally:
            ws.free()
    finally:
        job.close()


def reuse(gpu, large, small):
    """Larger, smaller, larger again on workspaces sized for the larger job, nothing refilled in between."""
    for job in (large, small):
        job.open(gpu)
    try:
        for sized, run, align in ((Road.compress_workspace_bytes, compress_on, large.compress_align()),
                                  (Road.decompress_workspace_bytes, decompress_on, large.decompress_align())):
            assert 0 < sized(small, gpu) <= sized(large, gpu)
            ws = FencedWorkspace(gpu, sized(large, gpu), align)
            try:
                for job, what in ((large, "the larger job"), (small, "the smaller job"), (large, "the larger job again")):
                    run(gpu, job, ws, what)
            finally:
                ws.free()
    finally:
        large.close()
        small.close()


# ---- content -------------------------------------------------------------------------------------------------------------------
def build(make, seeds=range(24)):
    """make(seed) -> Road; the first seed whose content the oracle finds free of ties."""
    for seed in seeds:
        try:
            return make(seed)
        except TieError:
            continue
    raise AssertionError("no tie-free content among the seeds")


def free_pictures(seed, sizes, nb, bs, n, mode, param, grey=False):
    """Pictures whose pooled samples are multiples of codec_oracle_n.make_band's step, constant on the pooling tiles, up to the
    peak that still codes in 15 bits.  grey: the bands of a picture are equal (RGB whose YCbCr is (v, 128, 128))."""
    rng = np.random.default_rng([seed, n, bs, nb, len(sizes)])
    step = 64 if mode == "divide" and abs(param) == 40.0 else 8 if mode == "divide" else 4
    peak = max(on.peak_for(n, mode, param), step)
    out = []
    for rows, cols in sizes:
        ph, pw = -(-rows // bs), -(-cols // bs)
        pooled = rng.integers(0, peak // step + 1, (ph, pw, 1 if grey else nb)) * step
        if grey:
            ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
            ycc = colour_model.rgb_to_ycbcr(ramp).astype(np.int64)
            source = {int(y): v for v, (y, cb, cr) in enumerate(ycc) if cb == 128 and cr == 128 and y % step == 0 and y <= peak}
            levels = np.array(sorted(source))
            assert levels.size >= 2, "no grey whose luma is a multiple of %d" % step
            wanted = levels[rng.integers(0, levels.size, (ph, pw, 1))]
            pooled = np.repeat(np.vectorize(source.get)(wanted), nb, axis=2)
        out.append(np.repeat(np.repeat(pooled, bs, 0), bs, 1)[:rows, :cols].astype(np.uint8))
    return out


def extreme_pictures(seed, sizes, nb):
    """Every sample 0 or 255: the busiest content 8 bits hold."""
    rng = np.random.default_rng([seed, nb, len(sizes)])
    return [(rng.integers(0, 2, (r, c, nb)) * 255).astype(np.uint8) for r, c in sizes]


def noise_pictures(seed, sizes, nb):
    rng = np.random.default_rng([seed, nb, len(sizes), 7])
    return [rng.integers(0, 256, (r, c, nb), dtype=np.uint8) for r, c in sizes]


def crafted(kind, blocks, n, seed=0):
    """Coefficient streams written down directly, one (1, blocks, n * n) array a plane: "zero" (one byte a block), "worst"
    (every coefficient +-16383: max_block_bytes(n) a block), "small" (a DC and a few low frequencies)."""
    out = []
    for p, nblk in enumerate(blocks):
        rng = np.random.default_rng([seed, p, nblk, n])
        if kind == "zero":
            z = np.zeros((1, nblk, n * n), np.int32)
        elif kind == "worst":
            z = np.where(rng.random((1, nblk, n * n)) < 0.5, -16383, 16383).astype(np.int32)
        else:
            z = np.zeros((1, nblk, n * n), np.int32)
            z[..., 0] = rng.integers(10, 23, (1, nblk)) * 4                  # multiples of 4: off the halves of the N = 2 inverse
            z[..., 1:min(4, n * n)] = rng.integers(-1, 2, (1, nblk, min(4, n * n) - 1)) * 4
        out.append(z)
    return out
