"""Device buffers whose addresses lie more than 2^32 bytes from their base, for tests/test_gpu_far_pitch.py (small data,
rows a long pitch apart) and tests/test_gpu_far_count.py (real volume past the wrap point), and the layouts of both,
which tests/test_far_layout.py checks on the CPU.  A plain helper module of the suite, like fenced.py.

A far buffer is never downloaded as a whole: rows go up and come down one by one, and what must not have been written is
looked at through byte windows -- the guards, the slack next to every written row, and the ALIAS windows 2^32 bytes below
and above every written row, which is where a store whose byte offset lost its high bits would land."""
import numpy as np
import pytest

CANARY = 0xA5
GUARD = 256                  # bytes in front of and behind every span; a multiple of 16
SLACK = 256                  # bytes looked at on either side of a written row
WRAP = 1 << 32
LIMIT = 16 << 30             # most device memory one test may hold


# ---- layouts (no device needed) ---------------------------------------------------------------------------------------------
def far_pitch(nrows, align):
    """Bytes between two rows of a plane of `nrows` rows such that its later rows start past 2^32 bytes: 2^26 + align for
    72 rows and more (row 64 is the first far one), else 2^32 / (nrows / 2) + align (the second half is far)."""
    assert nrows >= 2
    step = (WRAP >> 6) if nrows >= 72 else -(-WRAP // (nrows // 2))
    return (step + align - 1) // align * align + align


class Rows:
    """`nrows` rows of `row_bytes` bytes, `pitch` bytes apart, the first `start` bytes into the span."""

    def __init__(self, nrows, row_bytes, pitch, start=0):
        assert pitch >= row_bytes > 0 and nrows >= 1 and start >= 0
        self.nrows, self.row_bytes, self.pitch, self.start = int(nrows), int(row_bytes), int(pitch), int(start)

    @property
    def nbytes(self):
        return self.start + (self.nrows - 1) * self.pitch + self.row_bytes

    def offsets(self):
        return self.start + np.arange(self.nrows, dtype=np.int64) * self.pitch

    def extents(self):
        return [(int(o), self.row_bytes) for o in self.offsets()]

    def far_rows(self):
        return np.flatnonzero(self.offsets() >= WRAP)


def far_rows_layout(nrows, row_bytes, align, start=0):
    return Rows(nrows, row_bytes, far_pitch(nrows, align), start)


class SparseModel:
    """A span of canary bytes with rows of data in it, on the host: what a load from any address of the span gives, and
    hence what a kernel computes when its byte offsets lose their high bits.  rows: [(far.Rows, data)], all in one span."""

    def __init__(self, rows):
        starts, chunks = [], []
        for layout, data in rows:
            raw = np.ascontiguousarray(data).reshape(layout.nrows, -1).view(np.uint8)
            assert raw.shape[1] == layout.row_bytes
            starts += [int(o) for o in layout.offsets()]
            chunks += list(raw)
        order = np.argsort(starts)
        self.starts = np.array(starts, np.int64)[order]
        self.chunks = [chunks[i] for i in order]
        self.ends = self.starts + np.array([c.size for c in self.chunks], np.int64)
        assert np.all(self.ends[:-1] <= self.starts[1:]), "rows of one span overlap"

    def read(self, addr, n):
        out = np.full(n, CANARY, np.uint8)
        first = int(np.searchsorted(self.ends, addr, side="right"))
        last = int(np.searchsorted(self.starts, addr + n, side="left"))
        for i in range(first, last):
            lo, hi = max(addr, int(self.starts[i])), min(addr + n, int(self.ends[i]))
            if lo < hi:
                out[lo - addr:hi - addr] = self.chunks[i][lo - int(self.starts[i]):hi - int(self.starts[i])]
        return out

    def truncated_rows(self, layout):
        """The rows of `layout` as a kernel reads them whose byte offset from the span's start is cut to 32 bits."""
        return np.stack([self.read(int(o) & (WRAP - 1), layout.row_bytes) for o in layout.offsets()])


def pooled_staged_offsets(wb, nblk, pitch, bs, wave=0):
    """The staged pooled loader's per-lane byte offsets from the wave's first block (csrc/jpegx_forward.hip,
    forward_fused_body with STAGED != 0), untruncated: (2 bs, 64) int64 offsets and the block each one belongs to."""
    cpb, gsh, g0 = 2 * bs, (2 if bs == 2 else 1), wave * 64
    by0, bx0 = divmod(g0, wb)
    off, blk = np.empty((cpb, 64), np.int64), np.empty((cpb, 64), np.int64)
    for j in range(cpb):
        for lane in range(64):
            slot = 64 * j + lane
            b, sl = divmod(slot, cpb)
            q = sl ^ ((b >> gsh) & (cpb - 1))
            gb = min(g0 + b, nblk - 1)
            byb, bxb = divmod(gb, wb)
            off[j, lane] = ((byb - by0) * 8 * bs * pitch + (bxb - bx0) * 8 * bs + q * 4) * 4
            blk[j, lane] = gb
    return off, blk


def pooled_span_is_far(H, W, pitch, bs):
    """The library's dispatch condition restated: min(ceil(64 / wb), H / 8) * 8 bs * pitch * 4 + row bytes >= 2^32."""
    wb = W // 8
    return min(-(-64 // wb), H // 8) * 8 * bs * pitch * 4 + W * bs * 4 >= WRAP


# ---- windows and periodic streams (part B) ------------------------------------------------------------------------------------
def windows(total, extent, seed, align=1, count=16):
    """Sorted, distinct start offsets of the `extent`-byte windows that part B downloads from a span of `total` bytes: the
    first and the last, one straddling every multiple of 2^32 inside the span, and `count` pseudo-random ones."""
    assert 0 < extent <= total and extent % align == 0 and total % align == 0
    last = total - extent
    out = {0, last}
    k = WRAP
    while k < total:
        out.add(min(max(0, (k - extent // 2) // align * align), last))
        k += WRAP
    rng = np.random.default_rng(seed)
    while len(out) < 2 + (total - 1) // WRAP + count and len(out) < last // align + 1:
        out.add(int(rng.integers(0, last // align + 1)) * align)
    return sorted(out)


def periodic_expected(period_bytes, start, n):
    """Bytes start .. start + n of the stream that repeats `period_bytes` for ever."""
    p = np.frombuffer(period_bytes, np.uint8) if isinstance(period_bytes, (bytes, bytearray)) else np.asarray(period_bytes, np.uint8).ravel()
    return p[(int(start) + np.arange(int(n), dtype=np.int64)) % p.size]


# ---- the device side ----------------------------------------------------------------------------------------------------------
class FarBuffer:
    """One device allocation of GUARD + nbytes + GUARD bytes, every byte 0xA5 (set on the device); `ptr` is the span's
    first byte.  Offsets are relative to the span and may reach into the guards."""

    def __init__(self, gpu, nbytes):
        self.gpu, self.nbytes = gpu, int(nbytes)
        total = self.nbytes + 2 * GUARD
        assert total <= LIMIT, "a far buffer of %d bytes is beyond the %d a test may hold" % (total, LIMIT)
        try:
            self.buf = gpu.DeviceBuffer(total)
        except gpu.JpegxError as exc:
            pytest.skip("jpegx_malloc refused %d bytes (%.2f GiB): %s" % (total, total / 2.0 ** 30, exc))
        self.ptr = self.buf.ptr + GUARD
        try:
            gpu.check(gpu.lib().jpegx_memset(self.buf.ptr, CANARY, total, None), "jpegx_memset")
            gpu.check(gpu.lib().jpegx_device_synchronize())
        except BaseException:
            self.buf.free()
            raise

    def free(self):
        self.buf.free()

    def upload(self, array, offset=0):
        a = np.ascontiguousarray(array)
        assert 0 <= offset and offset + a.nbytes <= self.nbytes
        self.buf.upload(a, offset=GUARD + int(offset))

    def download(self, offset, nbytes):
        assert -GUARD <= offset and offset + nbytes <= self.nbytes + GUARD
        return self.buf.download((int(nbytes),), np.uint8, offset=GUARD + int(offset))

    def upload_rows(self, layout, data):
        raw = np.ascontiguousarray(data).reshape(layout.nrows, -1).view(np.uint8)
        assert raw.shape[1] == layout.row_bytes and layout.nbytes <= self.nbytes
        for o, row in zip(layout.offsets(), raw):
            self.upload(row, int(o))

    def download_rows(self, layout, dtype=np.uint8):
        self.gpu.check(self.gpu.lib().jpegx_device_synchronize())
        return np.stack([self.download(int(o), layout.row_bytes) for o in layout.offsets()]).view(dtype)

    def check_canary(self, wins, written=(), what=""):
        """Every byte of the (offset, nbytes) windows `wins` that lies in the allocation and in none of the `written`
        extents still holds the canary."""
        self.gpu.check(self.gpu.lib().jpegx_device_synchronize())
        ws = np.array([w[0] for w in written], np.int64)
        we = ws + np.array([w[1] for w in written], np.int64)
        for off, n in wins:
            lo, hi = max(int(off), -GUARD), min(int(off) + int(n), self.nbytes + GUARD)
            if lo >= hi:
                continue
            got = self.download(lo, hi - lo)
            keep = np.ones(hi - lo, bool)
            for s, e in zip(ws[(ws < hi) & (we > lo)], we[(ws < hi) & (we > lo)]):
                keep[max(int(s), lo) - lo:min(int(e), hi) - lo] = False
            bad = np.flatnonzero((got != CANARY) & keep)
            assert bad.size == 0, "%s: %d bytes outside the output were written, the first at byte %d of the span" % (what, bad.size, lo + bad[0])

    def check_output(self, written, what=""):
        """The windows every output check includes, for the (offset, nbytes) extents an entry may have written: both
        guards, the slack on either side of every extent, and every extent's aliases 2^32 bytes below and above."""
        wins = [(-GUARD, GUARD), (self.nbytes, GUARD)]
        for off, n in written:
            wins += [(off - SLACK, SLACK), (off + n, SLACK), (off - WRAP, n), (off + WRAP, n)]
        self.check_canary(wins, written, what)


def output_windows(written):
    """The span-relative windows of FarBuffer.check_output, for the CPU checks of a layout."""
    wins = []
    for off, n in written:
        wins += [("slack", off - SLACK, SLACK), ("slack", off + n, SLACK), ("alias", off - WRAP, n), ("alias", off + WRAP, n)]
    return wins


def tile_fill(gpu, buf, pattern_bytes, total_bytes, offset=0):
    """`pattern_bytes` repeated over total_bytes bytes of `buf` from `offset`: one upload, then device-to-device copies
    that double what is there."""
    p = np.frombuffer(pattern_bytes, np.uint8) if isinstance(pattern_bytes, (bytes, bytearray)) else np.ascontiguousarray(pattern_bytes).view(np.uint8).ravel()
    n, total = min(p.size, int(total_bytes)), int(total_bytes)
    assert offset >= 0 and offset + total <= buf.nbytes
    buf.upload(p[:n], offset)
    base = buf.ptr + offset
    while n < total:
        c = min(n, total - n)
        gpu.check(gpu.lib().jpegx_memcpy_d2d(base + n, base, c, None), "jpegx_memcpy_d2d")
        n += c
    gpu.check(gpu.lib().jpegx_device_synchronize())
