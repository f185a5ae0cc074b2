"""Device-side helpers of the batch-codec tests for dct_size != 8 (tests/test_gpu_batch_codec_n.py,
tests/test_gpu_batch_kernels_n.py): canaried device buffers and the per-band references.  A plain helper module of the
suite, like fenced.py and far.py."""
import numpy as np

CANARY = 0xA5
FENCE = 256                  # canary bytes in front of and behind the payload; a multiple of 16


class Fenced:
    """FENCE + nbytes + FENCE device bytes, every byte the canary; `ptr` is the payload's first byte (16-byte aligned
    plus `skew`)."""

    def __init__(self, gpu, nbytes, skew=0):
        self.gpu, self.nbytes, self.skew = gpu, int(nbytes), int(skew)
        self.total = FENCE + 16 + self.nbytes + FENCE
        self.buf = gpu.DeviceBuffer(self.total)
        assert self.buf.ptr % 16 == 0
        self.at = FENCE + self.skew
        self.ptr = self.buf.ptr + self.at
        self.fill()

    def fill(self):
        self.gpu.check(self.gpu.lib().jpegx_memset(self.buf.ptr, CANARY, self.total, None), "jpegx_memset")
        self.gpu.check(self.gpu.lib().jpegx_device_synchronize())

    def upload(self, array):
        a = np.ascontiguousarray(array)
        assert a.nbytes <= self.nbytes
        self.buf.upload(a, offset=self.at)

    def everything(self):
        """(front fence, payload, back fence) as uint8 arrays."""
        raw = self.buf.download((self.total,), np.uint8)
        return raw[:self.at], raw[self.at:self.at + self.nbytes], raw[self.at + self.nbytes:]

    def payload(self, written, what):
        """The payload after checking that both fences, and every payload byte from `written` on, still hold the canary."""
        front, body, back = self.everything()
        assert np.all(front == CANARY), "%s: bytes in front of the buffer were written" % what
        assert np.all(back == CANARY), "%s: bytes behind the buffer were written" % what
        assert np.all(body[written:] == CANARY), "%s: bytes behind the written part were written" % what
        return body[:written]

    def untouched(self, what):
        assert self.payload(0, what).size == 0

    def free(self):
        self.buf.free()


def pitched(rows2d, pitch, fill):
    """[r][cols] -> [r][pitch] with the gap behind every row filled with `fill`."""
    a = np.asarray(rows2d)
    out = np.full((a.shape[0], pitch), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def band_shape(hb, wb, n, bs, ragged):
    """(rows, cols) of a band whose plane of whole blocks is hb x wb blocks of n x n: exact, or with the longest Padding
    and DCTPadding on the rows and the shortest on the columns."""
    ph, pw = ((hb - 1) * n + 1, wb * n - 1) if ragged else (hb * n, wb * n)
    return (ph * bs - (bs - 1), pw * bs - (1 if bs > 1 else 0)) if ragged else (ph * bs, pw * bs)


def noise_bands(seed, nplanes, rows, cols, smooth_every=0):
    """uint8 [nplanes][rows][cols] of 8-bit noise; every `smooth_every`-th band a smooth ramp instead."""
    rng = np.random.default_rng(seed)
    bands = rng.integers(0, 256, (nplanes, rows, cols), dtype=np.uint8)
    if smooth_every:
        y, x = np.mgrid[0:rows, 0:cols]
        for p in range(0, nplanes, smooth_every):
            bands[p] = ((3 * y + 2 * x + 11 * p) // 4 % 256).astype(np.uint8)
    return bands
