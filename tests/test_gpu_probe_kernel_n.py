"""jpegx_probe_sizes_n against the road it stands for, run once per candidate on the same float64 planes:
jpegx_forward_fused_n + jpegx_entropy_sizes_n + the per-block sizes summed per plane.  Every comparison is exact.
Sizes 2..32 cover 64..1 blocks per workgroup, block lengths below 64, at 64, no multiple of 64 and 1024, and the strided passes
from 17 up; planes of 2 x 3 and 5 x 7 blocks leave the last workgroup partial and let workgroups straddle planes at N <= 7."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE, DISCARD, DIVIDE = 0, 1, 2
SIZES = [2, 3, 4, 7, 8, 9, 12, 16, 17, 24, 32]
BAD = np.uint64(1 << 63)
CANARY = np.uint64(0xC0FFEE0DDBA11AD5)


def _speck_plane(gpu, n, hb, wb, seed):
    """Flat blocks with one speck each: the flat level plus one basis function, so that the block holds its DC and ONE more
    coefficient, at zigzag position 15, 16, 63, 64 or N*N - 1 in turn -- chain codes up to and across a 64-step boundary."""
    c, _, _, zig = gpu.dct_tables_n(n)
    spots = [p for p in (15, 16, 63, 64, n * n - 1) if 0 < p < n * n] or [n * n - 1]
    plane = np.empty((hb * n, wb * n))
    for b in range(hb * wb):
        src = int(zig[spots[(b + seed) % len(spots)]])
        k, l = divmod(src, n)
        # the speck's coefficient is amp * |c_k|^2 |c_l|^2, between 3000 and 12000: inside the 15 bits of a code under divisor 1
        block = 10.0 + (1.0 if (b + seed) % 2 else -0.75) * 3000.0 / (n / 2.0) ** 2 * np.outer(c[k], c[l])
        y, x = divmod(b, wb)
        plane[y * n:(y + 1) * n, x * n:(x + 1) * n] = block
    return plane


def _planes(gpu, n, hb, wb, nplanes, seed=0):
    """nplanes planes [hb * n][wb * n], the four kinds of content in turn: noise, a smooth ramp, specks, all zero.  The samples
    stay within +-12000 / N^2 (128 at most), so that no coefficient of the unnormalised transform leaves the 15 bits of a code
    under divisor 1 and every total of the ordinary cases is compared."""
    rng = np.random.default_rng(1000 * n + seed)
    h, w = hb * n, wb * n
    yy, xx = np.mgrid[0:h, 0:w]
    amp = min(128.0, 12000.0 / (n * n))
    out = []
    for p in range(nplanes):
        kind = (p + seed) % 4
        if kind == 0:
            out.append(np.round(rng.uniform(-amp, amp, (h, w)), 2))
        elif kind == 1:
            out.append(((yy * 1.75 + xx * 0.5 + p) / (h * 1.75 + w * 0.5 + p) * 2.0 - 1.0) * amp)
        elif kind == 2:
            out.append(_speck_plane(gpu, n, hb, wb, p))
        else:
            out.append(np.zeros((h, w)))
    return np.stack(out)


class Device:
    """The planes on the device at a pitch, the probe between canaries, and the yardstick."""

    def __init__(self, gpu, planes, n, pad=0):
        self.gpu, self.L, self.n = gpu, gpu.lib(), n
        self.nplanes, self.h, self.w = planes.shape
        self.pitch = self.w + pad
        tall = np.full((self.nplanes * self.h, self.pitch), 1e300)      # the pitch gap would flag everything if it were read
        tall[:, :self.w] = planes.reshape(-1, self.w)
        self.bpp = (self.h // n) * (self.w // n)
        self.nblk = self.nplanes * self.bpp
        self.din = gpu.DeviceBuffer(tall.nbytes)
        self.din.upload(tall)
        self.dzz = gpu.DeviceBuffer(self.nblk * n * n * 4)
        self.dws = gpu.DeviceBuffer(self.L.jpegx_entropy_workspace_bytes_n(self.nblk, n * n))

    def probe(self, mode, params):
        k = len(params)
        count = self.nplanes * k
        dtot = self.gpu.DeviceBuffer((count + 4) * 8)
        fill = np.full(count + 4, np.uint64(0xDEADBEEFDEADBEEF))        # garbage where the totals go
        fill[:2] = fill[-2:] = CANARY
        dtot.upload(fill)
        self.gpu.probe_sizes_n_device(self.din.ptr, self.nplanes, self.h, self.w, self.n, mode, params, dtot.ptr + 16, pitch=self.pitch)
        self.gpu.check(self.L.jpegx_stream_synchronize(None))
        raw = dtot.download((count + 4,), np.uint64)
        dtot.free()
        assert (raw[:2] == CANARY).all() and (raw[-2:] == CANARY).all()
        raw = raw[2:-2].reshape(self.nplanes, k)
        return raw & ~BAD, (raw & BAD) != 0

    def yardstick(self, mode, params):
        nn = self.n * self.n
        sizes, bad = np.empty((self.nplanes, len(params)), np.uint64), np.empty((self.nplanes, len(params)), bool)
        per_block = np.empty(self.nblk, np.uint32)
        for q, param in enumerate(params):
            self.gpu.check(self.L.jpegx_forward_fused_n(self.din.ptr, self.nplanes * self.h, self.w, self.pitch, self.n, mode, float(param),
                                                        self.dzz.ptr, None), "jpegx_forward_fused_n")
            self.gpu.check(self.L.jpegx_entropy_sizes_n(self.dzz.ptr, self.nblk, nn, self.dws.ptr, None), "jpegx_entropy_sizes_n")
            self.gpu.check(self.L.jpegx_entropy_block_sizes(self.dws.ptr, self.nblk, per_block.ctypes.data, None))
            zz = self.dzz.download((self.nplanes, self.bpp * nn), np.int32).astype(np.int64)
            sizes[:, q] = per_block.reshape(self.nplanes, self.bpp).sum(axis=1)
            bad[:, q] = (np.abs(zz) > 16383).any(axis=1)
        return sizes, bad

    def check(self, mode, params, expect_bad=False):
        got, got_bad = self.probe(mode, params)
        want, want_bad = self.yardstick(mode, params)
        assert np.array_equal(got_bad, want_bad), (self.n, params)
        assert want_bad.any() == expect_bad, (self.n, params)
        assert np.array_equal(got[~want_bad], want[~want_bad]), (self.n, params, got, want)
        again, again_bad = self.probe(mode, params)                        # two calls in a row: identical totals
        assert np.array_equal(again[~want_bad], got[~want_bad]) and np.array_equal(again_bad, got_bad)
        return got

    def free(self):
        for b in (self.din, self.dzz, self.dws):
            b.free()


@pytest.fixture(scope="module", params=SIZES)
def shapes(request, gpu):
    """Per dct_size: 3 planes of 2 x 3 blocks at pitch W and 7 planes of 5 x 7 blocks at a larger pitch, and one lone plane."""
    n = request.param
    devs = [Device(gpu, _planes(gpu, n, 2, 3, 3), n), Device(gpu, _planes(gpu, n, 5, 7, 7, seed=1), n, pad=5),
            Device(gpu, _planes(gpu, n, 5, 7, 1, seed=2), n, pad=1)]
    yield n, devs
    for d in devs:
        d.free()


def test_divide_candidates(shapes):
    n, devs = shapes
    for d in devs:
        d.check(DIVIDE, [40.0])
        got = d.check(DIVIDE, [1.0, 2.0, 3.0, 40.0, 64.0, 1000.0])         # power-of-two and true-division paths side by side
        assert (got >= d.bpp).all()                                    # a block is one byte at least
    # all-zero planes (planes 2 and 6 of the second stack): one byte per block under every candidate
    got = devs[1].check(DIVIDE, [1.0, 7.0])
    assert (got[[2, 6]] == devs[1].bpp).all() and (got[[0, 1, 3, 4, 5]] > devs[1].bpp).all()


def test_the_same_value_twice_and_thirty_two_candidates(shapes):
    n, devs = shapes
    got = devs[1].check(DIVIDE, [40.0, 3.0, 40.0])
    assert np.array_equal(got[:, 0], got[:, 2])
    many = [float(v) for v in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128, 160, 200, 256, 300, 400, 512, 640,
                               800, 1000, 2000, 4096, 100000)]
    assert len(many) == 32
    got = devs[0].check(DIVIDE, many)
    assert (got[:, -1] == devs[0].bpp).all()                              # everything quantised away


def test_discard(shapes):
    n, devs = shapes
    for d in devs[:2]:
        got = d.check(DISCARD, [0.0, 1.0, float(n), float(n + 1)])
        assert (got[:, 0] == d.bpp).all() and np.array_equal(got[:, 2], got[:, 3])


def test_none_takes_one_candidate(shapes):
    n, devs = shapes
    devs[1].check(NONE, [0.0])


@pytest.mark.parametrize("n", [2, 7, 16])
def test_bit_63_for_exactly_the_bad_planes_and_candidates(gpu, n):
    """Divisor 0.001 beside 40: the noisy, ramp and speck planes pass 16383 under 0.001, the all-zero planes do not, and nothing
    does under 40; the totals of the clean candidate stay right."""
    d = Device(gpu, _planes(gpu, n, 5, 7, 7, seed=1), n, pad=2)
    try:
        got, bad = d.probe(DIVIDE, [0.001, 40.0])
        want, want_bad = d.yardstick(DIVIDE, [0.001, 40.0])
        assert np.array_equal(bad, want_bad)
        assert not bad[:, 1].any() and bad[:, 0].any() and not bad[:, 0].all()
        assert np.array_equal(got[:, 1], want[:, 1]) and np.array_equal(got[~bad], want[~bad])
    finally:
        d.free()


def test_explicit_device_form(gpu):
    d = Device(gpu, _planes(gpu, 4, 2, 3, 3), 4)
    try:
        dtot = gpu.DeviceBuffer(3 * 2 * 8)
        gpu.probe_sizes_n_device(d.din.ptr, 3, d.h, d.w, 4, DIVIDE, [3.0, 40.0], dtot.ptr, device=0)
        gpu.check(d.L.jpegx_stream_synchronize(None))
        assert np.array_equal(dtot.download((3, 2), np.uint64), d.yardstick(DIVIDE, [3.0, 40.0])[0])
        dtot.free()
    finally:
        d.free()
