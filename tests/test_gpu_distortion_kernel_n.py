"""jpegx_probe_distortion_n against the road it stands for, run once per candidate on the same planes (tests/distortion_device.py:
jpegx_forward_fused_n, jpegx_inverse_fused_n with the uint8 clamp, jpegx_inflate_crop_stacked_u8, NumPy's sum of squares against
the bands), and jpegx_band_moments_packed_stacked_n against its NumPy twin (tests/distortion_model.py).  Every comparison is
exact: the bands are 8-bit noise, rounding ties included, because the probe repeats the road's arithmetic.

Sizes 2..32 cover 64..1 blocks per turn and the strided passes from 17 up.  Per size: 70 planes of a single block (at N = 2 a
turn spans 64 planes, at N <= 7 several, and a wave of the reduction several from N = 2 to 5) at block_size 2, and three planes of
3 x 4 blocks at block_size 1 and 3, every band ragged -- a partial last tile and a pooled size that is no multiple of N."""
import numpy as np
import pytest

import distortion_model as dm
from distortion_device import Stack

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 4, 7, 9, 12, 16, 17, 24, 32]
MANY = [1, 2, 3, 4, 5, 6, 7, 8, -10, 12, 16, 20, 24, 32, -40, 48, 64, 80, 96, 128, 0.75, 0.5, -0.25, 0.3, 300, 400, 512, 640, -800, 1000,
        2000, 4096]


def _ragged(n, hb, wb, bs):
    """(rows, cols) of a band of hb x wb blocks whose last block row and column hold one sample of DCT padding and, for bs > 1,
    whose last tile is partial."""
    pr, pc = hb * n - 1, wb * n - 1
    return pr * bs - (bs - 1), pc * bs - (1 if bs > 1 else 0)


def _bands(n, nplanes, rows, cols, seed):
    return np.random.default_rng([n, nplanes, seed]).integers(0, 256, (nplanes, rows, cols), dtype=np.uint8)


@pytest.fixture(scope="module", params=SIZES)
def stacks(request, gpu):
    n = request.param
    made = [Stack(gpu, _bands(n, 70, *_ragged(n, 1, 1, 2), 1), 2, n, pad=3),
            Stack(gpu, _bands(n, 3, *_ragged(n, 3, 4, 1), 2), 1, n, mpad=5),
            Stack(gpu, _bands(n, 3, *_ragged(n, 3, 4, 3), 3), 3, n, pad=1, mpad=2)]
    assert [s.bpp for s in made] == [1, 12, 12]
    yield n, made
    for s in made:
        s.free()


def test_divide_one_five_and_thirty_two_candidates(stacks):
    n, made = stacks
    assert len(MANY) == 32
    for s in made:
        s.check("divide", [40.0], label="K 1")
        got, bad = s.check("divide", [3.0, -40.0, 64.0, 0.75, 1000.0], label="K 5")
        assert s.bpp == 1 or (got[:, 4] > got[:, 1]).all()                # 1000 loses more than 40 on noise
        got, bad = s.check("divide", [float(v) for v in MANY], label="K 32")
        assert not bad[:, 14:20].any()                                    # -40 .. 128 code at every size
    got, _ = made[1].check("divide", [40.0, 3.0, 40.0], label="twice")
    assert np.array_equal(got[:, 0], got[:, 2])


def test_discard_edges_and_none(stacks):
    n, made = stacks
    amp = min(255, 16383 // (n * n))                                              # a band whose DC codes without a divisor
    for s in made[:2]:
        dark = Stack(s.gpu, (s.bands.astype(np.int64) * amp // 255).astype(np.uint8), s.bs, n, pad=2)
        try:
            got, bad = dark.check("discard", [0.0, 1.0, 2.0, float(n), float(n + 3)], label="discard")
            assert not bad.any() and np.array_equal(got[:, 3], got[:, 4])
            # keep 0 decodes to zeros: the error is the band's own sum of squares
            assert np.array_equal(got[:, 0], (dark.bands.astype(np.int64) ** 2).sum(axis=(1, 2)))
            got, bad = dark.check("none", [0.0], label="none")
            assert not bad.any() and np.array_equal(got[:, 0], dark.check("discard", [float(n)])[0][:, 0])
        finally:
            dark.free()


@pytest.mark.parametrize("n", [4, 16])
def test_bit_63_for_exactly_the_bad_plane_and_candidate(gpu, n):
    """Three planes of 3 x 4 blocks: noise up to 40, a plane of 255s whose DC is 20000 under the first divisor, noise again.  Bit 63
    for (plane 1, candidate 0) alone; every other cell equals the road."""
    rows, cols = _ragged(n, 3, 4, 1)
    bands = _bands(n, 3, rows, cols, 4) % 41
    bands[1] = 255
    s = Stack(gpu, bands, 1, n)
    try:
        params = [255.0 * n * n / 20000.0, 40.0]
        got, bad = s.check("divide", params, label="bad")
        assert np.argwhere(bad).tolist() == [[1, 0]]
    finally:
        s.free()


def test_explicit_device_form(gpu):
    s = Stack(gpu, _bands(4, 3, *_ragged(4, 3, 4, 2), 5), 2, 4)
    try:
        got, bad = s.probe("divide", [3.0, 40.0], device=0)
        want, want_bad = s.road("divide", [3.0, 40.0])
        assert np.array_equal(got, want) and np.array_equal(bad, want_bad)
    finally:
        s.free()


@pytest.mark.parametrize("colour", [0, 1])
@pytest.mark.parametrize("bs, n, rows, cols", [(1, 4, 13, 18), (2, 3, 15, 22), (3, 16, 67, 93), (7, 2, 30, 1), (255, 2, 300, 260)])
def test_moments_against_the_twin(gpu, colour, bs, n, rows, cols):
    """Two pictures of three bands at a pitch with a gap; with colour 1 the moments are those of Pillow's YCbCr."""
    pixels = np.random.default_rng([bs, n, colour]).integers(0, 256, (2, rows, cols, 3), dtype=np.uint8)
    pitch = cols * 3 + 5
    padded = np.full((2 * rows, pitch), 255, np.uint8)
    padded[:, :cols * 3] = pixels.reshape(2 * rows, cols * 3)
    h, w = dm.blocked_shape(rows, cols, bs, n)
    assert gpu.band_shape_n(rows, cols, bs, n) == (h, w)
    din, dout = gpu.DeviceBuffer(padded.nbytes), gpu.DeviceBuffer(2 * 3 * h * (w + 3) * 8)
    try:
        din.upload(padded)
        dout.upload(np.full((6 * h, w + 3), np.uint64(0xABABABABABABABAB)))
        gpu.band_moments_packed_stacked_n_device(din.ptr, 2, 3, rows, cols, bs, n, dout.ptr, colour=colour, pitch=pitch, out_pitch=w + 3)
        gpu.check(gpu.lib().jpegx_stream_synchronize(None))
        got = dout.download((6 * h, w + 3), np.uint64)
    finally:
        din.free()
        dout.free()
    assert (got[:, w:] == np.uint64(0xABABABABABABABAB)).all()            # nothing written into the pitch gap
    got = got[:, :w].reshape(2, 3, h, w)
    coded = dm.ycbcr(pixels) if colour else pixels
    for p in range(2):
        for k in range(3):
            s1, s2, cnt = dm.moments(coded[p, :, :, k], bs, n)
            assert np.array_equal(got[p, k], dm.pack(s1, s2)), (p, k)
            assert not got[p, k][cnt == 0].any()
